"""Building and running the host programs of the CPU harnesses (tests/*_emul, tests/emul): one g++ line, one rebuild rule, one way
to run a program under AddressSanitizer + UndefinedBehaviorSanitizer.  Imported by the test modules; not a conftest.

The rebuild rule is derived, not listed: every translation unit is compiled with -MMD -MF, and a product is rebuilt when it or one
of its depfiles is missing or when any file a depfile names -- the source and everything it includes, transitively -- is newer
than the product.  Products go to tests/_build/ (ignored by git).  (tests/conftest.py builds tests/emul/emul_bodies.cpp itself, by
its own rule.)"""
import os
import subprocess

import pytest

BUILD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_build")
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}


class BuildError(RuntimeError):
    """the compiler's exit status was not 0; the text is its output"""


def _dep_files(depfile):
    """the prerequisites of a make rule as g++ -MMD writes it: target: file file \\<newline> file ..."""
    with open(depfile) as f:
        text = f.read().replace("\\\n", " ")
    return text.split(":", 1)[1].split()


def _stale(out, depfiles):
    try:
        built = os.path.getmtime(out)
        return any(os.path.getmtime(f) > built for d in depfiles for f in _dep_files(d))
    except (OSError, IndexError):           # the product, a depfile or a file it names is gone
        return True


def _build(out, sources, flags, link_flags=()):
    sources = [sources] if isinstance(sources, str) else list(sources)
    objs = ["%s.%d.o" % (out, i) for i in range(len(sources))]
    deps = ["%s.%d.d" % (out, i) for i in range(len(sources))]
    if _stale(out, deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        cmds = [["g++", "-g", "-std=c++17"] + flags + ["-MMD", "-MF", d, "-c", "-o", o, s] for s, o, d in zip(sources, objs, deps)]
        cmds.append(["g++"] + flags + list(link_flags) + ["-o", out] + objs)
        for cmd in cmds:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0:
                raise BuildError("%s failed:\n%s" % (" ".join(cmd), r.stdout))
    return out


def _flags(san, defines, opt, extra):
    return [opt or ("-O1" if san else "-O2")] + ["-D" + d for d in defines] + list(extra) + (SAN_FLAGS if san else [])


def program(name, sources, *, san=False, defines=(), opt=None, extra=(), build_dir=BUILD_DIR):
    """the path of an up-to-date executable tests/_build/<name>; san: built with ASan + UBSan (-O1 unless `opt` says otherwise)"""
    return _build(os.path.join(build_dir, name), sources, _flags(san, defines, opt, extra))


def shared(name, sources, *, defines=(), opt=None, extra=(), build_dir=BUILD_DIR):
    """the path of an up-to-date shared library tests/_build/<name> for ctypes"""
    return _build(os.path.join(build_dir, name), sources, _flags(False, defines, opt, ["-fPIC"] + list(extra)), ["-shared"])


def need_sanitizer_runtimes():
    """skips the test when the toolchain has no libasan.so / libubsan.so.  Asked BEFORE the build: a build that fails is a failure"""
    for rt in ("libasan.so", "libubsan.so"):
        path = subprocess.run(["g++", "-print-file-name=" + rt], stdout=subprocess.PIPE, text=True).stdout.strip()
        if not os.path.isabs(path) or not os.path.exists(path):
            pytest.skip("no %s in this toolchain" % rt)


def run(exe, stdin_text=None, timeout=600):
    """stdout of a run that must end with status 0"""
    r = subprocess.run([exe], input=stdin_text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return r.stdout


def run_sanitized(exe, stdin_text=None, timeout=1200):
    """output (stdout and stderr) of a program built with san=True: leak detection on, the first finding ends the program, and the
    run must end with status 0 and without a report"""
    r = subprocess.run([exe], input=stdin_text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout,
                       env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, r.stdout[-3000:]
    assert "AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
    return r.stdout
