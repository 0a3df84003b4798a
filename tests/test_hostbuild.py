"""tests/hostbuild.py itself, on a two-file toy program in tmp_path: the rebuild rule is the compiler's own list of what a
translation unit read (-MMD), a compile failure is an exception that carries the compiler's message, and run_sanitized fails on a
heap read one element past an array (a host program; nothing here touches a GPU)."""
import os

import pytest

import hostbuild

HEADER = "static int answer() { return %d; }\n"
MAIN = '#include <stdio.h>\n#include "toy.hpp"\nint main() { printf("%d\\n", answer()); return 0; }\n'
OVERRUN = ("#include <stdio.h>\n#include <stdlib.h>\n"
           "int main(int argc, char**) { int* a = (int*)malloc(4 * sizeof(int)); for (int i = 0; i < 4; i++) a[i] = i;\n"
           "  volatile int i = 3 + argc; int v = a[i]; printf(\"%d\\n\", v); free(a); return 0; }\n")


def _later(path, than):
    """gives `path` an mtime clearly after that of `than`, whatever the granularity of the file system's clock"""
    t = os.path.getmtime(than) + 10
    os.utime(path, (t, t))


@pytest.fixture
def toy(tmp_path):
    (tmp_path / "toy.hpp").write_text(HEADER % 41)
    (tmp_path / "toy.cpp").write_text(MAIN)
    return tmp_path


def _build(toy):
    return hostbuild.program("toy", str(toy / "toy.cpp"), build_dir=str(toy / "_build"))


def test_an_unchanged_tree_is_not_rebuilt(toy):
    exe = _build(toy)
    assert hostbuild.run(exe) == "41\n"
    os.utime(exe, (1000, 1000))                    # a rebuild would give it today's mtime; the sources are older still
    for f in ("toy.cpp", "toy.hpp"):
        os.utime(str(toy / f), (500, 500))
    assert _build(toy) == exe and os.path.getmtime(exe) == 1000


def test_touching_the_included_header_rebuilds(toy):
    exe = _build(toy)
    (toy / "toy.hpp").write_text(HEADER % 42)      # not named anywhere but in the depfile
    _later(str(toy / "toy.hpp"), exe)
    assert hostbuild.run(_build(toy)) == "42\n"


def test_deleting_the_depfile_rebuilds(toy):
    exe = _build(toy)
    os.utime(exe, (1000, 1000))
    for f in ("toy.cpp", "toy.hpp"):
        os.utime(str(toy / f), (500, 500))
    deps = [f for f in os.listdir(str(toy / "_build")) if f.endswith(".d")]
    assert len(deps) == 1
    os.remove(str(toy / "_build" / deps[0]))
    assert _build(toy) == exe and os.path.getmtime(exe) > 1000 and os.path.exists(str(toy / "_build" / deps[0]))


def test_a_syntax_error_raises_with_the_compilers_message(toy):
    (toy / "toy.hpp").write_text("static int answer() { return 41 }\n")
    with pytest.raises(hostbuild.BuildError) as e:
        _build(toy)
    assert "toy.hpp" in str(e.value) and "expected" in str(e.value)


def test_shared_builds_a_library_ctypes_can_load(toy):
    import ctypes
    (toy / "lib.cpp").write_text('#include "toy.hpp"\nextern "C" int toy_answer() { return answer() + VALUE; }\n')
    so = hostbuild.shared("libtoy.so", str(toy / "lib.cpp"), defines=("VALUE=1",), build_dir=str(toy / "_build"))
    assert ctypes.CDLL(so).toy_answer() == 42


def test_run_sanitized_fails_on_a_heap_read_past_the_end(toy):
    hostbuild.need_sanitizer_runtimes()
    (toy / "overrun.cpp").write_text(OVERRUN)
    exe = hostbuild.program("overrun_san", str(toy / "overrun.cpp"), san=True, build_dir=str(toy / "_build"))
    with pytest.raises(AssertionError) as e:
        hostbuild.run_sanitized(exe, timeout=60)
    assert "AddressSanitizer" in str(e.value) or "runtime error" in str(e.value)     # whichever of the two sees the load first
    (toy / "fine.cpp").write_text(OVERRUN.replace("3 + argc", "2 + argc"))
    assert hostbuild.run_sanitized(hostbuild.program("fine_san", str(toy / "fine.cpp"), san=True, build_dir=str(toy / "_build")), timeout=60) == "3\n"
