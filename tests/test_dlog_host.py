"""bjj_dlog without a GPU: the per-lane bodies of csrc/dlog.hpp -- what k_dlog.hip launches -- run on the CPU by the stand-alone
program tests/dlog_emul (bound assertions on, and a slot policy that refuses a slot outside the table): the table built thread by
thread with the build body, the check bodies over it (and over a table with one flipped bit), the search body over directed and
random items, each search once in one go and once cut into launches of three giant steps, everything with the kernels' 32-bit tags
and again with 3-bit tags that force false tag hits.  Expected values: the pure-Python oracle.  The same program runs once more
built with -fsanitize=address,undefined, directly (no preload)."""
import os
import subprocess

import pytest

import dlog_cases as dc
from conftest import ROOT, ints

SRC = os.path.join(ROOT, "tests", "dlog_emul", "dlog_emul.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "babyjubjub-rs_amd", "csrc", f)
                for f in ("fr.hpp", "fr_mul_columns.inc", "curve.hpp", "bjj_device.hpp", "dlog.hpp", "bjj_constants.inc")]
TABLES = [("b8", 4), ("b8", 6), ("order_8l", 4), ("order_8l", 6)]


def _build(exe, san):
    if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in DEPS):
        return None
    extra = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if san else ["-O2"]
    return subprocess.run(["g++", "-g", "-std=c++17"] + extra + ["-o", exe, SRC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


@pytest.fixture(scope="module")
def inputs(pyoracle, golden):
    """per table: the program's stdin, the cases and the ranges -- computed once"""
    o = pyoracle
    tors = [ints(t) for t in golden["gpu_expected"]["torsion_points"]]
    add = lambda p, q: o.proj_affine(o.proj_add((p[0], p[1], 1), (q[0], q[1], 1)))
    mul = lambda P, ks: [o.mul_scalar(P, k) for k in ks]
    bases = {"b8": o.B8, "order_8l": add(o.mul_scalar(o.B8, 0x1234567), tors[1])}
    assert o.mul_scalar(bases["order_8l"], o.SUBORDER) != (0, 1) and o.mul_scalar(bases["order_8l"], o.ORDER) == (0, 1)
    out = {}
    for name, b in TABLES:
        ranges = [3, b, 12]
        G = bases[name]
        cases = dc.interleave(dc.build(mul, add, G, b, ranges, tors[1], 0xD106 + b))
        assert all(o.on_curve((x % dc.Q, y)) == (t != dc.OFF_CURVE) for (x, y), t in cases)
        text = "G %x %x\nT %d 3\nR %d %s\nI %d\n%s\n" % (G[0] + (dc.Q if name == "order_8l" else 0), G[1], b, len(ranges),
                                                         " ".join(map(str, ranges)), len(cases), "\n".join("%x %x" % rec for rec, _ in cases))
        out[(name, b)] = {"text": text, "cases": cases, "ranges": ranges, "G": G}
    return out


def _check_output(out, inp, b):
    facts = {"r": {}, "s": {}, "check": {}, "flip": {}, "rejected": {}, "walked": {}}
    for line in out.split("\n"):
        f = line.split()
        if not f:
            continue
        if f[0] in ("r", "s"):
            facts[f[0]].setdefault((int(f[1]), int(f[2])), []).append((int(f[3]), int(f[4]), int(f[5], 16)))
            if f[0] == "s":
                facts["walked"][(int(f[1]), int(f[2]), int(f[3]))] = int(f[6])
        elif f[0] == "check":
            facts["check"][int(f[1])] = (int(f[2]), int(f[3]))
        elif f[0] == "flip":
            facts["flip"][(int(f[1]), f[2])] = int(f[3])
        elif f[0] == "rejected":
            facts["rejected"][int(f[1])] = int(f[2])
        elif f[0] == "small":
            assert f[1] == "0"
        elif f[0] == "base":
            assert (int(f[1], 16), int(f[2], 16)) == inp["G"]           # reduced mod r
    n = len(inp["cases"])
    for tag_bits in (32, 3):
        assert facts["check"][tag_bits] == (0, (1 << b) + 1)            # sound, and 2^b + 1 occupied slots
        assert facts["flip"][(tag_bits, "tag")] > 0 and facts["flip"][(tag_bits, "j")] > 0
        for rb in inp["ranges"]:
            want_m, want_ok = dc.expected(inp["cases"], rb)
            for kind in ("r", "s"):
                got = facts[kind][(tag_bits, rb)]
                assert [i for i, _, _ in got] == list(range(n))
                bad = [(i, ok, m, want_ok[i], want_m[i], inp["cases"][i][1]) for i, ok, m in got if (ok, m) != (want_ok[i], want_m[i])]
                assert not bad, (kind, tag_bits, rb, bad[:8])
    # a cut call walks a decided item no further: one whose m lies in the first window, found or confirmed beyond the range, and
    # one off the curve take part in the first launch alone; an item that is never found takes part in all of them
    stride, launches = 2 << b, -(-max(1, (1 << 12) // (2 << b)) // 3)
    assert launches > 1
    for i, (_, truth) in enumerate(inp["cases"]):
        for tag_bits in (32, 3):
            w12 = facts["walked"][(tag_bits, 12, i)]
            if truth == dc.OFF_CURVE or (isinstance(truth, int) and truth < stride):
                assert w12 == 1, (i, truth, w12)
            elif truth == dc.NOT_IN_RANGE:
                assert w12 == launches, (i, truth, w12)
    beyond = [i for i, (_, t) in enumerate(inp["cases"]) if isinstance(t, int) and (1 << 3) <= t < stride]
    assert beyond and all(facts["walked"][(32, 3, i)] == 1 for i in beyond)
    # the 3-bit instantiation proves something only if confirmation had false hits to refuse
    assert facts["rejected"][3] > 0
    # every kind of outcome occurs
    assert {2, 1, 0} == set(dc.expected(inp["cases"], 12)[1])


@pytest.mark.parametrize("name,b", TABLES)
def test_results_match_the_python_oracle(inputs, name, b):
    exe = os.path.join(ROOT, "tests", "dlog_emul", "dlog_emul")
    c = _build(exe, False)
    assert c is None or c.returncode == 0, c.stdout
    r = subprocess.run([exe], input=inputs[(name, b)]["text"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    _check_output(r.stdout, inputs[(name, b)], b)


def test_a_base_of_small_order_is_reported(golden):
    exe = os.path.join(ROOT, "tests", "dlog_emul", "dlog_emul")
    c = _build(exe, False)
    assert c is None or c.returncode == 0, c.stdout
    for t in golden["gpu_expected"]["torsion_points"]:                  # the identity and the seven other points of order <= 8
        x, y = ints(t)
        r = subprocess.run([exe], input="G %x %x\nT 4 3\nR 1 4\nI 0\n" % (x, y), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.split("\n")[0] == "small 1", (t, r.stdout, r.stderr)


@pytest.mark.parametrize("name,b", [("b8", 4), ("order_8l", 6)])
def test_the_same_program_under_asan_and_ubsan(inputs, name, b):
    for rt in ("libasan.so", "libubsan.so"):     # asked of the toolchain BEFORE the build: a build that fails is a failure
        path = subprocess.run(["g++", "-print-file-name=" + rt], stdout=subprocess.PIPE, text=True).stdout.strip()
        if not os.path.isabs(path) or not os.path.exists(path):
            pytest.skip("no %s in this toolchain" % rt)
    exe = os.path.join(ROOT, "tests", "dlog_emul", "dlog_emul_san")
    c = _build(exe, True)
    assert c is None or c.returncode == 0, c.stdout
    r = subprocess.run([exe], input=inputs[(name, b)]["text"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1200,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0, r.stdout[-3000:]
    assert "AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
    _check_output(r.stdout, inputs[(name, b)], b)
