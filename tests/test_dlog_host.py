"""bjj_dlog without a GPU: the per-lane bodies of csrc/dlog.hpp -- what k_dlog.hip launches -- run on the CPU by the stand-alone
program tests/dlog_emul (bound assertions on, and a slot policy that refuses a slot outside the table): the table built thread by
thread with the build body, the check bodies over it (and over a table with one flipped bit), the search body over directed and
random items, each search once in one go and once cut into launches of three giant steps, everything with the kernels' 32-bit tags
and again with 3-bit tags that force false tag hits.  Expected values: the pure-Python oracle.  The same program runs once more
built with -fsanitize=address,undefined, directly (no preload).  Further down, the plain-integer model tests/dlog_ref.py is held
against the same program: its slots, and the tag hits it refuses per item, for constructed false hits and a wrapped probe run."""
import os
import random
import subprocess

import pytest

import hostbuild
import dlog_cases as dc
import dlog_ref as dr
from conftest import ROOT, ints

SRC = os.path.join(ROOT, "tests", "dlog_emul", "dlog_emul.cpp")
TABLES = [("b8", 4), ("b8", 6), ("order_8l", 4), ("order_8l", 6)]


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
    _check_output(hostbuild.run(hostbuild.program("dlog_emul", SRC), inputs[(name, b)]["text"]), inputs[(name, b)], b)


def test_a_base_of_small_order_is_reported(golden):
    exe = hostbuild.program("dlog_emul", SRC)
    for t in golden["gpu_expected"]["torsion_points"]:                  # the identity and the seven other points of order <= 8
        x, y = ints(t)
        out = hostbuild.run(exe, "G %x %x\nT 4 3\nR 1 4\nI 0\n" % (x, y), timeout=60)
        assert out.split("\n")[0] == "small 1", (t, out)


@pytest.mark.parametrize("name,b", [("b8", 4), ("order_8l", 6)])
def test_the_same_program_under_asan_and_ubsan(inputs, name, b):
    hostbuild.need_sanitizer_runtimes()          # BEFORE the build: a build that fails is a failure
    out = hostbuild.run_sanitized(hostbuild.program("dlog_emul_san", SRC, san=True), inputs[(name, b)]["text"])
    _check_output(out, inputs[(name, b)], b)


# ---- constructed false hits and a wrapped probe run: the plain-integer model tests/dlog_ref.py against the source ---------------------
DIRECTED = [("b8", 4, 12), ("b8", 8, 14), ("order_8l", 6, 12)]


def _emul(text):
    out = hostbuild.run(hostbuild.program("dlog_emul", SRC), text)
    f = {"r": {}, "s": {}, "check": {}, "rejected": {}, "slots": {}}
    for line in out.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "r":       # (tag_bits, range_bits) -> [(ok, m, refused)] in item order
            f["r"].setdefault((int(w[1]), int(w[2])), []).append((int(w[4]), int(w[5], 16), int(w[6])))
        elif w[0] == "s":
            f["s"].setdefault((int(w[1]), int(w[2])), []).append((int(w[4]), int(w[5], 16), int(w[7])))
        elif w[0] == "check":
            f["check"][int(w[1])] = (int(w[2]), int(w[3]))
        elif w[0] == "rejected":
            f["rejected"][int(w[1])] = int(w[2])
        elif w[0] == "slots":
            f["slots"][int(w[1])] = {int(a): int(b) - 1 for a, b in (x.split(":") for x in w[2:])}
    return f


def _text(G, b, ranges, recs):
    return "G %x %x\nT %d 3\nR %d %s\nI %d\n%s\n" % (G[0], G[1], b, len(ranges), " ".join(map(str, ranges)), len(recs),
                                                     "\n".join("%x %x" % rec for rec in recs))


def _multiples(o, G, count):
    """{m * G: m} for m < count, by the Python oracle's addition: the definition of 'has a logarithm in the range'"""
    out, acc = {}, (0, 1)
    for m in range(count):
        out[acc] = m
        acc = o.proj_affine(o.proj_add((acc[0], acc[1], 1), (G[0], G[1], 1)))
    return out


def _base(o, golden, name):
    if name == "b8":
        return o.B8
    T1 = ints(golden["gpu_expected"]["torsion_points"][1])
    return o.proj_affine(o.proj_add(o.mul_scalar(o.B8, 0x1234567) + (1,), (T1[0], T1[1], 1)))


def test_the_model_of_the_table():
    """the occupied slots depend on the homes alone, not on who came first; craft() hits the index and the tag it is asked for"""
    rng = random.Random(0x51075)
    for b in (4, 8):
        T = dr.table(dr.mul((5299619240641551281634865583518297030282874472190772894086521144482721001553,
                             16950150798460657717958625567821834550301663161624707787222815936182638968203), 3), b)
        order = list(range(len(T.homes)))
        for _ in range(3):
            rng.shuffle(order)
            assert dr.occupied(T.homes, T.nslots, order) == T.occ and set(T.layout(order)) == T.occ
        for _ in range(20):
            idx, tag = rng.randrange(T.nslots), rng.getrandbits(32)
            Q = dr.craft(idx, tag, b, rng)
            assert dr.on_curve(Q) and dr.idx_of(dr.key(Q), b) == idx and dr.tag_of(dr.key(Q)) == tag and dr.key(Q) < dr.R


@pytest.mark.parametrize("name,b,rb", DIRECTED)
def test_constructed_false_hits_are_refused_as_the_model_counts(pyoracle, golden, name, b, rb):
    """Items built to collide, at a chosen giant step, with an entry's index run and full 32-bit tag while their y is no entry's: the
    model says which candidate each walk refuses, the program's per-item counts must equal it exactly -- with 32-bit tags, where
    only the constructed hits exist, and with 3-bit tags, where the model walks the table laid out as the program builds it -- and
    every item ends not found, in one go and cut into launches of three steps (steps 2 and 3: the last of a launch, the first of the
    next).  Not found is the definition's verdict: P is none of m * G, m < 2^range_bits, by the oracle."""
    o = pyoracle
    G = _base(o, golden, name)
    T = dr.table(G, b)
    items = dr.false_hit_items(T, rb, (2, 3, 5, 6), random.Random(0xFA15E + b))
    want32 = [dr.assert_false_hit(T, it, rb) for it in items]
    assert sum(want32) == len(items) - 2 and {it["kind"] for it in items} == {"first", "behind"}
    known = _multiples(o, G, 1 << rb)
    assert known[o.mul_scalar(G, 77)] == 77 and all(it["P"] not in known and o.on_curve(it["P"]) for it in items)
    f = _emul(_text(G, b, [rb], [it["P"] for it in items]))
    lay = T.layout()
    for tb in (32, 3):
        assert f["check"][tb] == (0, (1 << b) + 1) and f["slots"][tb] == lay
        want = want32 if tb == 32 else [dr.refused_hits(it["P"], G, b, rb, 3, lay) for it in items]
        for kind in ("r", "s"):
            got = f[kind][(tb, rb)]
            assert [(ok, m) for ok, m, _ in got] == [(0, dr.UINT64_MAX)] * len(items), (kind, tb)
            assert [n for _, _, n in got] == want, (kind, tb)
        assert f["rejected"][tb] == sum(want)
    assert f["rejected"][32] == len(items) - 2


def test_a_probe_run_that_crosses_the_end_of_the_table(pyoracle):
    """161 * B8 at 4 baby bits: entries 7 and 9 are homed at the last slot and the run goes on over slots 0 .. 3 -- by the model, which
    looks for the first such base from 161 on and asserts the wrap of whatever it finds.  The table is sound, every m of four windows is found (7, 9 and their
    mirrors in the later windows among them), and false hits planted behind the wrap are refused."""
    o = pyoracle
    b, rb = 4, 8
    k, T = dr.wrapped_base(o.B8, b)
    G = T.G
    assert G == o.mul_scalar(o.B8, k) and T.wraps(T.mask) and T.run_from(T.mask)[:2] == [T.mask, 0] and T.mask in T.homes
    if k == 161:
        assert (T.homes[7], T.homes[9], T.run_from(63)) == (63, 63, [63, 0, 1, 2, 3])
    sites = dr.hit_sites(T)["wrapped"]
    rng = random.Random(0x3A9)
    items = [dict(zip(("P", "Q"), dr.false_hit_item(T, step, idx, e, rng)), step=step, idx=idx, e=e, kind="wrapped")
             for step, (idx, e) in zip((0, 2, 3, 7, 1), sites + sites)]
    assert all(dr.assert_false_hit(T, it, rb) == 1 for it in items)
    known = _multiples(o, G, 1 << rb)
    assert all(it["P"] not in known for it in items)
    pts = sorted(known, key=known.get)
    assert [known[p] for p in pts] == list(range(1 << rb))
    f = _emul(_text(G, b, [rb, 6], pts + [it["P"] for it in items]))
    lay = T.layout()
    for tb in (32, 3):
        assert f["check"][tb] == (0, (1 << b) + 1) and f["slots"][tb] == lay
        for range_bits in (rb, 6):
            for kind in ("r", "s"):
                got = f[kind][(tb, range_bits)]
                assert [(ok, m) for ok, m, _ in got[:1 << range_bits]] == [(1, m) for m in range(1 << range_bits)], (tb, range_bits, kind)
                assert all((ok, m) == (0, dr.UINT64_MAX) for ok, m, _ in got[1 << range_bits:])
        assert [n for _, _, n in f["r"][(32, rb)][1 << rb:]] == [1] * len(items) == [n for _, _, n in f["s"][(32, rb)][1 << rb:]]
        want3 = [dr.refused_hits(p, G, b, rb, 3, lay) for p in pts + [it["P"] for it in items]]
        assert [n for _, _, n in f["r"][(3, rb)]] == want3 == [n for _, _, n in f["s"][(3, rb)]]
    assert sum(want3) > len(items)


def test_the_test_build_of_the_kernel_unit_is_the_shipped_code():
    """tests/devfuzz/libbjj_dlog_test_tag32.so is csrc/k_dlog.hip with the shipped tag width: the machine code of its five kernels is
    that of libbjj_hip.so, so what the 3-bit build differs in is the tag width alone (the three kernels that read a tag)"""
    from babyjubjub_rs_amd import srchash
    d = os.path.join(ROOT, "tests", "devfuzz")
    r = subprocess.run(["make", "-s", "libbjj_dlog_test_tag3.so", "libbjj_dlog_test_tag32.so"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    names = ["bjj_k_dlog_" + k for k in ("setup", "build", "check_entries", "check_slots", "search")]
    shipped = srchash.kernel_hashes()
    t32 = srchash.kernel_hashes(os.path.join(d, "libbjj_dlog_test_tag32.so"))
    t3 = srchash.kernel_hashes(os.path.join(d, "libbjj_dlog_test_tag3.so"))
    assert sorted(t32) == sorted(t3) == sorted(names) and all(shipped[k] for k in names)
    assert {k: shipped[k] for k in names} == t32
    assert {k for k in names if t3[k] != t32[k]} == {"bjj_k_dlog_build", "bjj_k_dlog_check_entries", "bjj_k_dlog_search"}
