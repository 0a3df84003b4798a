"""bjj_mul_bases without a GPU: the table code and the per-item body of csrc/bases.hpp -- what k_bases.hip launches -- run on the
CPU by the stand-alone program tests/bases_emul (bound assertions on).  Tables for B8 + T8, a generator of the whole group of
order 8l, at W = 4, 5 and 12, for the order-2 point (0, -1) at W = 4 and for B8 as a context's own table; every one passes the
generalised induction check, and every result for t = 1, 2, 3 bases is the oracle's: mul_var_base per term, folded with point_add.
The same program runs once more built with -fsanitize=address,undefined, directly (no preload)."""
import os

import numpy as np
import pytest

import hostbuild
from bases_cases import directed, random_scalars
from conftest import ROOT, ints, pack, unpack

Q = 21888242871839275222246405745257275088548364400416034343698204186575808495617
B8 = (5299619240641551281634865583518297030282874472190772894086521144482721001553,
      16950150798460657717958625567821834550301663161624707787222815936182638968203)
SRC = os.path.join(ROOT, "tests", "bases_emul", "bases_emul.cpp")
# the cases bases_emul.cpp runs: name -> its tables; the scalar of base j for item i is S[(i + 7 j) % count]
CASES = {"p4": "P", "p5": "P", "p12": "P", "two4": "2", "b8": "B", "p4+p12": "PP", "b8+p5": "BP", "two4+p4": "2P", "p12+b8": "PB",
         "p12+b8+two4": "PB2", "p4+p4+p5": "PPP"}


@pytest.fixture(scope="module")
def inputs(oracle, golden):
    tors = [ints(t) for t in golden["gpu_expected"]["torsion_points"]]
    gen = unpack(oracle.point_add(pack([B8]), pack([tors[1]])), 2)[0]          # B8 + T8: order 8l
    sc = directed((4, 5, 12)) + unpack(random_scalars(200, 0xBA5E5))
    text = "P %x %x\nS %d\n%s\n" % (gen[0], gen[1], len(sc), "\n".join("%x" % k for k in sc))
    return {"P": gen, "2": tors[4], "B": B8}, sc, text


@pytest.fixture(scope="module")
def expected(oracle, inputs):
    """per case the oracle's results, computed once: one mul_var_base per distinct point over all scalars, folded with point_add"""
    points, sc, _ = inputs
    n = len(sc)
    S = pack(sc).reshape(n, 32)
    prod = {k: oracle.mul_var_base(np.tile(pack([p]), n), S) for k, p in points.items()}
    want = {}
    for name, tbls in CASES.items():
        acc = pack([(0, 1)] * n).reshape(n, 64)
        for j, k in enumerate(tbls):
            idx = [(i + 7 * j) % n for i in range(n)]
            acc = oracle.point_add(acc, prod[k][idx])
        want[name] = unpack(acc, 2)
    return want


def _check_output(out, inputs, expected):
    points, sc, _ = inputs
    lines = out.split("\n")
    facts = {}
    for l in lines:
        f = l.split()
        if f and f[0] in ("check", "entry", "anchor", "corrupt"):
            facts.setdefault(f[0], []).append((int(f[1]), int(f[2])))
    assert sorted(set(facts["check"])) == [(i, 0) for i in range(5)] and len(facts["check"]) == 6    # table 1 again after the repair
    assert sorted(facts["entry"]) == [(i, 0) for i in range(5)]
    assert all(bad > 0 for _, bad in facts["anchor"]) and len(facts["anchor"]) == 2
    assert facts["corrupt"][0][0] == 1 and facts["corrupt"][0][1] > 0
    got = {}
    for l in lines:
        f = l.split()
        if f and f[0] == "r":
            got.setdefault(f[1], []).append((int(f[2]), (int(f[3], 16), int(f[4], 16))))
    assert sorted(got) == sorted(CASES)
    for name in CASES:
        assert [i for i, _ in got[name]] == list(range(len(sc))), name
        for i, xy in got[name]:
            assert xy == expected[name][i], (name, i, hex(sc[i]))


def test_window_counts_and_patterns():
    from bases_cases import ORDER8, base_windows, pattern
    assert [base_windows(W) for W in (4, 5, 12, 16, 23, 28)] == [64, 51, 22, 16, 12, 10]
    assert ORDER8 < 1 << 254
    for W in (4, 5, 12, 16):
        for d in (1 << (W - 1), (1 << (W - 1)) + 1):
            v = pattern(W, d)
            assert v < ORDER8 and v & ((1 << W) - 1) == d and v >> (W * (base_windows(W) - 3)) != 0


def signed_digits(v, W, nwin):
    """digit_next of csrc/bjj_device.hpp in plain integers: u = low W bits + carry; u > 2^(W-1) becomes u - 2^W and carries one
    into the next window (u == 2^W is digit 0 with a carry) -> (the nwin digits, the carry that leaves the top window)"""
    digits, carry = [], 0
    for _ in range(nwin):
        u = (v & ((1 << W) - 1)) + carry
        carry = 1 if u > 1 << (W - 1) else 0
        digits.append(u - (carry << W))
        v >>= W
    assert v == 0                                          # every bit of the scalar lies inside the windows
    return digits, carry


@pytest.mark.parametrize("W", range(4, 29))
def test_signed_recoding_fits_the_windows_of_every_width(W):
    """the argument of csrc/bases.hpp, lines 5-9, for every width bjj_base_create accepts: a scalar below 8l < 2^254 recoded over
    base_windows(W) = ceil(255 / W) windows sums back to itself, its top digit is non-negative and no carry leaves the top window;
    every digit is a slot of the window, |d| <= 2^(W-1).  tests/bases_emul prints results, not digits, so the shipped digit_next
    is held against this model through its results only (test_tables_and_results_match_the_oracle, W = 4, 5, 12)."""
    from bases_cases import ORDER8, base_windows, pattern
    nwin = base_windows(W)
    assert nwin * W >= 255 > (nwin - 1) * W
    half = 1 << (W - 1)
    rng = np.random.default_rng(0xD161 + W)
    seeded = [int.from_bytes(rng.bytes(32), "little") % ORDER8 for _ in range(1000)]
    for v in [ORDER8 - 1, pattern(W, half), pattern(W, half + 1)] + seeded:
        assert v < ORDER8
        digits, carry = signed_digits(v, W, nwin)
        assert sum(d << (W * j) for j, d in enumerate(digits)) == v, (W, hex(v))
        assert carry == 0 and digits[-1] >= 0, (W, hex(v), digits[-1])
        assert all(-half <= d <= half for d in digits), (W, hex(v))
    assert all(d == half for d in signed_digits(pattern(W, half), W, nwin)[0] if d)            # no carry anywhere
    neg = signed_digits(pattern(W, half + 1), W, nwin)[0]
    assert neg[0] == -(half - 1) and sum(d < 0 for d in neg) >= nwin - 2                         # the carry runs through every window


def test_tables_and_results_match_the_oracle(inputs, expected, tmp_path):
    _check_output(hostbuild.run(hostbuild.program("bases_emul", SRC), inputs[2]), inputs, expected)


def test_the_same_program_under_asan_and_ubsan(inputs, expected):
    hostbuild.need_sanitizer_runtimes()          # BEFORE the build: a build that fails is a failure
    _check_output(hostbuild.run_sanitized(hostbuild.program("bases_emul_san", SRC, san=True), inputs[2]), inputs, expected)
