"""include/bjj_hip_dleq.h without a GPU: the per-item bodies of csrc/dleq.hpp run on the CPU (tests/dleq_emul, bound assertions on)
on the directed sets of tests/dleq_ref.py and on a few hundred seeded random items, against the plain-integer model over the Python
oracle (mul_scalar, proj_add, poseidon); the same harness as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer; and a mutant check of this module's own checker.  Every comparison is byte for byte."""
import ctypes
import os
import random

import pytest

import curve_ref
import dleq_ref as dr
import hostbuild
from conftest import ROOT

EMUL_DIR = os.path.join(ROOT, "tests", "dleq_emul")
SK, SK2, LABEL = dr.L + 0x1234567, 0xABCDEF, 7          # sk >= l: the prover reduces it


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(hostbuild.shared("libdleq_emul.so", os.path.join(EMUL_DIR, "dleq_emul.cpp")))
    cp, sz = ctypes.c_char_p, ctypes.c_size_t
    lib.dq_emul_table.argtypes = [cp, ctypes.c_int]
    lib.dq_emul_pair.argtypes = [cp, cp, cp, cp, cp, sz, cp, cp]
    lib.dq_emul_verify.argtypes = [ctypes.c_int, ctypes.c_int, cp, cp, cp, cp, cp, cp, sz, cp]
    lib.dq_emul_prove.argtypes = [ctypes.c_int, cp, cp, cp, cp, sz, cp, cp, cp, cp, cp]
    lib.dq_emul_free_tables.restype = None
    yield lib
    lib.dq_emul_free_tables()


@pytest.fixture(scope="module")
def be(pyoracle):
    return dr.PyBackend(pyoracle)


@pytest.fixture(scope="module")
def world(be):
    return dr.world(be, curve_ref.TORSION_REF)


def points(raw, n):
    return dr.unpack_points(raw[:64 * n])


def run_pair(emul, P, a, Qp, b, A):
    n = len(P)
    out, ok = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)
    rc = emul.dq_emul_pair(dr.pack_points(P).tobytes(), dr.pack_scalars(a).tobytes(), dr.pack_points(Qp).tobytes(), dr.pack_scalars(b).tobytes(),
                           None if A is None else dr.pack_points(A).tobytes(), n, out, ok)
    assert rc == 0, rc
    return points(out.raw, n), list(ok.raw)


def run_verify(emul, g, pk, tag, C1, D, A, B, z):
    n = len(C1)
    ok = ctypes.create_string_buffer(n)
    rc = emul.dq_emul_verify(g, pk, dr.le(tag), *(dr.pack_points(x).tobytes() for x in (C1, D, A, B)), dr.pack_scalars(z).tobytes(), n, ok)
    assert rc == 0, rc
    return list(ok.raw)


def run_prove(emul, g, sk, tag, C1, w):
    n = len(C1)
    d, a, b = (ctypes.create_string_buffer(64 * n) for _ in range(3))
    z, ok = ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(n)
    rc = emul.dq_emul_prove(g, dr.le(sk), dr.le(tag), dr.pack_points(C1).tobytes(), dr.pack_scalars(w).tobytes(), n, d, a, b, z, ok)
    assert rc == 0, rc
    return points(d.raw, n), points(a.raw, n), points(b.raw, n), dr.unpack_scalars(z.raw[:32 * n]), list(ok.raw)


def first_difference(got, want):
    """the checker of this module: None when the two result tuples agree item for item, else (which array, item)"""
    for k, (g, w) in enumerate(zip(got, want)):
        if len(g) != len(w):
            return (k, -1)
        for i, (x, y) in enumerate(zip(g, w)):
            if x != y:
                return (k, i)
    return None


# ---- bjj_mul_pair -------------------------------------------------------------------------------------------------------------------
def test_mul_pair_directed_against_the_model(emul, be, world):
    P, a, Qp, b, A, names = dr.pair_directed(be, world)
    want = dr.mul_pair(be, P, a, Qp, b, A)
    got = run_pair(emul, P, a, Qp, b, A)
    d = first_difference(got, want)
    assert d is None, (d, names[d[1]])
    refused = [nm for nm, k in zip(names, want[1]) if k == 2]
    assert sorted(refused) == sorted(["off P", "off Q", "off A", "(0,0) P", "(0,0) Q", "(0,0) A"])
    for nm, p in zip(names, want[0]):
        if nm.endswith("A=O") or nm.startswith("A=-(aP+bQ)"):
            assert p == dr.IDENTITY, nm
    # add_xy == NULL is the identity
    idx = [i for i, x in enumerate(A) if x == dr.IDENTITY]
    sub = [[v[i] for i in idx] for v in (P, a, Qp, b)]
    assert first_difference(run_pair(emul, *sub, None), ([want[0][i] for i in idx], [want[1][i] for i in idx])) is None


def test_mul_pair_random_against_the_model(emul, be, world):
    P, a, Qp, b, A = dr.random_pair(be, world, 200, 0xD1E5)
    want = dr.mul_pair(be, P, a, Qp, b, A)
    assert want[1] == [1] * 200
    assert first_difference(run_pair(emul, P, a, Qp, b, A), want) is None
    # ... and it is the composition: A + a P, then + b Q, with the oracle's own mul_scalar on the raw scalars
    comp = be.add(be.add(A, be.mul(P, a)), be.mul(Qp, b))
    assert comp == want[0]


# ---- bjj_dleq_prove / bjj_dleq_verify -----------------------------------------------------------------------------------------------
SETUPS = {"b8_w4": (None, 4, 5), "gen_w5": ("s2", 5, 4)}       # G (None: the context's B8 table), its width, PK's width


@pytest.fixture(scope="module")
def statements(emul, be, world):
    out = {}
    for name, (gname, gw, pw) in SETUPS.items():
        G = dr.B8 if gname is None else world[gname]            # in the prime-order subgroup: PK = sk' G has the discrete log sk'
        PK, PK2 = be.mul([G, G], [SK % dr.L, SK2])
        rec = lambda p: dr.le(p[0]) + dr.le(p[1])   # noqa: E731
        hg = emul.dq_emul_table(None if gname is None else rec(G), gw)
        hpk, hpk2 = emul.dq_emul_table(rec(PK), pw), emul.dq_emul_table(rec(PK2), pw)
        assert min(hg, hpk, hpk2) >= 0
        out[name] = dict(G=G, PK=PK, PK2=PK2, hg=hg, hpk=hpk, hpk2=hpk2, tag=dr.dleq_tag(be, G, PK, LABEL))
    return out


@pytest.mark.parametrize("setup", sorted(SETUPS))
def test_dleq_directed_against_the_model(emul, be, world, statements, setup):
    s = statements[setup]
    cases = dr.dleq_directed(be, world, s["G"], SK, SK2, s["tag"])
    names = [c[0] for c in cases]
    C1, D, A, B, z, pinned = ([c[i] for c in cases] for i in range(1, 7))
    want = dr.dleq_verify(be, s["G"], s["PK"], s["tag"], C1, D, A, B, z)
    for nm, w, p in zip(names, want, pinned):
        assert p is None or w == p, (nm, w, p)                  # the model says what the contract states outright
    assert {"D + T2, c even", "D + T2, c odd"} <= set(names)
    got = run_verify(emul, s["hg"], s["hpk"], s["tag"], C1, D, A, B, z)
    assert got == want, [(nm, g, w) for nm, g, w in zip(names, got, want) if g != w]
    # the statement-wide mutations: a wrong tag and the wrong PK table reject every proof that was valid, and change nothing else
    valid = [i for i, w in enumerate(want) if w == 1]
    assert len(valid) >= 12
    for what, tag in dr.dleq_wrong_statements(s["tag"]):
        g2 = run_verify(emul, s["hg"], s["hpk"], tag, C1, D, A, B, z)
        w2 = dr.dleq_verify(be, s["G"], s["PK"], tag, C1, D, A, B, z)
        assert g2 == w2, what
        assert w2 == want if "same" in what else all(w2[i] == 0 for i in valid), what
    g3 = run_verify(emul, s["hg"], s["hpk2"], s["tag"], C1, D, A, B, z)
    assert g3 == dr.dleq_verify(be, s["G"], s["PK2"], s["tag"], C1, D, A, B, z) and all(g3[i] == 0 for i in valid)
    assert [g3[i] for i, w in enumerate(want) if w == 2] == [2] * want.count(2)


@pytest.mark.parametrize("setup", sorted(SETUPS))
def test_prove_against_the_model_and_round_trip(emul, be, world, statements, setup):
    s = statements[setup]
    rng = random.Random(0xD1E6)
    n = 60
    C1 = be.mul([dr.B8] * n, [rng.randrange(1, dr.L) for _ in range(n)])
    w = [rng.getrandbits(256) for _ in range(n)]
    w[0], w[1], w[2] = 0, dr.L, dr.M256                         # w == 0 (mod l) twice, the largest value
    C1[5], C1[6], C1[7] = world["off"], (0, 0), world["big"]    # off the curve twice; a coordinate >= r
    C1[8] = world["full"]                                       # outside the subgroup: defined, though no sound statement
    want = dr.dleq_prove(be, s["G"], SK, s["tag"], C1, w)
    got = run_prove(emul, s["hg"], SK, s["tag"], C1, w)
    assert first_difference(got, want) is None, first_difference(got, want)
    assert want[4] == [2 if i in (5, 6) else 1 for i in range(n)] and want[3][5] == 0 and want[0][6] == (0, 0)
    assert first_difference(run_prove(emul, s["hg"], SK % dr.L, s["tag"], C1, w), want) is None      # sk >= l is sk mod l
    D, A, B, z, ok = got
    v = run_verify(emul, s["hg"], s["hpk"], s["tag"], C1, D, A, B, z)
    assert v == dr.dleq_verify(be, s["G"], s["PK"], s["tag"], C1, D, A, B, z)
    assert all(v[i] == 1 for i in range(n) if i not in (5, 6, 8)) and v[5] == v[6] == 2


# ---- the checker checks --------------------------------------------------------------------------------------------------------------
def test_a_seeded_wrong_verdict_or_byte_is_reported(emul, be, world):
    P, a, Qp, b, A = dr.random_pair(be, world, 8, 0xD1E7)
    want = dr.mul_pair(be, P, a, Qp, b, A)
    got = run_pair(emul, P, a, Qp, b, A)
    assert first_difference(got, want) is None
    bad_byte = ([p for p in got[0]], list(got[1]))
    bad_byte[0][3] = (bad_byte[0][3][0] ^ (1 << 8), bad_byte[0][3][1])                    # one wrong byte of one point
    assert first_difference(bad_byte, want) == (0, 3)
    bad_verdict = (list(got[0]), [2 if i == 6 else k for i, k in enumerate(got[1])])      # one wrong verdict
    assert first_difference(bad_verdict, want) == (1, 6)
    assert first_difference((got[0][:-1], got[1]), want) == (0, -1)                       # a missing item


def test_the_harness_rejects_what_the_library_rejects(emul, statements):
    s = statements["b8_w4"]
    z = ctypes.create_string_buffer(64)
    assert emul.dq_emul_verify(s["hg"], s["hg"], dr.le(1), z, z, z, z, z, 1, z) == -1      # the context's table is no key
    assert emul.dq_emul_verify(s["hg"], s["hpk"], None, z, z, z, z, z, 1, z) == -1         # no tag
    assert emul.dq_emul_prove(s["hg"], None, dr.le(1), z, z, 1, z, z, z, z, z) == -1       # no sk
    assert emul.dq_emul_table(dr.le(1) + dr.le(1), 4) == -1                                # off the curve


# ---- the same bodies under the sanitizers -------------------------------------------------------------------------------------------
def test_the_mixed_case_under_asan_and_ubsan():
    """a stand-alone program: the harness and its driver compiled with -fsanitize=address,undefined, run directly"""
    out = hostbuild.run_sanitized(hostbuild.program("dleq_emul_san", os.path.join(EMUL_DIR, "dleq_emul_main.cpp"), san=True), timeout=600)
    assert "dleq ok" in out, out[-3000:]
