"""bjj_eddsa_verify_signer / bjj_schnorr_verify_signer without a GPU: the per-item body and the verdict step of csrc/signer.hpp --
what k_signer.hip launches -- run on the CPU by the stand-alone program tests/signer_emul (bound assertions on), over the signer's
table at W = 4 and W = 5 and a context's B8 table at W = 4.  Every verdict is the pure-Python oracle's verify / verify_schnorr for
the same key, for an ordinary key k*B8 and for a key of order 8l, k*B8 + T8.  signer_verdict alone: the same curve points under
several projective scalings give the same verdict (the homogeneity of PointProjective::add in its second operand), both verdicts
occur, and an R that makes the reference's sum z == 0 gives 0.  The same program runs once more built with
-fsanitize=address,undefined, directly (no preload)."""
import os

import numpy as np
import pytest

import hostbuild
import signer_cases as sc
from conftest import ROOT, ints, unpack

Q = sc.Q
SRC = os.path.join(ROOT, "tests", "signer_emul", "signer_emul.cpp")
SCALINGS = [2, Q - 1, 0x1234567890abcdef1234567890abcdef1234567890abcdef1234567890abcdef % Q, 3 * Q + 5]   # the last one is >= r: reduced to 5
KEYS = ("ordinary", "order 8l")


def _verdict_cases(o, A):
    """(l, t, R) triples: l, t curve points; expected verdict from the Python oracle's own proj_add / proj_affine"""
    t = o.mul_scalar(A, 0x1F3D5B79)
    r_on = o.mul_scalar(o.B8, 0xABCDEF123)
    l_true = o.proj_affine(o.proj_add((r_on[0], r_on[1], 1), (t[0], t[1], 1)))
    other = o.mul_scalar(o.B8, 77)
    cases = [(l_true, t, r_on), (other, t, r_on), (l_true, t, (r_on[0], r_on[1] ^ 8)), (t, t, (0, 1)), (l_true, t, (0, 0))]
    ry = 0x2b6a1f % Q
    for sign in (1, Q - 1):    # D rx ry tx ty = +1 makes f = 0, -1 makes g = 0: either way the sum has z == 0
        rx = sign * o.finv(o.D * ry * t[0] * t[1]) % Q
        assert o.proj_add((rx, ry, 1), (t[0], t[1], 1))[2] == 0 and o.proj_affine(o.proj_add((rx, ry, 1), (t[0], t[1], 1))) == (0, 0)
        cases.append((other, t, (rx, ry)))
    want = [int(o.proj_affine(o.proj_add((r[0] % Q, r[1] % Q, 1), (tt[0], tt[1], 1))) == tuple(l)) for l, tt, r in cases]
    assert all(o.on_curve(l) and o.on_curve(tt) for l, tt, _ in cases)
    return cases, want


@pytest.fixture(scope="module")
def inputs(oracle, pyoracle, golden):
    """per key: the program's stdin, the items, and the expected verdicts -- computed once"""
    o = pyoracle
    tors = [ints(t) for t in golden["gpu_expected"]["torsion_points"]]
    out = {}
    for name in KEYS:
        torsion = tors[1] if name == "order 8l" else None
        A = sc.key_point(oracle, sc.KEY_SCALAR, torsion)
        assert o.on_curve(A)
        items = {}
        for schnorr in (False, True):
            R, S, M = sc.directed(oracle, A, sc.KEY_SCALAR, 0x5167 + schnorr, schnorr, torsion is not None)
            R2, S2, M2 = sc.bulk(oracle, A, sc.KEY_SCALAR, 6, 0x77 + schnorr, schnorr, torsion is not None)
            items[schnorr] = (np.concatenate([R, R2]), np.concatenate([S, S2]), np.concatenate([M, M2]))
        R, S, M = (np.concatenate([items[False][j], items[True][j]]) for j in range(3))
        Rv, Sv, Mv = unpack(R, 2), unpack(S), unpack(M)
        n = len(Sv)
        cases, vwant = _verdict_cases(o, A)
        text = "P %x %x\nI %d\n%s\nZ %d\n%s\nV %d\n%s\n" % (
            A[0], A[1], n, "\n".join("%x %x %x %x" % (Rv[i][0], Rv[i][1], Sv[i], Mv[i]) for i in range(n)),
            len(SCALINGS), " ".join("%x" % z for z in SCALINGS),
            len(cases), "\n".join("%x %x %x %x %x %x" % (l + t + r) for l, t, r in cases))
        ed = [int(o.verify(A, Rv[i], Sv[i], Mv[i])) for i in range(n)]
        sn = [{None: 2, False: 0, True: 1}[o.verify_schnorr(A, Mv[i], Rv[i], Sv[i])] for i in range(n)]
        half = n // 2
        nd = len(sc.DIRECTED)
        # the inputs are what they claim to be: the valid directed items verify under their own scheme
        for scheme, base in ((ed, 0), (sn, half)):
            got = dict(zip(sc.DIRECTED, scheme[base:base + nd]))
            assert got["valid"] == got["valid2"] == got["s+l"] == got["R.x+r"] == 1, (name, got)
            assert got["flip s"] == got["flip msg"] == got["flip R.x"] == got["flip R.y"] == got["R=(0,0)"] == 0, (name, got)
        assert ed[sc.DIRECTED.index("msg=Q")] == 1 and ed[sc.DIRECTED.index("msg=Q+1")] == 0
        assert sn[half + sc.DIRECTED.index("msg=Q")] == 1 and sn[half + sc.DIRECTED.index("msg=Q+1")] == 2
        out[name] = {"text": text, "n": n, "eddsa": ed, "schnorr": sn, "nv": len(cases), "vwant": vwant}
    return out


def _check_output(out, inp):
    facts = {"check": [], "e": {}, "s": {}, "v": {}}
    for l in out.split("\n"):
        f = l.split()
        if not f:
            continue
        if f[0] == "check":
            facts["check"].append((int(f[1]), int(f[2])))
        elif f[0] in ("e", "s"):
            facts[f[0]].setdefault(int(f[1]), []).append((int(f[2]), int(f[3])))
        elif f[0] == "v":
            facts["v"].setdefault(int(f[1]), []).append(int(f[3]))
    assert facts["check"] == [(0, 0), (1, 0), (2, 0)]
    for W in (4, 5):
        for kind, want in (("e", inp["eddsa"]), ("s", inp["schnorr"])):
            got = facts[kind][W]
            assert [i for i, _ in got] == list(range(inp["n"]))
            bad = [(i, v, want[i]) for i, v in got if v != want[i]]
            assert not bad, (kind, W, bad)
    assert sorted(facts["v"]) == list(range(inp["nv"]))
    for i in range(inp["nv"]):
        assert facts["v"][i] == [inp["vwant"][i]] * (len(SCALINGS) + 1), (i, facts["v"][i], inp["vwant"][i])
    assert set(inp["vwant"]) == {0, 1} and set(inp["eddsa"]) == {0, 1} and set(inp["schnorr"]) == {0, 1, 2}


@pytest.mark.parametrize("key", KEYS)
def test_verdicts_match_the_python_oracle(inputs, key):
    _check_output(hostbuild.run(hostbuild.program("signer_emul", SRC), inputs[key]["text"]), inputs[key])


def test_the_same_program_under_asan_and_ubsan(inputs):
    hostbuild.need_sanitizer_runtimes()          # BEFORE the build: a build that fails is a failure
    exe = hostbuild.program("signer_emul_san", SRC, san=True)
    for key in KEYS:
        _check_output(hostbuild.run_sanitized(exe, inputs[key]["text"]), inputs[key])
