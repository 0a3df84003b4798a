"""bjj_msm without a GPU: the C ABI declares and exports it, and the bucket pipeline of csrc/msm.hpp -- the bodies k_msm.hip
launches -- run on the CPU (tests/msm_emul, bound assertions on) gives the reference fold of the Python oracle bit for bit:
acc = acc.add(&P_i.mul_scalar(k_i).projective()) from (0, 1, 1), then acc.affine() (src/lib.rs:149-164, 88-131, 70-85)."""
import ctypes
import json
import os
import random
import re
import subprocess
import sys

import pytest

import hostbuild
from conftest import ROOT

L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
ORDER8 = 8 * L
EDGE_SCALARS = [0, 1, 2, ORDER8 - 1, ORDER8, ORDER8 + 1, 2 * ORDER8 - 1, (1 << 256) - 1, (1 << 255) // 3, L, L - 1, (1 << 254) - 1,
                1 << 253, (1 << 256) - ORDER8]


@pytest.fixture(scope="module")
def msm_emul():
    lib = ctypes.CDLL(hostbuild.shared("libmsm_emul.so", os.path.join(ROOT, "tests", "msm_emul", "msm_emul.cpp")))
    lib.msm_emul_run.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p,
                                 ctypes.POINTER(ctypes.c_longlong)]
    lib.msm_emul_digits.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    return lib


def le(v):
    return int(v).to_bytes(32, "little")


def emul_msm(lib, pts, scalars, c):
    P = b"".join(le(x) + le(y) for x, y in pts)
    S = b"".join(le(k) for k in scalars)
    out = ctypes.create_string_buffer(64)
    st = ctypes.c_longlong(0)
    assert lib.msm_emul_run(P, S, len(pts), c, out, ctypes.byref(st)) == 0
    r = out.raw
    return (int.from_bytes(r[:32], "little"), int.from_bytes(r[32:], "little")), st.value


def fold(o, pts, scalars, cache=None):
    acc = (0, 1, 1)
    for p, k in zip(pts, scalars):
        key = (p, k)
        m = cache.get(key) if cache is not None else None
        if m is None:
            m = o.mul_scalar(p, k)
            if cache is not None:
                cache[key] = m
        acc = o.proj_add(acc, (m[0], m[1], 1))
    return o.proj_affine(acc)


# ---- the boundary -------------------------------------------------------------------------------------------------------------
def test_header_declares_msm():
    h = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "bjj_hip.h")).read(), flags=re.S)
    h = re.sub(r"\s+([,)])", r"\1", " ".join(h.split()))
    assert ("int bjj_msm(bjj_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, int window_bits, uint8_t* out_xy, "
            "int64_t* out_first_off_curve);") in h
    assert ("int bjj_msm_dev(bjj_ctx* ctx, const void* d_pts_xy, const void* d_scalars, size_t n, int window_bits, void* d_out_xy, "
            "void* d_first_off_curve, void* stream);") in h


def test_library_exports_msm():
    lib = os.path.join(ROOT, "babyjubjub-rs_amd", "csrc", "libbjj_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    assert "bjj_msm" in syms and "bjj_msm_dev" in syms
    sys.path.insert(0, ROOT)
    from babyjubjub_rs_amd import _lib
    assert "bjj_msm" in _lib.EXPORTED_SYMBOLS and "bjj_msm_dev" in _lib.EXPORTED_SYMBOLS


# ---- recoding -------------------------------------------------------------------------------------------------------------------
def test_signed_digits_round_trip(msm_emul):
    rng = random.Random(0x4D534D)
    for k in EDGE_SCALARS + [rng.getrandbits(256) for _ in range(20)]:
        for c in range(4, 21):
            W = (255 + c - 1) // c
            d = (ctypes.c_int * 64)()
            assert msm_emul.msm_emul_digits(le(k), c, d) == W
            digits = list(d[:W])
            assert all(-(1 << (c - 1)) <= x <= (1 << (c - 1)) for x in digits), (k, c)
            v = sum(x << (c * j) for j, x in enumerate(digits))
            assert v == k % ORDER8, (k, c)          # exact: no carry leaves the last window


# ---- the whole bucket algorithm on the CPU against the reference fold --------------------------------------------------------------
def _inputs(o, rng, kind, n):
    pt = lambda: o.mul_scalar(o.B8, rng.randrange(1, L))   # noqa: E731
    tors = [o.mul_scalar(o.T8, j) for j in range(8)]
    if kind == "random":
        return [pt() for _ in range(n)], [rng.getrandbits(256) for _ in range(n)]
    if kind == "torsion_shifted":
        P = [o.proj_affine(o.proj_add((*pt(), 1), (*tors[rng.randrange(8)], 1))) for _ in range(n)]
        return P, [rng.getrandbits(256) for _ in range(n)]
    if kind == "identity_and_torsion":
        P = [(0, 1) if i % 3 == 0 else tors[rng.randrange(8)] for i in range(n)]
        return P, [rng.getrandbits(256) for _ in range(n)]
    if kind == "duplicates":
        base = [pt() for _ in range(3)]
        return [base[rng.randrange(3)] for _ in range(n)], [rng.getrandbits(256) for _ in range(n)]
    if kind == "cancelling_pairs":
        P, K = [], []
        for i in range(n // 2):
            p, k = pt(), rng.getrandbits(256)
            P += [p, (o.Q - p[0], p[1])]
            K += [k, k]
        if n % 2:
            P.append(pt())
            K.append(rng.getrandbits(256))
        return P, K
    if kind == "edge_scalars":
        return [pt() for _ in range(n)], [EDGE_SCALARS[i % len(EDGE_SCALARS)] for i in range(n)]
    if kind == "zero_scalars":
        return [pt() for _ in range(n)], [0] * n
    if kind == "equal_scalars":
        k = rng.getrandbits(256)
        return [pt() for _ in range(n)], [k] * n
    raise AssertionError(kind)


KINDS = ["random", "torsion_shifted", "identity_and_torsion", "duplicates", "cancelling_pairs", "edge_scalars", "zero_scalars",
         "equal_scalars"]


@pytest.mark.parametrize("kind", KINDS)
def test_emulated_pipeline_matches_the_reference_fold(msm_emul, pyoracle, kind):
    rng = random.Random(0x4D53 + KINDS.index(kind))
    cache = {}
    for n, cs in ((1, (4, 8)), (2, (5,)), (3, (6, 4)), (17, (7,)), (64, (4, 8)), (129, (5,)), (300, (6, 8))):
        P, K = _inputs(pyoracle, rng, kind, n)
        want = fold(pyoracle, P, K, cache)
        for c in cs:
            got, st = emul_msm(msm_emul, P, K, c)
            assert st == -1 and got == tuple(want), (kind, n, c)
    if kind == "cancelling_pairs":   # n = 300: every point has its negation beside it
        assert emul_msm(msm_emul, P, K, 4) == ((0, 1), -1)


def test_emulated_empty_and_off_curve(msm_emul, pyoracle):
    assert emul_msm(msm_emul, [], [], 4) == ((0, 1), -1)
    P = [pyoracle.mul_scalar(pyoracle.B8, 5 + i) for i in range(40)]
    for bad in ([0], [20], [39], [33, 7, 12]):
        Q = list(P)
        for i in bad:
            Q[i] = (Q[i][0] ^ 1, Q[i][1])
        assert emul_msm(msm_emul, Q, [3] * 40, 5) == ((0, 0), min(bad))


def test_emulated_skew_one_bucket(msm_emul, pyoracle):
    """every digit of every scalar in one bucket of its window, and one huge bucket across several levels of partials"""
    P = [pyoracle.mul_scalar(pyoracle.B8, 1000 + i) for i in range(300)]
    sc = (1 << 255) // 3        # 0x5555...: digit 5 in every 4-bit window
    psum = (0, 1, 1)
    for p in P:
        psum = pyoracle.proj_add(psum, (*p, 1))
    want = pyoracle.mul_scalar(pyoracle.proj_affine(psum), sc)
    for c in (4, 8):
        got, st = emul_msm(msm_emul, P, [sc] * 300, c)
        assert st == -1 and got == tuple(want), c


# ---- the golden file of the GPU tests ---------------------------------------------------------------------------------------------
def test_msm_golden_is_reproducible(tmp_path):
    gen = os.path.join(ROOT, "tests", "golden", "make_msm_expected.py")
    src = open(gen).read().replace('os.path.join(HERE, "msm_expected.json")', repr(str(tmp_path / "out.json")))
    script = tmp_path / "gen.py"
    script.write_text(src.replace("HERE = os.path.dirname(os.path.abspath(__file__))", "HERE = %r" % os.path.dirname(gen)))
    subprocess.run([sys.executable, str(script)], check=True, stdout=subprocess.PIPE)
    committed = os.path.join(ROOT, "tests", "golden", "msm_expected.json")
    assert open(tmp_path / "out.json", "rb").read() == open(committed, "rb").read()
    doc = json.load(open(committed))
    assert 20 <= len(doc["cases"]) and os.path.getsize(committed) < 100 * 1024


def test_msm_golden_matches_the_emulated_pipeline(msm_emul):
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "msm_expected.json")))
    for case in doc["cases"]:
        P = [(int(x, 16), int(y, 16)) for x, y in case["points"]]
        K = [int(k, 16) for k in case["scalars"]]
        want = tuple(int(v, 16) for v in case["result"])
        for c in (4, 6):
            assert emul_msm(msm_emul, P, K, c) == (want, -1), (case["name"], c)
