"""bjj_msm_batch without a GPU: its header is plain C11, the library exports it, bjj_hip.h and what is pinned to it did not move, and
the batched bucket pipeline of csrc/msm.hpp -- the bodies k_msm.hip and k_msm_batch.hip launch -- run on the CPU
(tests/msm_batch_emul, bound and index assertions on) gives for EVERY segment the reference fold of the Python oracle bit for bit."""
import ctypes
import os
import random
import re
import subprocess
import sys

import pytest

import hostbuild
from conftest import ROOT
from test_msm_host import KINDS, _inputs, fold, le

HEADER = os.path.join(ROOT, "include", "bjj_hip_msm_batch.h")
OFFSETS_MIXED = [0, 1, 1, 2, 64, 65, 129, 300]


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(hostbuild.shared("libmsm_batch_emul.so", os.path.join(ROOT, "tests", "msm_batch_emul", "msm_batch_emul.cpp")))
    lib.msm_batch_emul_run.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_ulonglong),
                                       ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_longlong)]
    lib.msm_batch_emul_segment.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_size_t, ctypes.c_ulonglong]
    lib.msm_batch_emul_segment.restype = ctypes.c_uint
    return lib


def emul_batch(lib, pts, scalars, offsets, c):
    m = len(offsets) - 1
    P = b"".join(le(x) + le(y) for x, y in pts)
    S = b"".join(le(k) for k in scalars)
    off = (ctypes.c_ulonglong * (m + 1))(*offsets)
    out = ctypes.create_string_buffer(64 * m)
    st = (ctypes.c_longlong * m)()
    assert lib.msm_batch_emul_run(P, S, len(pts), off, m, c, out, st) == 0
    r = out.raw
    return [(int.from_bytes(r[64 * s:64 * s + 32], "little"), int.from_bytes(r[64 * s + 32:64 * s + 64], "little")) for s in range(m)], list(st)


def folds(o, P, K, offsets, cache):
    return [tuple(fold(o, P[a:b], K[a:b], cache)) for a, b in zip(offsets, offsets[1:])]


# ---- the boundary -------------------------------------------------------------------------------------------------------------
def _decls(path):
    h = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return re.sub(r"\s+([,)])", r"\1", " ".join(h.split()))


def test_header_declares_both_forms():
    h = _decls(HEADER)
    assert ("int bjj_msm_batch(bjj_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, const uint64_t* offsets, size_t m, "
            "int window_bits, uint8_t* out_xy, int64_t* out_first_off_curve);") in h
    assert ("int bjj_msm_batch_dev(bjj_ctx* ctx, const void* d_pts_xy, const void* d_scalars, size_t n, const void* d_offsets, size_t m, "
            "int window_bits, void* d_out_xy, void* d_first_off_curve, void* stream);") in h
    assert '#include "bjj_hip.h"' in h
    assert sorted(set(re.findall(r"\b(bjj_[a-z0-9_]+)\s*\(", h))) == ["bjj_msm_batch", "bjj_msm_batch_dev"]


def test_header_is_plain_c11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "bjj_hip_msm_batch.h"\n'
                   "int use(bjj_ctx* c, const uint8_t* p, const uint64_t* o, uint8_t* out, int64_t* st) {\n"
                   "  return bjj_msm_batch(c, p, p, 0, o, 1, 0, out, st) + bjj_msm_batch_dev(c, p, p, 0, o, 1, 0, out, st, 0);\n}\n")
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_library_exports_both_forms():
    lib = os.path.join(ROOT, "babyjubjub-rs_amd", "csrc", "libbjj_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    assert "bjj_msm_batch" in syms and "bjj_msm_batch_dev" in syms
    sys.path.insert(0, ROOT)
    from babyjubjub_rs_amd import _lib
    assert _lib.EXT_SYMBOLS == ("bjj_msm_batch", "bjj_msm_batch_dev")
    loaded = _lib.load()
    for name in _lib.EXT_SYMBOLS:
        assert getattr(loaded, name).argtypes is not None
    import babyjubjub_rs_amd as bjj
    assert callable(bjj.msm_batch) and hasattr(bjj.Context, "msm_batch") and hasattr(bjj.Context, "msm_batch_dev")


def test_the_pinned_abi_did_not_move():
    """the new entry points live in their own header: bjj_hip.h, the binding's EXPORTED_SYMBOLS and the Rust shim keep their 71
    functions (tests/test_abi.py, tests/test_rust_shim.py and tests/test_gpu_memory_contract.py enumerate them)"""
    sys.path.insert(0, ROOT)
    from babyjubjub_rs_amd import _lib
    names = set(re.findall(r"\b(bjj_[a-z0-9_]+)\s*\(", _decls(os.path.join(ROOT, "include", "bjj_hip.h"))))
    assert len(names) == len(_lib.EXPORTED_SYMBOLS) == 71 and names == set(_lib.EXPORTED_SYMBOLS)
    assert not any("msm_batch" in n for n in names)
    assert not set(_lib.EXT_SYMBOLS) & set(_lib.EXPORTED_SYMBOLS)
    ffi = open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()
    assert len(re.findall(r"\bfn (bjj_[a-z0-9_]+)", ffi)) == 71 and "msm_batch" not in ffi


# ---- the segment search: in range for ANY offsets content -----------------------------------------------------------------------
def test_segment_search_is_clamped_and_exact(emul):
    rng = random.Random(0xC5A)
    for offsets in ([0, 5], OFFSETS_MIXED, [0, 0, 0], [0, 0, 0, 7, 7, 9]):
        m = len(offsets) - 1
        off = (ctypes.c_ulonglong * (m + 1))(*offsets)
        for i in range(offsets[-1]):
            s = emul.msm_batch_emul_segment(off, m, i)
            assert offsets[s] <= i < offsets[s + 1]
    for _ in range(200):   # garbage: the result stays a valid segment number
        m = rng.randrange(1, 40)
        offsets = [rng.choice([0, 1, 5, 1 << 63, (1 << 64) - 1, rng.getrandbits(64), rng.randrange(64)]) for _ in range(m + 1)]
        off = (ctypes.c_ulonglong * (m + 1))(*offsets)
        for i in (0, 1, 63, 64, rng.getrandbits(32)):
            assert 0 <= emul.msm_batch_emul_segment(off, m, i) < m


# ---- the whole batched pipeline on the CPU against the reference fold of every segment ----------------------------------------------
def test_mixed_offsets_match_the_reference_fold(emul, pyoracle):
    rng = random.Random(0xBA7C4)
    P, K = _inputs(pyoracle, rng, "random", 300)
    want = folds(pyoracle, P, K, OFFSETS_MIXED, {})
    assert want[1] == (0, 1)
    for c in (4, 6):
        got, st = emul_batch(emul, P, K, OFFSETS_MIXED, c)
        assert st == [-1] * 7 and got == want, c


def test_all_segments_empty(emul):
    for c in (4, 6):
        assert emul_batch(emul, [], [], [0, 0, 0], c) == ([(0, 1), (0, 1)], [-1, -1])


@pytest.mark.parametrize("kind", KINDS)
def test_every_input_kind_in_six_segments(emul, pyoracle, kind):
    rng = random.Random(0xB47 + KINDS.index(kind))
    lengths = [0, 40] + [rng.randrange(0, 41) for _ in range(4)]
    rng.shuffle(lengths)
    offsets = [0]
    for n in lengths:
        offsets.append(offsets[-1] + n)
    P, K = _inputs(pyoracle, rng, kind, offsets[-1])
    want = folds(pyoracle, P, K, offsets, {})
    for c in (4, 6):
        got, st = emul_batch(emul, P, K, offsets, c)
        assert st == [-1] * 6 and got == want, (kind, c, lengths)


def test_equal_scalars_with_a_boundary_every_five_points(emul, pyoracle):
    """one digit per window for every item: only the segment part of the key keeps neighbouring segments apart"""
    rng = random.Random(0xE5)
    P, K = _inputs(pyoracle, rng, "equal_scalars", 60)
    offsets = list(range(0, 61, 5))
    want = folds(pyoracle, P, K, offsets, {})
    for c in (4, 8):
        got, st = emul_batch(emul, P, K, offsets, c)
        assert st == [-1] * 12 and got == want, c


def test_off_curve_points_spoil_only_their_segment(emul, pyoracle):
    rng = random.Random(0x0FF)
    P, K = _inputs(pyoracle, rng, "random", 300)
    clean, st = emul_batch(emul, P, K, OFFSETS_MIXED, 5)
    assert st == [-1] * 7
    for bad in ([70], [100, 66], [0, 64, 299], [1, 2, 3]):
        Q = list(P)
        for i in bad:
            Q[i] = (Q[i][0] ^ 1, Q[i][1])
        got, st = emul_batch(emul, Q, K, OFFSETS_MIXED, 5)
        for s, (a, b) in enumerate(zip(OFFSETS_MIXED, OFFSETS_MIXED[1:])):
            hit = [i for i in bad if a <= i < b]
            assert st[s] == (min(hit) if hit else -1), (bad, s)
            assert got[s] == ((0, 0) if hit else clean[s]), (bad, s)
    assert emul_batch(emul, P, K, OFFSETS_MIXED, 5) == (clean, [-1] * 7)


@pytest.mark.parametrize("offsets", [[0, 10, 5, 40], [1, 10, 20, 40], [0, 10, 20, 39], [0, 10, 20, 41], [0, 1 << 40, 3, 40]])
def test_bad_offsets_are_data_in_the_device_form(emul, pyoracle, offsets):
    """the emulator runs the device form: status -2 and (0, 0) everywhere, and no index leaves its array on the way (the harness
    returns -2 instead of 0 if one does)"""
    P = [pyoracle.mul_scalar(pyoracle.B8, 7 + i) for i in range(40)]
    got, st = emul_batch(emul, P, [3 + i for i in range(40)], offsets, 4)
    assert st == [-2] * 3 and got == [(0, 0)] * 3
