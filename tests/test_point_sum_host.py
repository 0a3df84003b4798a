"""bjj_point_sum without a GPU: its header is plain C11, the library exports it, bjj_hip.h and what is pinned to it did not move, and
a whole call of the segmented reduction of csrc/point_sum.hpp -- the bodies k_point_sum.hip launches -- run on the CPU
(tests/point_sum_emul, bound and index assertions on, tiles of 8 and 16 items) gives for EVERY segment the fold of the Python
oracle's additions bit for bit: acc = acc.add(+-P_i) from (0, 1, 1), then acc.affine() (src/lib.rs:88-131, 70-85)."""
import ctypes
import os
import random
import re
import subprocess
import sys

import pytest

import hostbuild
from conftest import ROOT
from test_msm_batch_host import OFFSETS_MIXED, emul as batch_emul, emul_batch  # noqa: F401  (batch_emul is a fixture)
from test_msm_host import KINDS, ORDER8, _inputs, le

HEADER = os.path.join(ROOT, "include", "bjj_hip_point_sum.h")
CSRC = os.path.join(ROOT, "babyjubjub-rs_amd", "csrc")
EMUL_DIR = os.path.join(ROOT, "tests", "point_sum_emul")
TILES = (8, 16)


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(hostbuild.shared("libpoint_sum_emul.so", os.path.join(EMUL_DIR, "point_sum_emul.cpp")))
    lib.point_sum_emul_run.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_ulonglong),
                                       ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_longlong)]
    lib.point_sum_emul_segment.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_size_t, ctypes.c_ulonglong]
    lib.point_sum_emul_segment.restype = ctypes.c_uint
    lib.point_sum_emul_levels.argtypes = [ctypes.c_ulonglong, ctypes.c_int]
    return lib


def emul_sum(lib, pts, neg, offsets, T):
    m = len(offsets) - 1
    P = b"".join(le(x) + le(y) for x, y in pts)
    G = None if neg is None else bytes(neg)
    off = (ctypes.c_ulonglong * (m + 1))(*offsets)
    out = ctypes.create_string_buffer(64 * m)
    st = (ctypes.c_longlong * m)()
    assert lib.point_sum_emul_run(P, G, len(pts), off, m, T, out, st) == 0
    r = out.raw
    return [(int.from_bytes(r[64 * s:64 * s + 32], "little"), int.from_bytes(r[64 * s + 32:64 * s + 64], "little")) for s in range(m)], list(st)


def fold_signed(o, pts, neg):
    acc = (0, 1, 1)
    for i, (x, y) in enumerate(pts):
        if neg is not None and neg[i]:
            x = (o.Q - x) % o.Q
        acc = o.proj_add(acc, (x, y, 1))
    return tuple(o.proj_affine(acc))


def folds(o, pts, neg, offsets):
    return [fold_signed(o, pts[a:b], None if neg is None else neg[a:b]) for a, b in zip(offsets, offsets[1:])]


def offsets_of(lengths):
    off = [0]
    for v in lengths:
        off.append(off[-1] + v)
    return off


@pytest.fixture(scope="module")
def pool(pyoracle):
    """300 random points of the prime-order subgroup shifted by torsion, computed once and never written"""
    rng = random.Random(0x9505)
    return tuple(_inputs(pyoracle, rng, "torsion_shifted", 300)[0])


# ---- the boundary -------------------------------------------------------------------------------------------------------------
def _decls(path):
    h = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return re.sub(r"\s+([,)])", r"\1", " ".join(h.split()))


def test_header_declares_both_forms():
    h = _decls(HEADER)
    assert ("int bjj_point_sum(bjj_ctx* ctx, const uint8_t* pts_xy, const uint8_t* neg, size_t n, const uint64_t* offsets, size_t m, "
            "uint8_t* out_xy, int64_t* out_first_off_curve);") in h
    assert ("int bjj_point_sum_dev(bjj_ctx* ctx, const void* d_pts_xy, const void* d_neg, size_t n, const void* d_offsets, size_t m, "
            "void* d_out_xy, void* d_first_off_curve, void* stream);") in h
    assert '#include "bjj_hip.h"' in h
    assert sorted(set(re.findall(r"\b(bjj_[a-z0-9_]+)\s*\(", h))) == ["bjj_point_sum", "bjj_point_sum_dev"]


def test_header_is_plain_c11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "bjj_hip_point_sum.h"\n'
                   "int use(bjj_ctx* c, const uint8_t* p, const uint64_t* o, uint8_t* out, int64_t* st) {\n"
                   "  return bjj_point_sum(c, p, 0, 0, o, 1, out, st) + bjj_point_sum_dev(c, p, p, 0, o, 1, out, st, 0);\n}\n")
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_library_exports_both_forms():
    lib = os.path.join(CSRC, "libbjj_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    assert "bjj_point_sum" in syms and "bjj_point_sum_dev" in syms
    sys.path.insert(0, ROOT)
    from babyjubjub_rs_amd import _lib
    assert _lib.POINT_SUM_SYMBOLS == ("bjj_point_sum", "bjj_point_sum_dev")
    loaded = _lib.load()
    for name in _lib.POINT_SUM_SYMBOLS:
        assert getattr(loaded, name).argtypes is not None
    import babyjubjub_rs_amd as bjj
    assert callable(bjj.point_sum)
    for name in ("point_sum", "point_sum_dev", "elgamal_sum"):
        assert hasattr(bjj.Context, name)


def test_the_pinned_abi_did_not_move():
    """the new entry points live in their own header: bjj_hip.h, the binding's EXPORTED_SYMBOLS and EXT_SYMBOLS stay as they were"""
    sys.path.insert(0, ROOT)
    from babyjubjub_rs_amd import _lib
    names = set(re.findall(r"\b(bjj_[a-z0-9_]+)\s*\(", _decls(os.path.join(ROOT, "include", "bjj_hip.h"))))
    assert len(names) == len(_lib.EXPORTED_SYMBOLS) == 71 and names == set(_lib.EXPORTED_SYMBOLS)
    assert not any("point_sum" in n for n in names)
    assert _lib.EXT_SYMBOLS == ("bjj_msm_batch", "bjj_msm_batch_dev")
    assert not set(_lib.POINT_SUM_SYMBOLS) & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.EXT_SYMBOLS))
    ffi = open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read()
    assert len(re.findall(r"\bfn (bjj_[a-z0-9_]+)", ffi)) == 71 and "point_sum" not in ffi


def test_the_tile_is_an_integer_literal():
    """tests and tools read PSUM_TILE from the header"""
    m = re.search(r"^#define PSUM_TILE (\d+)\b", open(os.path.join(CSRC, "point_sum.hpp")).read(), flags=re.M)
    assert m and int(m.group(1)) >= 64 and int(m.group(1)) & (int(m.group(1)) - 1) == 0


# ---- the segment search and the schedule ----------------------------------------------------------------------------------------
def test_segment_search_is_clamped_and_exact(emul):
    rng = random.Random(0xC5B)
    for offsets in ([0, 5], OFFSETS_MIXED, [0, 0, 0], [0, 0, 0, 7, 7, 9]):
        m = len(offsets) - 1
        off = (ctypes.c_ulonglong * (m + 1))(*offsets)
        for i in range(offsets[-1]):
            s = emul.point_sum_emul_segment(off, m, i)
            assert offsets[s] <= i < offsets[s + 1]
    for _ in range(200):   # garbage: the result stays a valid segment number
        m = rng.randrange(1, 40)
        offsets = [rng.choice([0, 1, 5, 1 << 63, (1 << 64) - 1, rng.getrandbits(64), rng.randrange(64)]) for _ in range(m + 1)]
        off = (ctypes.c_ulonglong * (m + 1))(*offsets)
        for i in (0, 1, 63, 64, rng.getrandbits(32)):
            assert 0 <= emul.point_sum_emul_segment(off, m, i) < m


def test_the_number_of_launches_is_logarithmic(emul):
    """whatever the offsets: n items, then two entries per tile, until one tile holds the rest"""
    assert [emul.point_sum_emul_levels(n, 256) for n in (1, 256, 257, 1 << 15, (1 << 15) + 1, 1 << 20, (1 << 32) - 1)] == [1, 1, 2, 2, 3, 3, 5]
    assert [emul.point_sum_emul_levels(n, 8) for n in (8, 9, 32, 33, 300)] == [1, 2, 2, 3, 4]


# ---- whole calls on the CPU against the fold of every segment -------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_every_input_kind_over_the_mixed_offsets(emul, pyoracle, kind):
    rng = random.Random(0x95A + KINDS.index(kind))
    P, _ = _inputs(pyoracle, rng, kind, 300)
    neg = [rng.randrange(2) for _ in range(300)]
    for g in (None, neg):
        want = folds(pyoracle, P, g, OFFSETS_MIXED)
        assert want[1] == (0, 1)
        for T in TILES:
            got, st = emul_sum(emul, P, g, OFFSETS_MIXED, T)
            assert st == [-1] * 7 and got == want, (kind, T, g is None)
    if kind == "cancelling_pairs":   # every point has its negation beside it: the segments of even length and even start cancel
        assert folds(pyoracle, P, None, [0, 64, 300]) == [(0, 1), (0, 1)] == emul_sum(emul, P, None, [0, 64, 300], 8)[0]


@pytest.mark.parametrize("T", TILES)
def test_segment_lengths_around_the_tile(emul, pyoracle, pool, T):
    lengths = [0, 1, 2, T - 1, T, T + 1, 2 * T, 3 * T + 1]
    for order in (lengths, lengths[::-1], [3 * T + 1, 1, T, 0, 2, 2 * T, T - 1, T + 1]):
        off = offsets_of(order)
        P = list(pool[:off[-1]])
        neg = [(i * 7 // 3) % 2 for i in range(len(P))]
        got, st = emul_sum(emul, P, neg, off, T)
        assert st == [-1] * 8 and got == folds(pyoracle, P, neg, off), (T, order)


@pytest.mark.parametrize("T", TILES)
def test_empty_segments_first_last_and_at_a_tile_boundary(emul, pyoracle, pool, T):
    for lengths in ([0, T, 0, 0, T, 3, 0], [0, 0, T - 1, 0, 1, 0, 0, 2 * T, 0], [T, 0, 0, T]):
        off = offsets_of(lengths)
        P = list(pool[:off[-1]])
        got, st = emul_sum(emul, P, None, off, T)
        assert st == [-1] * len(lengths) and got == folds(pyoracle, P, None, off), (T, lengths)
        assert all(got[s] == (0, 1) for s, v in enumerate(lengths) if v == 0)


def test_all_segments_empty(emul):
    for T in TILES:
        assert emul_sum(emul, [], None, [0, 0, 0], T) == ([(0, 1), (0, 1)], [-1, -1])
        assert emul_sum(emul, [], b"", [0, 0], T) == ([(0, 1)], [-1])


def test_pairs_duplicates_and_small_orders(emul, pyoracle, pool):
    o = pyoracle
    p, q = pool[0], pool[1]
    minus = lambda a: ((o.Q - a[0]) % o.Q, a[1])   # noqa: E731
    tors = [o.mul_scalar(o.T8, j) for j in range(8)]
    assert tors[0] == (0, 1) and tors[4] == (0, o.Q - 1)          # orders 1 and 2; tors[2]: 4, tors[1]: 8
    segs = [[p, minus(p)], [p, p], [p] * 3, [p] * 8, [p, minus(p)] * 9 + [q],
            [tors[0]] * 3, [tors[4]] * 2, [tors[4]] * 3, [tors[2]] * 4, [tors[2]] * 3, [tors[1]] * 8, [tors[1]] * 5, [tors[1], q, tors[7]]]
    P = [a for s in segs for a in s]
    off = offsets_of([len(s) for s in segs])
    want = folds(o, P, None, off)
    assert want[0] == (0, 1) and want[1] == o.mul_scalar(p, 2) and want[2] == o.mul_scalar(p, 3) and want[3] == o.mul_scalar(p, 8)
    assert want[4] == q and want[5] == want[6] == want[8] == want[10] == (0, 1) and want[7] == tors[4] and want[12] == q
    for T in TILES:
        assert emul_sum(emul, P, None, off, T) == (want, [-1] * len(segs)), T
    # the same cancellation through the sign array: p - p, and p + p - p - p over a tile boundary
    P2 = [p, p] + [q] * 16
    for T in TILES:
        got, st = emul_sum(emul, P2, [0, 1] + [0, 1] * 8, [0, 2, 18], T)
        assert got == [(0, 1), (0, 1)] and st == [-1, -1]


def test_signs_all_added_all_subtracted_alternating(emul, pyoracle, pool):
    P = list(pool)
    plus = folds(pyoracle, P, None, OFFSETS_MIXED)
    for neg in (None, [0] * 300, [1] * 300, [7] * 300, [i % 2 for i in range(300)]):
        want = folds(pyoracle, P, neg, OFFSETS_MIXED)
        if neg and all(neg):
            assert want == [((pyoracle.Q - x) % pyoracle.Q, y) for x, y in plus]     # the sum of the negations is the negation
        for T in TILES:
            assert emul_sum(emul, P, neg, OFFSETS_MIXED, T) == (want, [-1] * 7)


def test_parity_with_the_batched_msm(emul, batch_emul, pool):
    """scalar 1 for an added term, 8l - 1 for a subtracted one: the same bytes from the bucket pipeline"""
    P = list(pool)
    rng = random.Random(0x8E1)
    neg = [rng.randrange(2) for _ in range(300)]
    want, wst = emul_batch(batch_emul, P, [ORDER8 - 1 if g else 1 for g in neg], OFFSETS_MIXED, 5)
    assert wst == [-1] * 7
    for T in TILES:
        assert emul_sum(emul, P, neg, OFFSETS_MIXED, T) == (want, wst)
    Q = list(P)
    Q[70] = (Q[70][0] ^ 1, Q[70][1])
    want, wst = emul_batch(batch_emul, Q, [ORDER8 - 1 if g else 1 for g in neg], OFFSETS_MIXED, 5)
    assert wst[5] == 70 and emul_sum(emul, Q, neg, OFFSETS_MIXED, 16) == (want, wst)


def test_off_curve_points_spoil_only_their_segment(emul, pool):
    P = list(pool)
    T = 16
    alt = [i % 2 for i in range(300)]
    for neg in (None, alt):
        clean, st = emul_sum(emul, P, neg, OFFSETS_MIXED, T)
        assert st == [-1] * 7
        # first / last of a segment; both sides of a tile boundary (one segment, the smaller index wins; two segments); two in
        # one segment in either order; a subtracted one (alt: odd indices); the single-point segments
        for bad in ([2], [63], [65], [128], [T - 1, T], [4 * T, 4 * T - 1], [8 * T, 8 * T - 1, 129], [100, 66], [70], [71], [0, 64, 299], [1, 2, 3]):
            Q = list(P)
            for i in bad:
                Q[i] = (Q[i][0] ^ 1, Q[i][1])
            got, st = emul_sum(emul, Q, neg, OFFSETS_MIXED, T)
            for s, (a, b) in enumerate(zip(OFFSETS_MIXED, OFFSETS_MIXED[1:])):
                hit = [i for i in bad if a <= i < b]
                assert st[s] == (min(hit) if hit else -1), (bad, s)
                assert got[s] == ((0, 0) if hit else clean[s]), (bad, s)
        assert emul_sum(emul, P, neg, OFFSETS_MIXED, T) == (clean, [-1] * 7)


@pytest.mark.parametrize("offsets", [[0, 10, 5, 40], [1, 10, 20, 40], [0, 10, 20, 39], [0, 10, 20, 41], [0, 1 << 40, 3, 40]])
def test_bad_offsets_are_data_in_the_device_form(emul, pool, offsets):
    """the emulator runs the device form: status -2 and (0, 0) everywhere, and no index leaves its array on the way (the harness
    returns -2 instead of 0 if one does)"""
    for T in TILES:
        got, st = emul_sum(emul, list(pool[:40]), [1] * 40, offsets, T)
        assert st == [-2] * 3 and got == [(0, 0)] * 3


# ---- the same bodies under the sanitizers -------------------------------------------------------------------------------------------
def test_the_mixed_case_under_asan_and_ubsan():
    """a stand-alone program: the harness and its driver compiled with -fsanitize=address,undefined, run directly"""
    hostbuild.need_sanitizer_runtimes()
    out = hostbuild.run_sanitized(hostbuild.program("point_sum_emul_san", os.path.join(EMUL_DIR, "point_sum_emul_main.cpp"), san=True), timeout=600)
    assert "point_sum ok" in out, out[-3000:]
