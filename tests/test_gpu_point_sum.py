"""bjj_point_sum on the MI355X: m signed point sums over CSR segments in one call.  Every result and every status word is expected
to be byte for byte what bjj_msm_batch gives for the same points and offsets with the scalar 1 for an added term and 8l - 1 for a
subtracted one (gpu_ctx.msm_batch); the 300-point case also what the C oracle composes (mul_var_base, then a point_add tree).
The shapes sit around the tile of the kernel, PSUM_TILE of csrc/point_sum.hpp."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pack, unpack
from test_gpu_msm import IDENTITY, ORDER8, ZERO, group_points, oracle_msm
from test_gpu_msm_batch import BAD_OFFSETS, MIXED, offsets_of

pytestmark = pytest.mark.gpu

T = int(re.search(r"^#define PSUM_TILE (\d+)\b", open(os.path.join(ROOT, "babyjubjub-rs_amd", "csrc", "point_sum.hpp")).read(),
                  flags=re.M).group(1))
ONE, MINUS_ONE = pack([1]).reshape(1, 32), pack([ORDER8 - 1]).reshape(1, 32)
POOL = 20000


def odd(neg):
    """the sign bytes at an odd address"""
    buf = np.zeros(neg.size + 2, np.uint8)
    k = 1 if buf.ctypes.data % 2 == 0 else 2
    v = buf[k:k + neg.size]
    v[:] = neg
    assert neg.size == 0 or v.ctypes.data % 2 == 1
    return v


def raw_sum(ctx, pts, neg, offsets):
    """bjj_point_sum as the C ABI returns it: rc, (m, 64) result bytes, (m,) status words (pre-filled with a sentinel)"""
    pts = np.ascontiguousarray(pts, np.uint8).reshape(-1)
    off = np.ascontiguousarray(offsets, np.uint64)
    n, m = pts.size // 64, off.size - 1
    g = None if neg is None else odd(np.asarray(neg, np.uint8))
    out = np.full(max(m, 1) * 64, 0xAB, np.uint8)
    st = np.full(max(m, 1), 12345, np.int64)
    rc = ctx.lib.bjj_point_sum(ctx.handle, pts.ctypes.data if n else None, g.ctypes.data if g is not None and n else None, n,
                               off.ctypes.data, m, out.ctypes.data, st.ctypes.data)
    return rc, out[:m * 64].reshape(m, 64), st[:m]


def ok_sum(ctx, pts, neg, offsets):
    rc, out, st = raw_sum(ctx, pts, neg, offsets)
    assert rc == 0, ctx.lib.bjj_last_error()
    return out, st


def unit_scalars(n, neg):
    sc = np.repeat(ONE, n, axis=0)
    if neg is not None:
        sc[np.asarray(neg) != 0] = MINUS_ONE
    return sc


def by_msm_batch(ctx, pts, neg, offsets):
    return ctx.msm_batch(pts, unit_scalars(len(pts), neg), offsets)


def signs(n, seed):
    """none, all, random (any non-zero byte subtracts)"""
    r = np.random.RandomState(seed).randint(0, 2, size=n).astype(np.uint8) * np.uint8(1 + seed % 200)
    return [None, np.full(n, 0xFF, np.uint8), r]


@pytest.fixture(scope="module")
def pool(gpu_ctx, golden):
    """points of the whole group, generated once and never written; every test takes a prefix"""
    pts = group_points(gpu_ctx, golden, POOL, seed_offset=0x95)
    pts.setflags(write=False)
    return pts


SHAPES = {
    "one_0": [0], "one_1": [1], "one_2": [2], "one_63": [63], "one_64": [64], "one_65": [65], "one_T-1": [T - 1], "one_T": [T],
    "one_T+1": [T + 1], "one_4T+1": [4 * T + 1],
    "mixed": [b - a for a, b in zip(MIXED, MIXED[1:])],
    "5000_short": [int(v) for v in np.random.RandomState(0x5000).randint(0, 8, size=5000)],
    "long_then_short": [3 * T] + [3] * 500,
    "short_then_long": [3] * 500 + [3 * T],
    "2T_singletons": [1] * (2 * T),
    "T_shifted_by_1": [1] + [T] * 4 + [T - 1],
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_parity_with_msm_batch(gpu_ctx, pool, shape):
    off = offsets_of(SHAPES[shape])
    n = off[-1]
    assert n <= POOL
    pts = pool[:n]
    for k, neg in enumerate(signs(n, 7 + len(shape))):
        want, wst = by_msm_batch(gpu_ctx, pts, neg, off)
        got, st = ok_sum(gpu_ctx, pts, neg, off)
        assert (wst == -1).all() and (st == wst).all() and (got == want).all(), (shape, k)


def test_mixed_equals_the_oracle_composition(gpu_ctx, oracle, pool):
    pts = pool[:300]
    neg = signs(300, 3)[2]
    sc = unit_scalars(300, neg)
    composed = np.concatenate([oracle_msm(oracle, pts[a:b], sc[a:b]) for a, b in zip(MIXED, MIXED[1:])])
    got, st = ok_sum(gpu_ctx, pts, neg, MIXED)
    assert (st == -1).all() and (got == composed).all() and (got[1] == IDENTITY).all()
    out, st = gpu_ctx.point_sum(pts, MIXED, neg)
    assert (st == -1).all() and (out == composed).all()


OFF_TILE = [0, 1, 1, 2, T // 4, T // 4 + 1, 2 * T + 1, 3 * T, 3 * T + 44]   # segment 5 crosses the tile boundaries T and 2 T, 6 ends at 3 T


def test_off_curve_points_spoil_only_their_segment(gpu_ctx, pool):
    n = OFF_TILE[-1]
    pts = pool[:n]
    alt = (np.arange(n) % 2).astype(np.uint8)
    for neg in (None, alt):
        clean, st = ok_sum(gpu_ctx, pts, neg, OFF_TILE)
        assert (st == -1).all()
        # first / last of a segment; both sides of a tile boundary inside one segment (the smaller index wins) and between two
        # segments; two in one segment in either order; subtracted ones (alt: the odd indices); single-point segments; the ends
        for bad in ([2], [T // 4 - 1], [T // 4 + 1], [2 * T], [T - 1, T], [2 * T, 2 * T - 1], [3 * T, 3 * T - 1], [T + 5, T // 4 + 3],
                    [T + 4], [T + 5], [0, T // 4, n - 1], [1, 2, 3]):
            p = pts.copy()
            for i in bad:
                p[i, 0] ^= 1
            got, st = ok_sum(gpu_ctx, p, neg, OFF_TILE)
            want, wst = by_msm_batch(gpu_ctx, p, neg, OFF_TILE)
            assert (st == wst).all() and (got == want).all(), bad
            for s, (a, b) in enumerate(zip(OFF_TILE, OFF_TILE[1:])):
                hit = [i for i in bad if a <= i < b]
                assert st[s] == (min(hit) if hit else -1), (bad, s)
                assert (got[s] == (ZERO[0] if hit else clean[s])).all(), (bad, s)
        got, st = ok_sum(gpu_ctx, pts, neg, OFF_TILE)               # the next clean call is unaffected
        assert (st == -1).all() and (got == clean).all()


def test_no_segments_and_empty_segments(gpu_ctx):
    e = np.zeros(0, np.uint8)
    rc, out, st = raw_sum(gpu_ctx, e, None, [0])
    assert rc == 0 and out.shape == (0, 64)
    assert raw_sum(gpu_ctx, pack([(0, 1)]), None, [0])[0] == -1            # m == 0 requires n == 0
    for neg in (None, e):
        got, st = ok_sum(gpu_ctx, e, neg, [0, 0, 0])
        assert st.tolist() == [-1, -1] and (got == np.repeat(IDENTITY, 2, axis=0)).all()
    out, st = gpu_ctx.point_sum([], [0, 0, 0, 0])
    assert out.shape == (3, 64) and st.tolist() == [-1] * 3 and (out == IDENTITY).all()


@pytest.mark.parametrize("kind", sorted(BAD_OFFSETS))
def test_host_form_rejects_bad_offsets(gpu_ctx, pool, kind):
    rc, out, st = raw_sum(gpu_ctx, pool[:300], None, BAD_OFFSETS[kind])
    assert rc == -1 and b"offsets" in gpu_ctx.lib.bjj_last_error()
    assert (out == 0xAB).all() and (st == 12345).all()          # nothing was written


def test_null_arguments_are_invalid_and_write_nothing(gpu_ctx, pool):
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    pts = np.ascontiguousarray(pool[:4]).reshape(-1)
    off = np.asarray([0, 4], np.uint64)
    out, st = np.full(64, 0xAB, np.uint8), np.full(1, 12345, np.int64)
    P, O, R, S = pts.ctypes.data, off.ctypes.data, out.ctypes.data, st.ctypes.data
    for args in ((None, P, None, 4, O, 1, R, S), (h, None, None, 4, O, 1, R, S), (h, P, None, 4, None, 1, R, S), (h, P, None, 4, O, 1, None, S),
                 (h, P, None, 4, O, 1, R, None), (h, P, None, 1 << 32, O, 1, R, S), (h, P, None, 4, O, 1 << 32, R, S)):
        assert lib.bjj_point_sum(*args) == -1, args
        assert lib.bjj_point_sum_dev(*args, None) == -1, args
    assert lib.bjj_point_sum_dev(h, (P & ~15) + 8, None, 4, O, 1, R, S, None) == -1 and b"aligned" in lib.bjj_last_error()
    assert (out == 0xAB).all() and st[0] == 12345


def _dev_call(ctx, pts, neg, offsets, stream=0):
    import torch
    dev = torch.device("cuda", 0)
    m, n = len(offsets) - 1, len(pts)
    d_p = torch.from_numpy(np.array(pts).reshape(-1)).to(dev)
    d_g = None
    if neg is not None:
        d_g = torch.zeros(n + 1, dtype=torch.uint8, device=dev)
        d_g[1:] = torch.from_numpy(np.array(neg, np.uint8)).to(dev)
        assert (d_g.data_ptr() + 1) % 2 == 1
    d_off = torch.from_numpy(np.asarray(offsets, np.uint64).view(np.int64)).to(dev)
    d_out = torch.full((m * 64,), 0xAB, dtype=torch.uint8, device=dev)
    d_st = torch.full((m + 1,), 12345, dtype=torch.int64, device=dev)
    ctx.point_sum_dev(d_p.data_ptr(), d_g.data_ptr() + 1 if d_g is not None else None, n, d_off.data_ptr(), m, d_out.data_ptr(),
                      d_st.data_ptr(), stream)
    ctx.sync()
    st = d_st.cpu().numpy()
    assert st[m] == 12345
    return d_out.cpu().numpy().reshape(m, 64), st[:m]


@pytest.mark.parametrize("kind", sorted(BAD_OFFSETS))
def test_device_form_reports_bad_offsets_as_data(gpu_ctx, pool, kind):
    got, st = _dev_call(gpu_ctx, pool[:300], signs(300, 5)[2], BAD_OFFSETS[kind])
    assert st.tolist() == [-2] * 3 and (got == 0).all()


def test_pinned_pageable_and_device_forms_agree(gpu_ctx, pool):
    n = 2 * T + 44
    off = [0, 1, 1, 2, T + 7, n]
    pts, neg = pool[:n], signs(n, 11)[2]
    want, wst = by_msm_batch(gpu_ctx, pts, neg, off)
    pageable, st = ok_sum(gpu_ctx, pts, neg, off)
    assert (st == wst).all() and (pageable == want).all()
    pp, pg = gpu_ctx.host_empty(n * 64), gpu_ctx.host_empty(n)
    try:
        pp[:] = pts.reshape(-1)
        pg[:] = neg
        assert gpu_ctx.host_is_pinned(pp) and gpu_ctx.host_is_pinned(pg)
        out, st = np.full(5 * 64, 0xAB, np.uint8), np.full(5, 12345, np.int64)
        o = np.asarray(off, np.uint64)
        assert gpu_ctx.lib.bjj_point_sum(gpu_ctx.handle, pp.ctypes.data, pg.ctypes.data, n, o.ctypes.data, 5, out.ctypes.data, st.ctypes.data) == 0
        assert (st == wst).all() and (out.reshape(5, 64) == want).all()
    finally:
        gpu_ctx.host_free(pp)
        gpu_ctx.host_free(pg)
    got, st = _dev_call(gpu_ctx, pts, neg, off)
    assert (st == wst).all() and (got == want).all()
    got, st = _dev_call(gpu_ctx, pts, None, off)
    assert (got == by_msm_batch(gpu_ctx, pts, None, off)[0]).all()


def test_two_streams_at_once(gpu_ctx, pool):
    import torch
    dev = torch.device("cuda", 0)
    cases = []
    for s in range(2):
        lengths = np.random.RandomState(77 + s).randint(0, 60, size=64)
        off = offsets_of(lengths)
        n = off[-1]
        pts = pool[1000 * s:1000 * s + n]
        neg = signs(n, 20 + s)[2]
        d = (torch.from_numpy(np.array(pts).reshape(-1)).to(dev), torch.from_numpy(neg).to(dev),
             torch.from_numpy(np.asarray(off, np.uint64).view(np.int64)).to(dev))
        cases.append((n, d))
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]

    def run(which):
        outs = [(torch.zeros(64 * 64, dtype=torch.uint8, device=dev), torch.zeros(64, dtype=torch.int64, device=dev)) for _ in range(2)]
        torch.cuda.synchronize()
        for s in range(2):
            n, d = cases[s]
            gpu_ctx.point_sum_dev(d[0].data_ptr(), d[1].data_ptr(), n, d[2].data_ptr(), 64, outs[s][0].data_ptr(), outs[s][1].data_ptr(),
                                  stream=streams[which[s]].cuda_stream)
        gpu_ctx.sync()
        torch.cuda.synchronize()
        return [(o.cpu().numpy(), st.cpu().numpy()) for o, st in outs]

    one = run((0, 0))
    assert not (one[0][0] == one[1][0]).all()                        # different inputs
    for s in range(2):
        assert (one[s][1] == -1).all()
    for rep in range(3):
        two = run((0, 1))
        for s in range(2):
            assert (two[s][0] == one[s][0]).all() and (two[s][1] == one[s][1]).all(), (rep, s)


def test_elgamal_tally(gpu_ctx):
    """64 voters, 3 candidates, plaintexts 0 or 1: the per-candidate sums of the ciphertexts decrypt to the per-candidate counts"""
    rng = np.random.default_rng(0x7A11)
    voters, cands = 64, 3
    n = voters * cands
    suborder = ORDER8 // 8
    sk = int.from_bytes(rng.bytes(31), "little") % suborder
    votes = rng.integers(0, 2, size=(cands, voters))
    ms = [int(v) for v in votes.reshape(-1)]
    rs = [int.from_bytes(rng.bytes(31), "little") for _ in range(n)]
    pk = tuple(unpack(gpu_ctx.mul_fixed_base(pack([sk])), 2)[0])
    base = gpu_ctx.base(pk, 8)
    try:
        c1 = gpu_ctx.mul_fixed_base(pack(rs))
        c2 = gpu_ctx.mul_bases([None, base], [pack(ms), pack(rs)])
    finally:
        base.close()
    off = [voters * k for k in range(cands + 1)]
    table = gpu_ctx.dlog_table(None, 16)
    try:
        s1, s2, st = gpu_ctx.elgamal_sum(c1, c2, off)
        assert st.tolist() == [-1] * cands
        m, ok = gpu_ctx.elgamal_decrypt(table, sk, s1, s2, 16)
        assert (ok == 1).all() and [int(v) for v in m] == [int(v) for v in votes.sum(axis=1)]
        # a balance: the first half of every segment credited, the second half debited
        neg = np.tile(np.repeat([0, 1], voters // 2), cands).astype(np.uint8)
        d1, d2, st = gpu_ctx.elgamal_sum(c1, c2, off, neg)
        diff = votes[:, :voters // 2].sum(axis=1) - votes[:, voters // 2:].sum(axis=1)
        m, ok = gpu_ctx.elgamal_decrypt(table, sk, d1, d2, 16)
        for k in range(cands):
            assert (ok[k], int(m[k])) == ((1, int(diff[k])) if diff[k] >= 0 else (0, (1 << 64) - 1)), k
        # status: the smaller non-negative word of the two components
        b1, b2 = c1.copy(), c2.copy()
        b1[70, 0] ^= 1
        b2[66, 0] ^= 1
        b2[130, 0] ^= 1
        _, _, st = gpu_ctx.elgamal_sum(b1, b2, off)
        assert st.tolist() == [-1, 66, 130]
    finally:
        table.close()


def test_module_level_point_sum(gpu_ctx, pool):
    import babyjubjub_rs_amd as bjj
    P = [bjj.Point(x, y) for x, y in unpack(pool[:6], 2)]
    got = bjj.point_sum([[P[0], P[1], P[2]], [], [P[3], (P[3], True)], [(P[4], True), (P[5].x, P[5].y)]], ctx=gpu_ctx)
    want, st = gpu_ctx.point_sum(pool[:3], [0, 3])
    assert (got[0].x, got[0].y) == tuple(unpack(want, 2)[0]) and (got[1].x, got[1].y) == (0, 1) == (got[2].x, got[2].y)
    want, st = gpu_ctx.point_sum(pool[4:6], [0, 2], [1, 0])
    assert (got[3].x, got[3].y) == tuple(unpack(want, 2)[0])
    assert bjj.point_sum([], ctx=gpu_ctx) == []
    with pytest.raises(bjj.BjjError, match="segment 1: point 1 is not on the curve"):
        bjj.point_sum([[P[0]], [P[1], (P[2].x ^ 1, P[2].y)]], ctx=gpu_ctx)
