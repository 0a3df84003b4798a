"""bjj_msm_batch on the MI355X: m sums over CSR segments in one call.  Every segment is expected to be byte for byte what bjj_msm
gives for its slice (gpu_ctx.msm) and, for the small shapes, what the C oracle composes (mul_var_base, then a point_add tree)."""
import ctypes

import numpy as np
import pytest

from conftest import ints, pack
from test_gpu_msm import IDENTITY, ZERO, _golden, group_points, oracle_msm, raw_msm, scalars

pytestmark = pytest.mark.gpu

MIXED = [0, 1, 1, 2, 64, 65, 129, 300]
BAD_OFFSETS = {"non_monotone": [0, 200, 100, 300], "first_not_zero": [1, 100, 200, 300], "last_not_n": [0, 100, 200, 299]}


def raw_batch(ctx, pts, sc, offsets, window_bits=0):
    """bjj_msm_batch as the C ABI returns it: rc, (m, 64) result bytes, (m,) status words (pre-filled with a sentinel)"""
    pts = np.ascontiguousarray(pts, np.uint8).reshape(-1)
    sc = np.ascontiguousarray(sc, np.uint8).reshape(-1)
    off = np.ascontiguousarray(offsets, np.uint64)
    n, m = sc.size // 32, off.size - 1
    out = np.full(max(m, 1) * 64, 0xAB, np.uint8)
    st = np.full(max(m, 1), 12345, np.int64)
    rc = ctx.lib.bjj_msm_batch(ctx.handle, pts.ctypes.data if n else None, sc.ctypes.data if n else None, n, off.ctypes.data, m, window_bits,
                               out.ctypes.data, st.ctypes.data)
    return rc, out[:m * 64].reshape(m, 64), st[:m]


def ok_batch(ctx, pts, sc, offsets, window_bits=0):
    rc, out, st = raw_batch(ctx, pts, sc, offsets, window_bits)
    assert rc == 0, ctx.lib.bjj_last_error()
    return out, st


def per_slice(ctx, pts, sc, offsets):
    """(m, 64): bjj_msm of every slice"""
    return np.concatenate([ctx.msm(pts[a:b], sc[a:b]) for a, b in zip(offsets, offsets[1:])])


def offsets_of(lengths):
    return [0] + [int(v) for v in np.cumsum(np.asarray(lengths, np.int64))]


@pytest.fixture(scope="module")
def mixed(gpu_ctx, oracle, golden):
    """300 points of the whole group, their scalars, and the expected result of every segment of MIXED: computed once, never written"""
    pts = group_points(gpu_ctx, golden, 300, seed_offset=0xB47)
    sc = scalars(300, offset=0xB47)
    want = per_slice(gpu_ctx, pts, sc, MIXED)
    composed = np.concatenate([oracle_msm(oracle, pts[a:b], sc[a:b]) for a, b in zip(MIXED, MIXED[1:])])
    assert (want == composed).all() and (want[1] == IDENTITY).all()
    for a in (pts, sc, want):
        a.setflags(write=False)
    return pts, sc, want


@pytest.mark.parametrize("n", [0, 1, 65, 4097])
def test_one_segment_equals_bjj_msm(gpu_ctx, golden, n):
    pts = group_points(gpu_ctx, golden, n, seed_offset=n) if n else np.zeros((0, 64), np.uint8)
    sc = scalars(n, offset=n) if n else np.zeros((0, 32), np.uint8)
    want, wst = raw_msm(gpu_ctx, pts, sc)
    for wb in (0, 4, 9):
        got, st = ok_batch(gpu_ctx, pts, sc, [0, n], wb)
        assert st.tolist() == [wst] == [-1] and (got == want).all(), wb
    if n > 1:   # the status word of an off-curve point is bjj_msm's
        p = pts.copy()
        p[n - 2, 0] ^= 1
        got, st = ok_batch(gpu_ctx, p, sc, [0, n])
        assert raw_msm(gpu_ctx, p, sc)[1] == n - 2 and st.tolist() == [n - 2] and (got == ZERO).all()


@pytest.mark.parametrize("wb", [0, 4, 5, 8, 13])
def test_mixed_segments(gpu_ctx, mixed, wb):
    pts, sc, want = mixed
    got, st = ok_batch(gpu_ctx, pts, sc, MIXED, wb)
    assert st.tolist() == [-1] * 7 and (got == want).all()


def test_no_segments_and_empty_segments(gpu_ctx):
    e = np.zeros(0, np.uint8)
    rc, out, st = raw_batch(gpu_ctx, e, e, [0])
    assert rc == 0 and out.shape == (0, 64)
    one = pack([(0, 1)])
    assert raw_batch(gpu_ctx, one, pack([1]), [0])[0] == -1            # m == 0 requires n == 0
    got, st = ok_batch(gpu_ctx, e, e, [0, 0, 0])
    assert st.tolist() == [-1, -1] and (got == np.repeat(IDENTITY, 2, axis=0)).all()
    out, st = gpu_ctx.msm_batch([], [], [0, 0, 0, 0])
    assert out.shape == (3, 64) and st.tolist() == [-1] * 3 and (out == IDENTITY).all()


def test_5000_short_segments(gpu_ctx, golden):
    """more segments than a workgroup of the finish has lanes, lengths 0..7; expected: mul_var_base per item, then one addition chain
    per segment position (the same group sums in another order)"""
    rng = np.random.RandomState(0x5000)
    lengths = rng.randint(0, 8, size=5000)
    off = offsets_of(lengths)
    n = off[-1]
    pts = group_points(gpu_ctx, golden, n, seed_offset=5000)
    sc = scalars(n, offset=5000)
    prod = gpu_ctx.mul_var_base(pts, sc)
    want = np.repeat(IDENTITY, 5000, axis=0)
    starts = np.asarray(off[:-1])
    for t in range(7):
        sel = np.nonzero(lengths > t)[0]
        want[sel] = gpu_ctx.point_add(want[sel], prod[starts[sel] + t])
    got, st = ok_batch(gpu_ctx, pts, sc, off)
    assert (st == -1).all() and (got == want).all()
    for s in (0, 1, 2499, 4999):   # and bjj_msm itself on a few slices
        assert (gpu_ctx.msm(pts[off[s]:off[s + 1]], sc[off[s]:off[s + 1]]) == got[s]).all()


def test_one_long_segment_before_many_short_ones(gpu_ctx, golden):
    lengths = [70000] + [3] * 500
    off = offsets_of(lengths)
    n = off[-1]
    pts = group_points(gpu_ctx, golden, n, seed_offset=70000)
    sc = scalars(n, offset=70000)
    got, st = ok_batch(gpu_ctx, pts, sc, off)
    assert (st == -1).all()
    assert (got[0] == gpu_ctx.msm(pts[:70000], sc[:70000])[0]).all()
    prod = gpu_ctx.mul_var_base(pts[70000:], sc[70000:]).reshape(500, 3, 64)
    want = gpu_ctx.point_add(gpu_ctx.point_add(prod[:, 0], prod[:, 1]), prod[:, 2])
    assert (got[1:] == want).all()


@pytest.mark.parametrize("c", [4, 8])
def test_equal_scalars_boundary_every_five_points(gpu_ctx, oracle, golden, c):
    """every item has the same digit in every window: neighbouring lanes of a wave differ only in the segment part of the key"""
    n = 1000
    pts = group_points(gpu_ctx, golden, n, seed_offset=0xE5)
    k = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDE
    sc = pack([k] * n).reshape(n, 32)
    off = list(range(0, n + 1, 5))
    g = pts.reshape(200, 5, 64)
    psum = g[:, 0]
    for t in range(1, 5):
        psum = oracle.point_add(np.ascontiguousarray(psum), np.ascontiguousarray(g[:, t]))
    want = oracle.mul_var_base(psum, sc[:200])
    got, st = ok_batch(gpu_ctx, pts, sc, off, c)
    assert (st == -1).all() and (got == want).all()


def test_off_curve_points_spoil_only_their_segment(gpu_ctx, mixed):
    pts, sc, clean = mixed
    for bad in ([70], [100, 66], [0, 64, 299]):
        p = pts.copy()
        for i in bad:
            p[i, 0] ^= 1
        got, st = ok_batch(gpu_ctx, p, sc, MIXED)
        for s, (a, b) in enumerate(zip(MIXED, MIXED[1:])):
            hit = [i for i in bad if a <= i < b]
            assert st[s] == (min(hit) if hit else -1), (bad, s)
            assert (got[s] == (ZERO[0] if hit else clean[s])).all(), (bad, s)
        got, st = ok_batch(gpu_ctx, pts, sc, MIXED)             # the next clean call is unaffected
        assert (st == -1).all() and (got == clean).all()


@pytest.mark.parametrize("kind", sorted(BAD_OFFSETS))
def test_host_form_rejects_bad_offsets(gpu_ctx, mixed, kind):
    pts, sc, _ = mixed
    rc, out, st = raw_batch(gpu_ctx, pts, sc, BAD_OFFSETS[kind])
    assert rc == -1 and b"offsets" in gpu_ctx.lib.bjj_last_error()
    assert (out == 0xAB).all() and (st == 12345).all()          # nothing was written


def test_key_range_is_invalid(gpu_ctx):
    n, m = 400, 400
    pts, sc = np.repeat(pack([(0, 1)]).reshape(1, 64), n, axis=0), np.zeros((n, 32), np.uint8)
    rc, _, _ = raw_batch(gpu_ctx, pts, sc, list(range(m + 1)), 20)          # 400 * 13 * 2^19 >= 2^31
    assert rc == -1 and b"2^31" in gpu_ctx.lib.bjj_last_error()
    for wb in (-1, 3, 21):
        assert raw_batch(gpu_ctx, pts, sc, list(range(m + 1)), wb)[0] == -1
    got, st = ok_batch(gpu_ctx, pts, sc, list(range(m + 1)), 0)
    assert (st == -1).all() and (got == IDENTITY).all()


def _dev_call(ctx, pts, sc, offsets, stream=0, window_bits=0):
    import torch
    dev = torch.device("cuda", 0)
    m = len(offsets) - 1
    d_p, d_s = torch.from_numpy(np.array(pts).reshape(-1)).to(dev), torch.from_numpy(np.array(sc).reshape(-1)).to(dev)
    d_off = torch.from_numpy(np.asarray(offsets, np.uint64).view(np.int64)).to(dev)
    d_out = torch.full((m * 64,), 0xAB, dtype=torch.uint8, device=dev)
    d_st = torch.full((m + 1,), 12345, dtype=torch.int64, device=dev)
    ctx.msm_batch_dev(d_p.data_ptr(), d_s.data_ptr(), len(pts), d_off.data_ptr(), m, d_out.data_ptr(), d_st.data_ptr(), window_bits, stream)
    ctx.sync()
    st = d_st.cpu().numpy()
    assert st[m] == 12345
    return d_out.cpu().numpy().reshape(m, 64), st[:m]


@pytest.mark.parametrize("kind", sorted(BAD_OFFSETS))
def test_device_form_reports_bad_offsets_as_data(gpu_ctx, mixed, kind):
    pts, sc, _ = mixed
    got, st = _dev_call(gpu_ctx, pts, sc, BAD_OFFSETS[kind])
    assert st.tolist() == [-2] * 3 and (got == 0).all()


def test_pinned_pageable_and_device_forms_agree(gpu_ctx, mixed):
    pts, sc, want = mixed
    pp, ps = gpu_ctx.host_empty(300 * 64), gpu_ctx.host_empty(300 * 32)
    try:
        pp[:] = pts.reshape(-1)
        ps[:] = sc.reshape(-1)
        assert gpu_ctx.host_is_pinned(pp)
        pinned, st = ok_batch(gpu_ctx, pp, ps, MIXED)
        assert (st == -1).all() and (pinned == want).all()
    finally:
        gpu_ctx.host_free(pp)
        gpu_ctx.host_free(ps)
    got, st = _dev_call(gpu_ctx, pts, sc, MIXED)
    assert (st == -1).all() and (got == want).all()
    out, st = gpu_ctx.msm_batch(pts, sc, MIXED)
    assert (st == -1).all() and (out == want).all()


def test_two_streams_at_once(gpu_ctx, golden):
    import torch
    dev = torch.device("cuda", 0)
    cases = []
    for s in range(2):
        lengths = np.random.RandomState(77 + s).randint(0, 200, size=64)
        off = offsets_of(lengths)
        n = off[-1]
        pts = group_points(gpu_ctx, golden, n, seed_offset=200 + s)
        sc = scalars(n, offset=200 + s)
        cases.append((n, off, pts, sc, per_slice(gpu_ctx, pts, sc, off)))
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    dev_in = [(torch.from_numpy(p.reshape(-1)).to(dev), torch.from_numpy(k.reshape(-1)).to(dev),
               torch.from_numpy(np.asarray(off, np.uint64).view(np.int64)).to(dev)) for _, off, p, k, _ in cases]
    outs = [(torch.zeros(64 * 64, dtype=torch.uint8, device=dev), torch.zeros(64, dtype=torch.int64, device=dev)) for _ in range(2)]
    torch.cuda.synchronize()
    for rep in range(3):
        for s in range(2):
            gpu_ctx.msm_batch_dev(dev_in[s][0].data_ptr(), dev_in[s][1].data_ptr(), cases[s][0], dev_in[s][2].data_ptr(), 64,
                                  outs[s][0].data_ptr(), outs[s][1].data_ptr(), window_bits=0, stream=streams[s].cuda_stream)
        gpu_ctx.sync()
        for s in range(2):
            assert (outs[s][1].cpu().numpy() == -1).all()
            assert (outs[s][0].cpu().numpy().reshape(64, 64) == cases[s][4]).all(), (rep, s)
            outs[s][0].zero_()
        torch.cuda.synchronize()


def test_module_level_msm_batch(gpu_ctx):
    import babyjubjub_rs_amd as bjj
    cases = _golden()[:4]
    segs = [([bjj.Point(*ints(p)) for p in c["points"]], [ints(k) for k in c["scalars"]]) for c in cases]
    segs.insert(2, ([], []))
    got = bjj.msm_batch(segs, ctx=gpu_ctx)
    want = [ints(c["result"]) for c in cases]
    want.insert(2, (0, 1))
    assert [(q.x, q.y) for q in got] == want
    assert bjj.msm_batch([], ctx=gpu_ctx) == []
    pts, ks = segs[3]
    assert len(pts) >= 1
    segs[3] = ([bjj.Point(p.x ^ 1, p.y) if i == len(pts) - 1 else p for i, p in enumerate(pts)], ks)
    with pytest.raises(bjj.BjjError, match="segment 3: point %d is not on the curve" % (len(pts) - 1)):
        bjj.msm_batch(segs, ctx=gpu_ctx)
