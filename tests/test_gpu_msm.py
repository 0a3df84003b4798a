"""bjj_msm on the MI355X: Q = sum k_i * P_i.  Expected values come from the C oracle (mul_var_base, then a pairwise tree of
point_add -- the reference's mul_scalar and PointProjective::add + affine) and from tests/golden/msm_expected.json (the reference
fold, written by tests/golden/make_msm_expected.py); the pure-Python oracle is not used here."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import ROOT, ints, pack

pytestmark = pytest.mark.gpu

L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
ORDER8 = 8 * L
IDENTITY = pack([(0, 1)]).reshape(1, 64)
ZERO = np.zeros((1, 64), np.uint8)


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "msm_expected.json")) as f:
        return json.load(f)["cases"]


def raw_msm(ctx, pts, sc, window_bits=0):
    """bjj_msm as the C ABI returns it: (64 result bytes, status word)"""
    pts = np.ascontiguousarray(pts, np.uint8).reshape(-1)
    sc = np.ascontiguousarray(sc, np.uint8).reshape(-1)
    n = sc.size // 32
    out = np.empty(64, np.uint8)
    first = ctypes.c_int64(12345)
    rc = ctx.lib.bjj_msm(ctx.handle, pts.ctypes.data if n else None, sc.ctypes.data if n else None, n, window_bits,
                         out.ctypes.data, ctypes.byref(first))
    assert rc == 0, ctx.lib.bjj_last_error()
    return out.reshape(1, 64), first.value


def tree_sum(add, pts):
    """pairwise tree of affine additions (an odd element waits for the next level)"""
    pts = np.ascontiguousarray(pts, np.uint8).reshape(-1, 64)
    if len(pts) == 0:
        return IDENTITY.copy()
    while len(pts) > 1:
        h = len(pts) // 2
        s = add(pts[0:2 * h:2], pts[1:2 * h:2])
        pts = np.concatenate([s, pts[2 * h:]]) if len(pts) % 2 else s
    return np.ascontiguousarray(pts[:1])


def oracle_msm(oracle, pts, sc):
    return tree_sum(oracle.point_add, oracle.mul_var_base(pts, sc))


def group_points(ctx, golden, n, seed_offset=0):
    """k_i * B8 + c_i * T8 (the whole group: every 3rd point torsion-shifted), generated on the device"""
    from babyjubjub_rs_amd import workload as w
    k = w.from_ints([v % L for v in w.to_ints(w.random_u256(w.SEED_POINTS, n, seed_offset))])
    c = (w.splitmix64(w.SEED_POINTS ^ 0x3D, n, seed_offset) & np.uint64(7)).astype(np.int64)
    c[np.arange(n) % 3 != 0] = 0
    tors = pack([ints(t) for t in golden["gpu_expected"]["torsion_points"]]).reshape(8, 64)
    return gpu_add(ctx, ctx.mul_fixed_base(k), tors[c])


def gpu_add(ctx, p, q):
    return ctx.point_add(p, q).copy()


def scalars(n, offset=0):
    from babyjubjub_rs_amd import workload as w
    return w.random_u256(w.SEED_SCALARS ^ 0x4D53, n, offset)


def test_golden_cases(gpu_ctx):
    for case in _golden():
        pts = pack([ints(p) for p in case["points"]])
        sc = pack([ints(k) for k in case["scalars"]])
        want = pack([ints(case["result"])]).reshape(1, 64)
        for wb in (0, 4, 7, 13):
            got, st = raw_msm(gpu_ctx, pts, sc, wb)
            assert st == -1 and (got == want).all(), (case["name"], wb)


def test_empty_is_the_identity(gpu_ctx):
    got, st = raw_msm(gpu_ctx, np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    assert st == -1 and (got == IDENTITY).all()
    assert (gpu_ctx.msm([], []) == IDENTITY).all()


def test_one_point_equals_mul_var_base(gpu_ctx, golden):
    pts = group_points(gpu_ctx, golden, 8)
    sc = scalars(8)
    for i in range(8):
        want = gpu_ctx.mul_var_base(pts[i:i + 1], sc[i:i + 1])
        assert (gpu_ctx.msm(pts[i:i + 1], sc[i:i + 1]) == want).all()


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 257, 4097, 65537, 1 << 20])
def test_random_against_oracle(gpu_ctx, oracle, golden, n):
    pts = group_points(gpu_ctx, golden, n, seed_offset=n)
    sc = scalars(n, offset=n)
    assert (gpu_ctx.msm(pts, sc) == oracle_msm(oracle, pts, sc)).all()


def test_every_window_gives_the_same_bytes(gpu_ctx, oracle, golden):
    n = 4097
    pts = group_points(gpu_ctx, golden, n, seed_offset=7)
    sc = scalars(n, offset=7)
    want = oracle_msm(oracle, pts, sc)
    for wb in [0] + list(range(4, 21)):
        got, st = raw_msm(gpu_ctx, pts, sc, wb)
        assert st == -1 and (got == want).all(), wb


def test_bad_window_is_invalid(gpu_ctx):
    out = np.empty(64, np.uint8)
    first = ctypes.c_int64(0)
    pts, sc = pack([(0, 1)]), pack([1])
    for wb in (-1, 1, 3, 21, 64):
        assert gpu_ctx.lib.bjj_msm(gpu_ctx.handle, pts.ctypes.data, sc.ctypes.data, 1, wb, out.ctypes.data, ctypes.byref(first)) == -1


def _one(oracle, p, k):
    return oracle.mul_var_base(np.ascontiguousarray(p).reshape(1, 64), pack([k]).reshape(1, 32))


def test_skewed_inputs_1m(gpu_ctx, oracle, golden):
    n = 1 << 20
    pts = group_points(gpu_ctx, golden, n, seed_offset=11)
    psum = tree_sum(oracle.point_add, pts)
    k = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDE
    # all scalars equal: k * sum P
    got, st = raw_msm(gpu_ctx, pts, pack([k] * n))
    assert st == -1 and (got == _one(oracle, psum, k)).all()
    # every digit of every scalar in ONE bucket (c = 16: digit 1 in all 16 windows)
    u = sum(1 << (16 * j) for j in range(16))
    got, st = raw_msm(gpu_ctx, pts, pack([u] * n), 16)
    assert st == -1 and (got == _one(oracle, psum, u)).all()
    # all points equal: (sum k_i mod 8l) * P
    sc = scalars(n, offset=11)
    from babyjubjub_rs_amd import workload as w
    ksum = sum(w.to_ints(sc)) % ORDER8
    same = np.repeat(pts[5:6], n, axis=0)
    got, st = raw_msm(gpu_ctx, same, sc)
    assert st == -1 and (got == _one(oracle, pts[5], ksum)).all()
    # half of the scalars zero
    half = sc.copy()
    half[::2] = 0
    got, st = raw_msm(gpu_ctx, pts, half)
    assert st == -1 and (got == oracle_msm(oracle, pts[1::2], sc[1::2])).all()


def test_off_curve_points_are_data(gpu_ctx, oracle, golden):
    n = 1000
    pts = group_points(gpu_ctx, golden, n, seed_offset=3)
    sc = scalars(n, offset=3)
    want = oracle_msm(oracle, pts, sc)
    for bad in ([0], [n // 2], [n - 1], [999, 17, 640, 18]):
        p = pts.copy()
        for i in bad:
            p[i, 0] ^= 1
        got, st = raw_msm(gpu_ctx, p, sc)
        assert st == min(bad) and (got == ZERO).all(), bad
        got, st = raw_msm(gpu_ctx, pts, sc)                   # the next clean call is unaffected
        assert st == -1 and (got == want).all()
    import babyjubjub_rs_amd as bjj
    p = pts.copy()
    p[n // 2, 0] ^= 1
    with pytest.raises(bjj.BjjError, match="point %d is not on the curve" % (n // 2)):
        gpu_ctx.msm(p, sc)


def test_pinned_pageable_and_device_forms_agree(gpu_ctx, golden):
    import torch
    n = 70000
    pts = group_points(gpu_ctx, golden, n, seed_offset=5)
    sc = scalars(n, offset=5)
    pageable, st = raw_msm(gpu_ctx, pts, sc)
    assert st == -1
    pp, ps = gpu_ctx.host_empty(n * 64), gpu_ctx.host_empty(n * 32)
    try:
        pp[:] = pts.reshape(-1)
        ps[:] = sc.reshape(-1)
        assert gpu_ctx.host_is_pinned(pp)
        pinned, st = raw_msm(gpu_ctx, pp, ps)
        assert st == -1 and (pinned == pageable).all()
    finally:
        gpu_ctx.host_free(pp)
        gpu_ctx.host_free(ps)
    dev = torch.device("cuda", 0)
    d_p, d_s = torch.from_numpy(pts.reshape(-1)).to(dev), torch.from_numpy(sc.reshape(-1)).to(dev)
    d_out, d_st = torch.zeros(64, dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    gpu_ctx.msm_dev(d_p.data_ptr(), d_s.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr())
    gpu_ctx.sync()
    assert int(d_st[0]) == -1 and (d_out.cpu().numpy().reshape(1, 64) == pageable).all()


def test_two_streams_at_once(gpu_ctx, oracle, golden):
    import torch
    dev = torch.device("cuda", 0)
    n = 1 << 16
    cases = []
    for s in range(2):
        pts = group_points(gpu_ctx, golden, n, seed_offset=100 + s)
        sc = scalars(n, offset=100 + s)
        cases.append((pts, sc, oracle_msm(oracle, pts, sc)))
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    dev_in = [(torch.from_numpy(p.reshape(-1)).to(dev), torch.from_numpy(s.reshape(-1)).to(dev)) for p, s, _ in cases]
    outs = [(torch.zeros(64, dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)) for _ in range(2)]
    torch.cuda.synchronize()
    for rep in range(3):
        for s in range(2):
            gpu_ctx.msm_dev(dev_in[s][0].data_ptr(), dev_in[s][1].data_ptr(), n, outs[s][0].data_ptr(), outs[s][1].data_ptr(),
                            window_bits=0, stream=streams[s].cuda_stream)
        gpu_ctx.sync()
        for s in range(2):
            assert int(outs[s][1][0]) == -1
            assert (outs[s][0].cpu().numpy().reshape(1, 64) == cases[s][2]).all(), (rep, s)


def test_4m_against_the_gpu_composition(gpu_ctx, golden):
    """2^22 random inputs: bjj_msm against what callers compose today -- bjj_mul_var_base, then a bjj_point_add tree"""
    n = 1 << 22
    pts = group_points(gpu_ctx, golden, n, seed_offset=1 << 22)
    sc = scalars(n, offset=1 << 22)
    want = tree_sum(lambda p, q: gpu_add(gpu_ctx, p, q), gpu_ctx.mul_var_base(pts, sc))
    assert (gpu_ctx.msm(pts, sc) == want).all()


def test_module_level_msm_returns_a_point(gpu_ctx, golden):
    import babyjubjub_rs_amd as bjj
    case = _golden()[3]
    P = [bjj.Point(*ints(p)) for p in case["points"]]
    q = bjj.msm(P, [ints(k) for k in case["scalars"]], ctx=gpu_ctx)
    assert (q.x, q.y) == ints(case["result"])
