"""K1's epilogue on the GPU: the workgroup-wide inversion (csrc/k_common.hpp: block_invert with the division-step core
fr_inv_k1) and the backward walk of every lane's running inverse, in both shapes of the kernel (one 512-lane workgroup per CU;
two 256-lane workgroups, the shape overlapping launches get) and both output forms (64-byte affine points, 32-byte compressed
points), plus the constant-time signer form (the scanning kernel runs the same epilogue).  W = 16: the 67 MB table; the table
width does not touch the epilogue.  Batch sizes: partial waves, partial groups of block_invert, a workgroup whose inverting
wave holds idle lanes, and sizes at which the first lanes of the grid hold two or three items and the rest fewer.
Needs a real MI355X: run with `pytest -m gpu`."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LANES_PER_CU = 512      # both shapes keep 512 resident lanes per CU (2 waves per SIMD): 1 x 512 or 2 x 256
SMALL = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513]
N_BUSY = 1 << 19        # the launch that keeps the other stream busy while a launch of the two-workgroup shape is issued


def _specials():
    from babyjubjub_rs_amd.api import SUBORDER as l
    return [0, 1, l - 1, l, l + 1, (1 << 256) - 1]


def _scalars(n, offset):
    """uniform 254-bit scalars with 0, 1, l - 1, l, l + 1, 2^256 - 1 at the start, at the end and every 61 items: the identity
    appears as a result (Z of a lane's item repeats in its running product) next to ordinary points"""
    from babyjubjub_rs_amd import workload as w
    sc = np.ascontiguousarray(w.scalars_254(n, offset=offset)).reshape(n, 32).copy()
    sp = np.stack([np.frombuffer(int(v).to_bytes(32, "little"), np.uint8) for v in _specials()])
    for k in range(min(n, len(sp))):
        sc[k] = sp[k]
        if n - 1 - k >= len(sp):
            sc[n - 1 - k] = sp[(k + 3) % len(sp)]
    idx = np.arange(7, n, 61)
    sc[idx] = sp[(idx // 61) % len(sp)]
    return sc


class _Rig:
    def __init__(self):
        import torch
        import babyjubjub_rs_amd as bjj
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        # bjj_init reads the knob: no short-call kernel (four lanes per item up to 2^15 items), every size goes to K1
        saved = os.environ.get("BJJ_FB_QUAD_MAX")
        os.environ["BJJ_FB_QUAD_MAX"] = "0"
        try:
            self.ctx = bjj.Context(0, 16)
        finally:
            if saved is None:
                del os.environ["BJJ_FB_QUAD_MAX"]
            else:
                os.environ["BJJ_FB_QUAD_MAX"] = saved
        self.lanes = self.ctx.info().compute_units * LANES_PER_CU
        self.sa, self.sb = torch.cuda.Stream(device=self.dev), torch.cuda.Stream(device=self.dev)
        from babyjubjub_rs_amd import workload as w
        self.busy_sc = torch.from_numpy(np.ascontiguousarray(w.scalars_254(N_BUSY, offset=5)).reshape(-1)).to(self.dev)
        self.busy_out = torch.empty(N_BUSY * 64, dtype=torch.uint8, device=self.dev)

    def run(self, sc, shape, compressed):
        """one launch of the wanted shape on stream `sa`; returns the output bytes"""
        torch, ctx = self.torch, self.ctx
        n = sc.shape[0]
        d_sc = torch.from_numpy(np.ascontiguousarray(sc).reshape(-1)).to(self.dev)
        d_out = torch.zeros(n * (32 if compressed else 64), dtype=torch.uint8, device=self.dev)
        call = ctx.mul_fixed_base_compressed_dev if compressed else ctx.mul_fixed_base_dev
        ctx.sync()
        if shape == 1:      # alternate over two streams without synchronising: the other set is busy when `sa` launches
            ctx.mul_fixed_base_dev(self.busy_sc.data_ptr(), N_BUSY, self.busy_out.data_ptr(), self.sb.cuda_stream)
            call(d_sc.data_ptr(), n, d_out.data_ptr(), self.sa.cuda_stream)
        else:               # one stream: the first launch behind a call on another stream may still look like a ping-pong
            call(d_sc.data_ptr(), n, d_out.data_ptr(), self.sa.cuda_stream)
            call(d_sc.data_ptr(), n, d_out.data_ptr(), self.sa.cuda_stream)
        got_shape = ctx.info().last_fixed_base_shape
        ctx.sync()
        assert got_shape == shape, "wanted kernel shape %d, the host chose %d" % (shape, got_shape)
        return d_out.cpu().numpy().reshape(n, -1)


@pytest.fixture(scope="module")
def rig():
    r = _Rig()
    yield r
    r.ctx.close()


def _large_sizes(lanes):
    return [lanes + 1, 2 * lanes + 257, 3 * lanes - 1]


def _sample(n):
    if n <= 2048:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(600), np.arange(n - 600, n), np.arange(0, n, max(1, n // 2048))[:2048]]))


@pytest.fixture(scope="module")
def cases(rig, oracle):
    """per batch size: the scalars, the compared items and the oracle's points for them -- computed once, shared by both shapes"""
    out = {}
    for k, n in enumerate(SMALL + _large_sizes(rig.lanes)):
        sc = _scalars(n, offset=1000 * (k + 1))
        idx = _sample(n)
        out[k] = (sc, idx, oracle.mul_fixed_base(sc[idx]))
    return out


@pytest.mark.parametrize("shape", [0, 1], ids=["one_512_lane_workgroup", "two_256_lane_workgroups"])
@pytest.mark.parametrize("case", range(len(SMALL) + 3), ids=[str(n) for n in SMALL] + ["lanes+1", "2lanes+257", "3lanes-1"])
def test_affine_and_compressed_against_the_oracle(rig, oracle, cases, case, shape):
    sc, idx, want = cases[case]
    n = sc.shape[0]
    pts = rig.run(sc, shape, compressed=False)
    assert pts.shape == (n, 64)
    bad = np.nonzero((pts[idx] != want).any(axis=1))[0]
    assert bad.size == 0, "n = %d: %d of %d compared items differ, first at item %d" % (n, bad.size, idx.size, idx[bad[0]])
    c32 = rig.run(sc, shape, compressed=True)
    assert c32.shape == (n, 32)
    bad = np.nonzero((c32 != oracle.compress(pts)).any(axis=1))[0]     # every item
    assert bad.size == 0, "n = %d: %d compressed items differ from compress(affine), first at item %d" % (n, bad.size, bad[0])
    if n >= len(_specials()):      # scalars 0 and l give the identity (0, 1)
        ident = np.zeros(64, np.uint8)
        ident[32] = 1
        assert (pts[0] == ident).all() and (pts[3] == ident).all()


def test_constant_time_signer_form(rig, oracle):
    """bjj_set_signer_constant_time: public_keys through the scanning kernel, whose epilogue is K1's"""
    torch, ctx = rig.torch, rig.ctx
    from babyjubjub_rs_amd import workload as w
    n = 257
    keys = np.ascontiguousarray(w.scalars_254(n, offset=4242)).reshape(n, 32)
    d_keys = torch.from_numpy(keys.reshape(-1).copy()).to(rig.dev)
    d_out = torch.zeros(n * 64, dtype=torch.uint8, device=rig.dev)
    ctx.set_signer_constant_time(True)
    try:
        assert ctx.info().signer_constant_time == 1
        ctx.public_keys_dev(d_keys.data_ptr(), n, d_out.data_ptr(), 0)
        ctx.sync()
    finally:
        ctx.set_signer_constant_time(False)
    assert (d_out.cpu().numpy().reshape(n, 64) == oracle.public_keys(keys)).all()
