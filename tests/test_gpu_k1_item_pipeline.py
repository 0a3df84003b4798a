"""K1's overlap form (bjj_k_mul_fixed_base_2x256[_c32], csrc/k_fixed.hip) starts work ahead of need: the next item's scalar,
digit stream and first two gathers before the current item's last addition, the next phase-2 record before the current one's
multiplications, and the first phase-2 record before the workgroup inversion.  What can go wrong is state carried across an item
boundary: a digit stream or a carry of item k+1 that leaks into item k's last window, a gather issued for a lane that has no
next item (the loop is wave-uniform: such a lane clamps to the last item), a record loaded before its stores are visible, a
record finished twice or not at all in a ragged last round.

Every case runs on a context that picks the kernel form by itself: the launch follows, without a synchronisation, a launch on the
other stream (bjj_info.last_fixed_base_shape must say 1), as affine and as compressed output.  Every output byte is compared
with the oracle and with the same inputs through the 512-lane form on one stream.  All cases are prefixes of ONE scalar array,
dealt from 4093 distinct scalars, so the oracle runs once and on those only.  W = 12 (21 windows: the last gather of an item
lands in staging area 0) and W = 14 (18 windows: area 1).
Needs a real MI355X: run with `pytest -m gpu`."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIDTHS = [12, 14]
SMALL = [1, 37, 63, 64, 65, 255, 256, 257]      # partial waves, clamped lanes inside a live wave, lanes with no item in a wave that gathers
# sizes in units of the launch's lane count L (compute units x 256: one workgroup slot per CU) plus a rest
RELATIVE = [(1, -1), (1, 0), (1, 1), (2, 65), (3, 0)]
CASES = [(str(n), 0, n) for n in SMALL] + [("%dL%+d" % (m, r), m, r) for m, r in RELATIVE]
UNIQUE = 4093                                   # distinct scalars in the shared array (prime)
W14_CASES = ["65", "257", "1L+1", "2L+65"]     # the second staging-area parity: the shapes that clamp, wrap and end ragged


def _le32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


def _specials():
    """0, 1, l - 1, l, 2^256 - 1, and per table width scalars below 2^250 (< l: the digits are those of the integer itself) whose
    windows sit at the edge of the signed recoding: every window 2^(W-1) (the largest digit, no carry), window 0 = 2^(W-1) + 1
    and the rest 2^(W-1) (digit -(2^(W-1) - 1), then a carry into every following window), every window 2^W - 1 (digit -1, then
    digits 0 with the carry running to the top), and the two alternations of 2^(W-1) + 1 with 2^(W-1) - 1"""
    from babyjubjub_rs_amd.api import SUBORDER as l
    out = [0, 1, l - 1, l, (1 << 256) - 1]
    top = (1 << 250) - 1
    for W in WIDTHS + [28]:
        half, nw = 1 << (W - 1), 250 // W + 1
        rep = lambda f: sum(f(j) << (W * j) for j in range(nw)) & top
        new = [rep(lambda j: half), rep(lambda j: half + 1 if j == 0 else half), rep(lambda j: (1 << W) - 1),
               rep(lambda j: half + 1 if j & 1 else half - 1), rep(lambda j: half - 1 if j & 1 else half + 1)]
        assert all(0 < v < l for v in new)
        assert {(new[0] >> (W * j)) & (2 * half - 1) for j in range(250 // W)} == {half}
        out += new
    return np.stack([_le32(v) for v in out])


def _context(W, env):
    """a context created under the given BJJ_* knobs (bjj_init reads them)"""
    import babyjubjub_rs_amd as bjj
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return bjj.Context(0, W)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class _Rig:
    """the contexts, the streams, ONE scalar array for all cases and its oracle results"""

    def __init__(self, oracle):
        import torch
        import babyjubjub_rs_amd as bjj
        from babyjubjub_rs_amd import workload as w
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        # K1 for every size, no short-call kernel; `ctx` picks the kernel form by itself, `alone` is held to the 512-lane form
        self.ctx = {W: _context(W, {"BJJ_FB_QUAD_MAX": "0"}) for W in WIDTHS}
        self.alone = {W: _context(W, {"BJJ_K1_VARIANT": "0"}) for W in WIDTHS}
        self.lanes = self.ctx[WIDTHS[0]].info().compute_units * 256
        self.sizes = {name: m * self.lanes + r for name, m, r in CASES}
        nmax = max(self.sizes.values())
        # UNIQUE distinct scalars, the special ones among them, dealt over the array with a stride coprime to UNIQUE (a prime): every
        # lane and every round sees all kinds, and the oracle -- a function of the item alone -- runs on UNIQUE items only
        sp = _specials()
        base = np.ascontiguousarray(w.scalars_254(UNIQUE, offset=4242)).reshape(UNIQUE, 32).copy()
        base[:len(sp)] = sp
        idx = (np.arange(nmax, dtype=np.int64) * 40503) % UNIQUE
        idx[:len(sp)] = np.arange(len(sp))                    # the first lanes ...
        for k, n in enumerate(sorted(self.sizes.values())):   # ... and the last items of every case get special scalars
            for t in range(min(n, 3)):
                idx[n - 1 - t] = (5 * k + t) % len(sp)
        self.sc = np.ascontiguousarray(base[idx])
        self.d_sc = torch.from_numpy(self.sc.reshape(-1)).to(self.dev)
        want = oracle.mul_fixed_base(base)
        self.want = want[idx]
        self.want32 = oracle.compress(want)[idx]
        self.streams = [torch.cuda.Stream(device=self.dev), torch.cuda.Stream(device=self.dev)]
        self.filler = torch.empty(nmax * 64, dtype=torch.uint8, device=self.dev)
        # grow both scratch sets of every context to the largest case now: a set that grows inside a case waits for the device,
        # and the launch under test would find the other stream idle
        for ctx in self.ctx.values():
            for st in self.streams:
                ctx.mul_fixed_base_dev(self.d_sc.data_ptr(), nmax, self.filler.data_ptr(), st.cuda_stream)
                ctx.sync()
                ctx.mul_fixed_base_compressed_dev(self.d_sc.data_ptr(), nmax, self.filler.data_ptr(), st.cuda_stream)
                ctx.sync()

    def close(self):
        for c in list(self.ctx.values()) + list(self.alone.values()):
            c.close()

    def run_alone(self, W, n, compressed):
        """the 512-lane form on one stream"""
        torch, ctx = self.torch, self.alone[W]
        d_out = torch.zeros(n * (32 if compressed else 64), dtype=torch.uint8, device=self.dev)
        (ctx.mul_fixed_base_compressed_dev if compressed else ctx.mul_fixed_base_dev)(self.d_sc.data_ptr(), n, d_out.data_ptr(), 0)
        shape = ctx.info().last_fixed_base_shape
        ctx.sync()
        assert shape == 0, shape
        return d_out.cpu().numpy().reshape(n, -1)

    def run_overlap(self, W, n, compressed):
        """the launch under test follows a launch of the largest case on the other stream, nothing synchronises in between"""
        torch, ctx = self.torch, self.ctx[W]
        call = ctx.mul_fixed_base_compressed_dev if compressed else ctx.mul_fixed_base_dev
        d_out = torch.zeros(n * (32 if compressed else 64), dtype=torch.uint8, device=self.dev)
        torch.cuda.synchronize(self.dev)   # the fill runs on torch's stream, which the two streams below do not wait for
        ctx.sync()
        ctx.mul_fixed_base_dev(self.d_sc.data_ptr(), self.sc.shape[0], self.filler.data_ptr(), self.streams[0].cuda_stream)
        call(self.d_sc.data_ptr(), n, d_out.data_ptr(), self.streams[1].cuda_stream)
        shape = ctx.info().last_fixed_base_shape
        ctx.sync()
        assert shape == 1, "the launch under test did not get the overlap form (last_fixed_base_shape = %d)" % shape
        return d_out.cpu().numpy().reshape(n, -1)


@pytest.fixture(scope="module")
def rig(oracle):
    r = _Rig(oracle)
    yield r
    r.close()


def _same(got, want, what):
    assert got.shape == want.shape, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: %d of %d items differ, first at item %d (%d output rows are all zero)" % (
        what, bad.size, want.shape[0], bad[0], int((~got.any(axis=1)).sum()))


PARAMS = [(W, name) for W in WIDTHS for name, _, _ in CASES if W == WIDTHS[0] or name in W14_CASES]


@pytest.mark.parametrize("W,name", PARAMS, ids=["W%d-%s" % p for p in PARAMS])
def test_overlap_form_equals_oracle_and_alone_form(rig, W, name):
    n = rig.sizes[name]
    for compressed in (False, True):
        form = "compressed" if compressed else "affine"
        want = (rig.want32 if compressed else rig.want)[:n]
        got = rig.run_overlap(W, n, compressed)
        _same(got, want, "W = %d, n = %d, %s, overlap form against the oracle" % (W, n, form))
        _same(got, rig.run_alone(W, n, compressed), "W = %d, n = %d, %s, overlap form against the 512-lane form" % (W, n, form))

