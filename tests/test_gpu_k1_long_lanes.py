"""K1's overlap form with ONE workgroup slot per CU and launch (csrc/bjj_hip.hip: fixed_base_lanes, BJJ_K1_OVERLAP_SLOTS): the grid
is compute_units x 256 lanes, a lane keeps its slot for all of its items -- 16 of them at 2^20 items on 256 CUs -- and runs one
ramp, one running product and one block_invert where the two-slot grid runs two of each.  The kernel is the same
bjj_k_mul_fixed_base_2x256; what can go wrong is the item bookkeeping of long lanes: lanes of one grid that hold unequal item
counts, a last round that fills part of a wave / a group of block_invert / a workgroup, and grids that shrink below one
workgroup per CU.  Every size runs as affine and as compressed output, on both scratch sets at once (two streams), and is compared
byte for byte with the alone form (BJJ_K1_VARIANT=0) on the same inputs, which in turn is compared with the oracle on a strided
sample.  W = 16: the 67 MB table; the table width does not touch the grid.
Needs a real MI355X: run with `pytest -m gpu`."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROUNDS = [1, 2, 3]                                   # full rounds of the one-slot grid ...
REST = [0, 1, 63, 64, 255, 256, 65535]               # ... plus this many items (65 535 = lanes - 1 on a 256-CU part)
SHRUNK = [1, 255, 256, 257]                          # fewer items than lanes: the grid shrinks to ceil(n / 256) workgroups
CASES = [("%dx+%d" % (m, r), m, r) for m in ROUNDS for r in REST] + [(str(n), 0, n) for n in SHRUNK]


def _specials():
    from babyjubjub_rs_amd.api import SUBORDER as l
    return [0, 1, l - 1, l, (1 << 256) - 1]


def _scalars(n, offset):
    """uniform 254-bit scalars with 0, 1, l - 1, l, 2^256 - 1 at the start, at the end and every 61 items (the identity, Z = 1
    of a table entry and unreduced scalars inside the lanes' running products)"""
    from babyjubjub_rs_amd import workload as w
    sc = np.ascontiguousarray(w.scalars_254(n, offset=offset)).reshape(n, 32).copy()
    sp = np.stack([np.frombuffer(int(v).to_bytes(32, "little"), np.uint8) for v in _specials()])
    for k in range(min(n, len(sp))):
        sc[k] = sp[k]
        if n - 1 - k >= len(sp):
            sc[n - 1 - k] = sp[(k + 2) % len(sp)]
    idx = np.arange(7, n, 61)
    sc[idx] = sp[(idx // 61) % len(sp)]
    return sc


def _context(env):
    """a W = 16 context created under the given BJJ_* knobs (bjj_init reads them)"""
    import babyjubjub_rs_amd as bjj
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return bjj.Context(0, 16)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class _Rig:
    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.alone = _context({"BJJ_K1_VARIANT": "0"})
        self.long = _context({"BJJ_K1_VARIANT": "1", "BJJ_K1_OVERLAP_SLOTS": "1"})
        self.lanes = self.long.info().compute_units * 256
        self.streams = [torch.cuda.Stream(device=self.dev), torch.cuda.Stream(device=self.dev)]

    def close(self):
        self.alone.close()
        self.long.close()

    def run_alone(self, d_sc, n, compressed):
        torch, ctx = self.torch, self.alone
        d_out = torch.zeros(n * (32 if compressed else 64), dtype=torch.uint8, device=self.dev)
        (ctx.mul_fixed_base_compressed_dev if compressed else ctx.mul_fixed_base_dev)(d_sc.data_ptr(), n, d_out.data_ptr(), 0)
        i = ctx.info()
        ctx.sync()
        assert (i.last_fixed_base_shape, i.last_fixed_base_slots) == (0, 0)
        return d_out.cpu().numpy().reshape(n, -1)

    def run_long(self, d_sc, n, compressed):
        """the same batch on two streams at once: one launch per scratch set, neither waits for the other"""
        torch, ctx = self.torch, self.long
        outs = [torch.zeros(n * (32 if compressed else 64), dtype=torch.uint8, device=self.dev) for _ in self.streams]
        call = ctx.mul_fixed_base_compressed_dev if compressed else ctx.mul_fixed_base_dev
        ctx.sync()
        for st, o in zip(self.streams, outs):
            call(d_sc.data_ptr(), n, o.data_ptr(), st.cuda_stream)
            i = ctx.info()
            assert (i.last_fixed_base_shape, i.last_fixed_base_slots) == (1, 1)
        ctx.sync()
        return [o.cpu().numpy().reshape(n, -1) for o in outs]


@pytest.fixture(scope="module")
def rig():
    r = _Rig()
    yield r
    r.close()


def _sample(n):
    if n <= 512:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(64), np.arange(n - 64, n), np.arange(0, n, max(1, n // 256))]))


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_one_slot_grid_equals_the_alone_form(rig, oracle, case):
    _, m, r = CASES[case]
    n = m * rig.lanes + r
    sc = _scalars(n, offset=3000 * (case + 1))
    d_sc = rig.torch.from_numpy(sc.reshape(-1)).to(rig.dev)
    idx = _sample(n)
    want = rig.run_alone(d_sc, n, compressed=False)
    bad = np.nonzero((want[idx] != oracle.mul_fixed_base(sc[idx])).any(axis=1))[0]
    assert bad.size == 0, "n = %d, alone form: %d of %d sampled items differ from the oracle, first at item %d" % (n, bad.size, idx.size, idx[bad[0]])
    if n >= 4:      # scalars 0 and l give the identity (0, 1)
        ident = np.zeros(64, np.uint8)
        ident[32] = 1
        assert (want[0] == ident).all() and (want[3] == ident).all()
    for compressed in (False, True):
        if compressed:
            want = rig.run_alone(d_sc, n, compressed=True)
            assert (want[idx] == oracle.compress(oracle.mul_fixed_base(sc[idx]))).all()
        for k, got in enumerate(rig.run_long(d_sc, n, compressed)):
            assert got.shape == want.shape
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, "n = %d, %s, scratch set %d: %d items differ from the alone form, first at item %d" % (
                n, "compressed" if compressed else "affine", k, bad.size, bad[0])


def _ping_pong(ctx, torch, dev, n, launches, sync_each):
    from babyjubjub_rs_amd import workload as w
    d_sc = torch.from_numpy(np.ascontiguousarray(w.scalars_254(n, offset=91)).reshape(-1)).to(dev)
    outs = [torch.empty(n * 64, dtype=torch.uint8, device=dev) for _ in range(2)]
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    seen = []
    ctx.sync()
    for k in range(launches):
        ctx.mul_fixed_base_dev(d_sc.data_ptr(), n, outs[k & 1].data_ptr(), streams[k & 1].cuda_stream)
        i = ctx.info()
        seen.append((i.last_fixed_base_shape, i.last_fixed_base_slots))
        if sync_each:
            ctx.sync()
    ctx.sync()
    return seen


@pytest.mark.parametrize("knob", [None, "1", "2"], ids=["default", "one_slot_forced", "two_slots_forced"])
def test_info_reports_the_grid_of_the_overlap_form(knob):
    """bjj_info.last_fixed_base_slots next to last_fixed_base_shape: alternating streams without a synchronisation get the
    two-workgroup shape on the context's grid for overlapping launches; a caller that synchronises after every launch gets the
    alone form from its second launch on, whatever the knob says; the knob forces either grid"""
    import torch
    dev = torch.device("cuda", 0)
    ctx = _context({} if knob is None else {"BJJ_K1_OVERLAP_SLOTS": knob})
    try:
        n = (1 << 18) + 1      # above the short-call kernel's reach (2^15 items)
        slots = DEFAULT_SLOTS if knob is None else int(knob)
        seen = _ping_pong(ctx, torch, dev, n, 8, sync_each=False)
        assert seen[1:] == [(1, slots)] * 7, seen
        seen = _ping_pong(ctx, torch, dev, n, 6, sync_each=True)
        assert seen[1:] == [(0, 0)] * 5, seen
        # the short-call kernel takes no workgroup slot of K1
        _ping_pong(ctx, torch, dev, 256, 1, sync_each=True)
        i = ctx.info()
        assert (i.last_fixed_base_shape, i.last_fixed_base_slots) == (2, 0)
    finally:
        ctx.close()


DEFAULT_SLOTS = 1      # what bjj_init picks without the knob (bjj_hip.hip: BJJ_K1_OVERLAP_SLOTS_DEFAULT)
