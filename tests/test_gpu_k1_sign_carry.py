"""K1's overlap form (bjj_k_mul_fixed_base_2x256[_c32], csrc/k_fixed.hip) with the glue of BJJ_K1_SIGN_CARRY, BJJ_K1_REG_RECORDS,
BJJ_K1_ADDR_MAD, BJJ_K1_UNIFORM_STAGE and BJJ_K1_ALIGN_DIGITS: the accumulator carries the sign of the current digit and takes
every table entry as stored (the negation is a select inside the addition before), phase 2 unpacks its records and packs its
results in registers, a gather address is one multiply-add on two per-lane bases, the staging area is addressed from a scalar
wave index, and the digit stream moves by funnel shifts.

Same rig as tests/test_gpu_k1_item_boundary.py: the launch under test follows, without a synchronisation, a launch on the other
stream (bjj_info.last_fixed_base_shape must say 1), as affine and as compressed output; every output byte is compared with the
oracle and with the 512-lane form on one stream (code this change does not touch).  Small tables, W = 4, 8, 16 (63, 32 and
16 windows: both staging-area parities, and with W = 4 the longest run of sign decisions per item).  All cases are prefixes
of ONE scalar array dealt from the directed scalars and 2^14 random ones:
  * 0, 1, l - 1, l, l + 1, 2^254 - 1;
  * per width, digit strings that are all positive, all negative (below the top digit) and alternating either way; a zero
    digit in each window position in turn; every window all ones (the recoding carry runs to the top).
Call sizes: 1, 63, 64, 65, 255, 256, 257, then in units of the launch's lane count L (compute units x 256; 65 536 on an
MI355X) L + 1 -- one lane has two items -- and 2 L + 65: lanes with 2 and 3 items and a partly filled wave.
The sign of the LAST digit is always positive (a negative top digit would leave a carry behind the top window, which the
reduction excludes: tests/test_k1_weak_mod_l_host.py), so the kernel's last addition never flips; the two cases on the last
items of every lane are therefore the last sign CHANGE: the digit below the top one negative, and every digit positive.
Phase 2 reads its own stash: with the outputs preset to 0xFF and to 0x00 the results are the same bytes.
Needs a real MI355X: run with `pytest -m gpu`."""
import random

import numpy as np
import pytest

from test_gpu_k1_item_pipeline import _context, _le32, _same

pytestmark = pytest.mark.gpu

L_ORDER = 2736030358979909402780800718157159386076813972158567259200215660948447373041
WIDTHS = [4, 8, 16]
SMALL = [1, 63, 64, 65, 255, 256, 257]
RELATIVE = [(1, 1), (2, 65)]
CASES = [(str(n), 0, n) for n in SMALL] + [("%dL%+d" % (m, r), m, r) for m, r in RELATIVE]
RANDOM = 1 << 14
POOL = 61                                        # distinct scalars per kind of last item


def _nwin(W):
    return (252 + W - 1) // W


def _value(digits, W):
    v = sum(d << (W * j) for j, d in enumerate(digits))
    assert 0 <= v < L_ORDER                      # below l: the kernel's digits are those of the integer itself
    return v


def _signs(v, W):
    """the signs of the recoding's digits of v < l: +1, -1, 0"""
    half, carry, out = 1 << (W - 1), 0, []
    for j in range(_nwin(W)):
        u = ((v >> (W * j)) & ((1 << W) - 1)) + carry
        carry = 1 if u > half else 0
        out.append(0 if u in (0, 1 << W) else (-1 if carry else 1))   # 2^W: digit 0 behind a carry, "minus zero"
    assert carry == 0
    return out


def _directed():
    out = [0, 1, L_ORDER - 1, L_ORDER, L_ORDER + 1, (1 << 254) - 1]
    for W in WIDTHS:
        nw = _nwin(W)
        pos, neg = [3] * (nw - 1) + [1], [-3] * (nw - 1) + [1]
        alt0 = [3 if j % 2 == 0 else -3 for j in range(nw - 1)] + [1]
        alt1 = [-d for d in alt0[:-1]] + [1]
        for digits in (pos, neg, alt0, alt1):
            v = _value(digits, W)
            assert _signs(v, W) == [1 if d > 0 else -1 for d in digits]
            out.append(v)
        for p in range(nw):
            digits = list(alt1 if p % 2 else alt0)
            digits[p] = 0
            if p == nw - 1:
                digits[p - 1] = 3
            v = _value(digits, W)
            assert _signs(v, W)[p] == 0
            out.append(v)
        v = ((1 << (W * nw)) - 1) & ((1 << 250) - 1)
        s = _signs(v, W)
        assert s[0] == -1 and not any(s[1:-1]) and s[-1] == 1
        out.append(v)
    return out


def _last_items(W, below_top):
    """POOL scalars with random digits whose digit below the top one has the given sign (and, for +1, every digit positive)"""
    rnd = random.Random(0x5167 + W + below_top)
    half, nw, out = 1 << (W - 1), _nwin(W), []
    for _ in range(POOL):
        if below_top > 0:
            digits = [rnd.randrange(1, half) for _ in range(nw - 1)] + [1]
        else:
            digits = [rnd.randrange(-half + 1, half) for _ in range(nw - 2)] + [-rnd.randrange(1, half), 1]
        v = _value(digits, W)
        s = _signs(v, W)
        assert s[-1] == 1 and s[-2] == below_top and (below_top < 0 or all(x == 1 for x in s))
        out.append(v)
    return out


class _Rig:
    """the contexts, the streams, ONE scalar array for all cases and its oracle results"""

    def __init__(self, oracle):
        import torch
        from babyjubjub_rs_amd import workload as w
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.ctx = {W: _context(W, {"BJJ_FB_QUAD_MAX": "0"}) for W in WIDTHS}
        self.alone = {W: _context(W, {"BJJ_K1_VARIANT": "0"}) for W in WIDTHS}
        self.lanes = self.ctx[WIDTHS[0]].info().compute_units * 256
        self.sizes = {name: m * self.lanes + r for name, m, r in CASES}
        self.nmax = nmax = max(self.sizes.values())
        sp = np.stack([_le32(v) for v in _directed()])
        self.pools = {(W, sgn): np.stack([_le32(v) for v in _last_items(W, sgn)]) for W in WIDTHS for sgn in (1, -1)}
        unique = np.concatenate([sp, np.ascontiguousarray(w.scalars_254(RANDOM, offset=6161)).reshape(RANDOM, 32)]
                                + [self.pools[k] for k in sorted(self.pools)])
        self.pool_at = {}
        at = len(sp) + RANDOM
        for k in sorted(self.pools):
            self.pool_at[k] = at
            at += POOL
        step = 40507                                                  # a prime beyond the main part's size: every lane and round sees all kinds
        main = len(sp) + RANDOM
        idx = (np.arange(nmax, dtype=np.int64) * step) % main
        head = min(len(sp), nmax)
        idx[:head] = np.arange(head)
        for k, n in enumerate(sorted(self.sizes.values())):           # the last items of every case get directed scalars
            for t in range(min(n, 3)):
                idx[n - 1 - t] = (7 * k + t) % len(sp)
        self.idx = idx
        self.unique = unique
        self.want_unique = oracle.mul_fixed_base(unique)
        self.want32_unique = oracle.compress(self.want_unique)
        self.streams = [torch.cuda.Stream(device=self.dev), torch.cuda.Stream(device=self.dev)]
        self.filler = torch.empty(nmax * 64, dtype=torch.uint8, device=self.dev)
        self.d_sc = self.upload(idx)
        for ctx in self.ctx.values():                                 # grow both scratch sets now, not inside a case
            for st in self.streams:
                ctx.mul_fixed_base_dev(self.d_sc.data_ptr(), nmax, self.filler.data_ptr(), st.cuda_stream)
                ctx.sync()
                ctx.mul_fixed_base_compressed_dev(self.d_sc.data_ptr(), nmax, self.filler.data_ptr(), st.cuda_stream)
                ctx.sync()

    def upload(self, idx):
        return self.torch.from_numpy(np.ascontiguousarray(self.unique[idx]).reshape(-1)).to(self.dev)

    def want(self, idx, compressed):
        return (self.want32_unique if compressed else self.want_unique)[idx]

    def close(self):
        for c in list(self.ctx.values()) + list(self.alone.values()):
            c.close()

    def run_alone(self, W, d_sc, n, compressed):
        """the 512-lane form on one stream"""
        torch, ctx = self.torch, self.alone[W]
        d_out = torch.zeros(n * (32 if compressed else 64), dtype=torch.uint8, device=self.dev)
        (ctx.mul_fixed_base_compressed_dev if compressed else ctx.mul_fixed_base_dev)(d_sc.data_ptr(), n, d_out.data_ptr(), 0)
        shape = ctx.info().last_fixed_base_shape
        ctx.sync()
        assert shape == 0, shape
        return d_out.cpu().numpy().reshape(n, -1)

    def run_overlap(self, W, d_sc, n, compressed, preset=0):
        """the launch under test follows a launch of the largest case on the other stream, nothing synchronises in between"""
        torch, ctx = self.torch, self.ctx[W]
        call = ctx.mul_fixed_base_compressed_dev if compressed else ctx.mul_fixed_base_dev
        d_out = torch.full((n * (32 if compressed else 64),), preset, dtype=torch.uint8, device=self.dev)
        torch.cuda.synchronize(self.dev)
        ctx.sync()
        ctx.mul_fixed_base_dev(self.d_sc.data_ptr(), self.nmax, self.filler.data_ptr(), self.streams[0].cuda_stream)
        call(d_sc.data_ptr(), n, d_out.data_ptr(), self.streams[1].cuda_stream)
        shape = ctx.info().last_fixed_base_shape
        ctx.sync()
        assert shape == 1, "the launch under test did not get the overlap form (last_fixed_base_shape = %d)" % shape
        return d_out.cpu().numpy().reshape(n, -1)


@pytest.fixture(scope="module")
def rig(oracle):
    r = _Rig(oracle)
    yield r
    r.close()


PARAMS = [(W, name) for W in WIDTHS for name, _, _ in CASES]


@pytest.mark.parametrize("W,name", PARAMS, ids=["W%d-%s" % p for p in PARAMS])
def test_sign_carry_equals_oracle_and_alone_form(rig, W, name):
    n = rig.sizes[name]
    for compressed in (False, True):
        form = "compressed" if compressed else "affine"
        got = rig.run_overlap(W, rig.d_sc, n, compressed)
        _same(got, rig.want(rig.idx[:n], compressed), "W = %d, n = %d, %s, overlap form against the oracle" % (W, n, form))
        _same(got, rig.run_alone(W, rig.d_sc, n, compressed), "W = %d, n = %d, %s, overlap form against the 512-lane form" % (W, n, form))


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("below_top", [-1, 1], ids=["negative_below_top", "all_positive"])
def test_last_sign_change_on_every_lanes_last_item(rig, W, below_top):
    n = 2 * rig.lanes + 65                        # the last item of every lane is one of the last L items
    idx = rig.idx[:n].copy()
    idx[n - rig.lanes:] = rig.pool_at[(W, below_top)] + (np.arange(rig.lanes) * 7) % POOL
    d_sc = rig.upload(idx)
    for compressed in (False, True):
        got = rig.run_overlap(W, d_sc, n, compressed)
        _same(got, rig.want(idx, compressed), "W = %d, last items with sign %+d below the top digit, compressed = %s, against the oracle"
              % (W, below_top, compressed))
        _same(got, rig.run_alone(W, d_sc, n, compressed), "W = %d, the same against the 512-lane form" % W)


@pytest.mark.parametrize("W", WIDTHS)
def test_phase_two_reads_its_own_stash(rig, W):
    n = 2 * rig.lanes + 65
    for compressed in (False, True):
        ones = rig.run_overlap(W, rig.d_sc, n, compressed, preset=0xFF)
        zeros = rig.run_overlap(W, rig.d_sc, n, compressed, preset=0x00)
        _same(ones, zeros, "W = %d, compressed = %s: outputs preset to 0xFF against outputs preset to 0x00" % (W, compressed))
        _same(ones, rig.want(rig.idx[:n], compressed), "W = %d, compressed = %s, preset outputs, against the oracle" % (W, compressed))
