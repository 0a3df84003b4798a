"""K1's overlap form (bjj_k_mul_fixed_base_2x256[_c32], csrc/k_fixed.hip) at the boundary between two items of a lane: the stash
stores of the item before and the load of the next scalar are issued behind the two waits that open an item (the stash waits in
registers meanwhile; a lane's last item is stored at once), the first addition takes its operands straight from the entries of
windows 0 and 1 (window 0's sign moves to window 1's t2d), the scalar is reduced without the last conditional subtraction
(scalar_mod_l_weak: the digit stream sees values up to 1.17 l), and a gather's slot numbers go through a wave-private LDS strip.

Same rig as tests/test_gpu_k1_item_pipeline.py: the launch under test follows, without a synchronisation, a launch on the other
stream (bjj_info.last_fixed_base_shape must say 1), as affine and as compressed output; every output byte is compared with the
oracle and with the 512-lane form on one stream; all cases are prefixes of ONE scalar array dealt from 4093 distinct scalars.
W = 12 and W = 14: for both nwin * W = 252, the same tight top window as W = 28, and the two staging-area parities.
The scalars add to that test's specials, all found with plain integers here:
  * per top byte, one scalar whose weak remainder lies in [l, 1.17 l) and one just below l (where the byte's range holds one);
  * scalars whose weak remainder has the largest top window the weak form can give, with and without a carry coming in;
  * window 0 and window 1 at digit 0 (the identity entry; also "minus zero": all ones plus a carry), +1, -1, +2^(W-1) and
    -(2^(W-1) - 1), the most negative digit of the recoding, in every combination.
Needs a real MI355X: run with `pytest -m gpu`."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_k1_item_pipeline import _context, _le32, _same, _specials

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_ORDER = 2736030358979909402780800718157159386076813972158567259200215660948447373041
WIDTHS = [12, 14]
SMALL = [1, 63, 64, 65, 255, 256, 257]
# sizes in units of the launch's lane count L (compute units x 256) plus a rest.  L - 1, L, L + 1: a lane's only item is also its
# last, so its stash is stored at once; beyond L the stash of every item but the last waits in registers
RELATIVE = [(1, -1), (1, 0), (1, 1), (2, 65), (3, 0)]
CASES = [(str(n), 0, n) for n in SMALL] + [("%dL%+d" % (m, r), m, r) for m, r in RELATIVE]
UNIQUE = 4093
CHILD = "BJJ_K1_BOUNDARY_CHILD"     # set in the child run of the variant-build cases below


def _quotient(v):
    return ((v >> 248) * 10834) >> 16


def _weak(v):
    """scalar_mod_l_weak in plain integers"""
    return v - _quotient(v) * L_ORDER


def _weak_range_scalars():
    """per top byte: a scalar whose weak remainder is in [l, 1.17 l) and one whose remainder is just below l"""
    rnd = random.Random(0x1B0D)
    out, above, below = [], 0, 0
    for t in range(256):
        lo, hi, q = t << 248, (t + 1) << 248, (t * 10834) >> 16
        v = max(lo, (q + 1) * L_ORDER) + rnd.getrandbits(200)
        if v < hi:
            assert L_ORDER <= _weak(v) and 100 * _weak(v) < 117 * L_ORDER
            out.append(v)
            above += 1
        v = min(hi - 1, (q + 1) * L_ORDER - 1) - rnd.getrandbits(16)
        if v >= lo:
            assert 0 <= _weak(v) < L_ORDER
            out.append(v)
            below += 1
    # each multiple l .. 42 l lies in the range of one top byte, and every byte's range starts below (q + 1) l
    assert above >= 40 and below >= 250, (above, below)
    return out


def _top_window_scalars():
    """per width: weak remainders whose top window is the largest the weak form can give, the window below it all ones (a carry
    comes in) and zero (none)"""
    out = []
    for W in WIDTHS + [28]:
        sh = 252 - W
        dmax = max((((t + 1) << 248) - 1 - ((t * 10834) >> 16) * L_ORDER) >> sh for t in range(256))
        assert dmax + 1 <= 1 << (W - 1)
        for below in ((1 << W) - 1, 0):
            found = []
            for d in (dmax, dmax - 1):     # the largest remainder need not have the window below it all ones: then one less, plus the carry
                s = (d << sh) | (below << (sh - W)) | 0x5A5A5
                found += [s + q * L_ORDER for q in range(43) if s + q * L_ORDER < 1 << 256 and _quotient(s + q * L_ORDER) == q]
            assert found, (W, below)
            assert (_weak(found[0]) >> sh) + (1 if below else 0) >= dmax
            out.append(found[0])
    return out


def _low_window_scalars():
    """windows 0 and 1 at the digits 0, +1, +2^(W-1), -(2^(W-1) - 1), -1 (and, behind a carry, "minus zero")"""
    rnd = random.Random(0xD161)
    out = []
    for W in WIDTHS + [28]:
        half, mask = 1 << (W - 1), (1 << W) - 1
        for w0 in (0, 1, half, half + 1, mask):
            for w1 in (0, 1, half, half + 1, mask):
                out.append((rnd.getrandbits(190) << (2 * W)) | (w1 << W) | w0)
    assert all(v < L_ORDER for v in out)
    return out


def _all_specials():
    extra = _weak_range_scalars() + _top_window_scalars() + _low_window_scalars()
    return np.concatenate([_specials(), np.stack([_le32(v) for v in extra])])


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
        nmax = max(self.sizes.values())
        sp = _all_specials()
        assert len(sp) < UNIQUE // 2
        base = np.ascontiguousarray(w.scalars_254(UNIQUE, offset=5151)).reshape(UNIQUE, 32).copy()
        base[:len(sp)] = sp
        idx = (np.arange(nmax, dtype=np.int64) * 40503) % UNIQUE      # coprime to UNIQUE: every lane and round sees all kinds
        head = min(len(sp), nmax)
        idx[:head] = np.arange(head)
        for k, n in enumerate(sorted(self.sizes.values())):           # the last items of every case get special scalars
            for t in range(min(n, 3)):
                idx[n - 1 - t] = (7 * k + t) % len(sp)
        self.sc = np.ascontiguousarray(base[idx])
        self.d_sc = torch.from_numpy(self.sc.reshape(-1)).to(self.dev)
        want = oracle.mul_fixed_base(base)
        self.want = want[idx]
        self.want32 = oracle.compress(want)[idx]
        self.streams = [torch.cuda.Stream(device=self.dev), torch.cuda.Stream(device=self.dev)]
        self.filler = torch.empty(nmax * 64, dtype=torch.uint8, device=self.dev)
        for ctx in self.ctx.values():                                 # grow both scratch sets now, not inside a case
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
        torch.cuda.synchronize(self.dev)
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


PARAMS = [(W, name) for W in WIDTHS for name, _, _ in CASES]


@pytest.mark.parametrize("W,name", PARAMS, ids=["W%d-%s" % p for p in PARAMS])
def test_item_boundary_equals_oracle_and_alone_form(rig, W, name):
    n = rig.sizes[name]
    for compressed in (False, True):
        form = "compressed" if compressed else "affine"
        want = (rig.want32 if compressed else rig.want)[:n]
        got = rig.run_overlap(W, n, compressed)
        _same(got, want, "W = %d, n = %d, %s, overlap form against the oracle" % (W, n, form))
        _same(got, rig.run_alone(W, n, compressed), "W = %d, n = %d, %s, overlap form against the 512-lane form" % (W, n, form))


# The developer's A/B builds with the other record schedules (tools/ab_k1_item_pipeline.sh: BJJ_K1_EARLY_RECORD=1, whose wait before
# the first record load must still cover the deferred stores, and BJJ_K1_PIPE_RECORD=1) are not part of a checkout: where one is
# on the machine, the ragged two-round case runs against it in a child process (the library is chosen at import).
VARIANTS = [("early_record", "tools/ab_early.so"), ("pipe_record", "tools/ab_record.so")]


@pytest.mark.parametrize("label,lib", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_item_boundary_with_variant_build(label, lib):
    if os.environ.get(CHILD):
        pytest.skip("inside the child run of a variant build")
    path = os.path.join(ROOT, lib)
    if not os.path.exists(path):
        pytest.skip("no %s on this machine (a developer's A/B build of csrc with the %s schedule)" % (lib, label))
    env = dict(os.environ, BJJ_LIB_PATH=path)
    env[CHILD] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "W12-2L+65 or W14-2L+65"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    assert r.returncode == 0, r.stdout[-3000:]
