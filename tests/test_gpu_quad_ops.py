"""The four-lane ("quad") point arithmetic of the short-call kernels on the device (csrc/k_small.hip: quad_dbl, quad_add,
quad_entry, quad_lift, quad_from_ref_affine, qtbl_build / qtbl_load, quad_walk, quad_walk_joint, quad_affine, quad_is_identity,
qfb_load, quad_mul_fixed_base, quad_add_fixed_base): the layer under tests/test_gpu_small_calls.py, which reaches it through the
C ABI alone -- canonical affine inputs, Z = 1, canonical bytes or a verdict out.

tests/devfuzz/quad.hip includes the kernel unit as it ships and hands raw limbs to those functions, the lanes 4k .. 4k + 3 of a
wave on item k as in the kernels, the tables in LDS.  The directed sets of tests/quad_ref.py -- every edge point in every
representative and edge Z, P + (-P), P + P, P + O, the torsion pairs through every table slot and both signs, the lazily negated
zero, the carry-chain scalars, waves of mixed window counts -- and 2^14 seeded random items per op are checked against plain
integers: value for value where the op is one formula (dbl, dbl4, add, entry, lift, from_ref, table, fb_load), as a projective
point with T Z == X Y and the N-form bound below 2r where it is a ladder (walk, walk_joint, fb_mul, fb_add), canonical words for
affine, the verdict for is_identity.  Where a one-item-per-lane function of csrc/curve.hpp / csrc/bjj_device.hpp does the same
field operations in the same order (quad_ref.LANE_OP), the same records run through libbjj_curve_test.so as well and the two
results are compared limb for limb; so are the `walk` items of 64 windows and vb_build_table + vb_mul_windowed.  There is no CPU build of this layer (DPP, wave shuffles); the model and the sets are judged
in tests/test_quad_ops_host.py.  Needs a real MI355X: `pytest -m gpu`."""
import ctypes
import os
import random
import subprocess
import time

import numpy as np
import pytest

import curve_ref as cr
import quad_ref as qr
from conftest import ROOT
from test_gpu_curve_ops import CurveHarness

pytestmark = pytest.mark.gpu

N_RANDOM = 1 << 14                 # seeded random items per op
GUARD = 64
FILL = 0xEEEEEEEE


class QuadHarness:
    """ctypes view of tests/devfuzz/libbjj_quad_test.so"""

    def __init__(self):
        d = os.path.join(ROOT, "tests", "devfuzz")
        name = "libbjj_quad_test.so"
        # always through make: it knows the product sources the harness includes, so an edit of csrc/ never runs a stale library
        r = subprocess.run(["make", "-s", name], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        import torch  # (loads the HIP runtime first, see babyjubjub-rs_amd/_lib.py)
        self.lib = ctypes.CDLL(os.path.join(d, name))
        vp = ctypes.c_void_p
        self.lib.qd_run.argtypes = [ctypes.c_int, vp, vp, vp, vp, ctypes.c_size_t, vp]
        self.lib.qd_words.argtypes = [ctypes.c_int, ctypes.c_int]
        self.lib.qd_fb_build.argtypes = [vp, vp]
        for op, code in qr.OPS.items():
            assert tuple(self.lib.qd_words(code, k) for k in range(3)) == qr.WIDTHS[op], op
        assert self.lib.qd_fb_window_bits() == qr.FB_W and self.lib.qd_fb_words() == (qr.FB_SLOTS + qr.FB_NWIN) * 32
        nw = self.lib.qd_fb_words()
        self.fb = torch.full((nw + GUARD,), FILL - (1 << 32), dtype=torch.int32, device="cuda")
        assert self.lib.qd_fb_build(self.fb.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert (self.fb[nw:].cpu().numpy().view(np.uint32) == FILL).all()

    def run(self, op, a, b):
        """the op on the device: a, b uint32 records (numpy) -> (n, out words) uint32.  Workgroups hold 16 items: more than one
        runs, the last partly filled; the guard words behind the last record stay as they were"""
        import torch
        n = a.shape[0]
        wa, wb, wo = qr.WIDTHS[op]
        assert n > 16 and n % 16 != 0
        assert a.shape == (n, wa) and ((b is None and wb == 0) or (b is not None and b.shape == (n, wb)))
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32).reshape(-1)).cuda()  # noqa: E731
        d_a = dev(a)
        d_b = dev(b) if b is not None else None
        d_o = torch.full((n * wo + GUARD,), FILL - (1 << 32), dtype=torch.int32, device="cuda")
        rc = self.lib.qd_run(qr.OPS[op], d_a.data_ptr(), d_b.data_ptr() if d_b is not None else None, d_o.data_ptr(), self.fb.data_ptr(), n, None)
        assert rc == 0
        torch.cuda.synchronize()
        o = d_o.cpu().numpy().view(np.uint32)
        assert (o[n * wo:] == FILL).all()                  # nothing written past the last record: the tail quads store nothing
        return o[:n * wo].reshape(n, wo)


@pytest.fixture(scope="module")
def quad():
    return QuadHarness()


@pytest.fixture(scope="module")
def lane():
    return CurveHarness(0)


def _run_and_check(quad, lane, op, items):
    items = qr.padded(items)
    a, b = qr.records(op, items)
    got = quad.run(op, a, b)
    bad = qr.check(op, items, got)
    assert bad == [], (op, len(bad), [(items[i], why) for i, why in bad[:3]])
    if op in qr.LANE_OP:                                   # the second opinion: the lane function, limb for limb
        la, lb = qr.lane_records(op, items)
        want = lane.run(qr.LANE_OP[op], la, lb)
        if op == "table":
            want = qr.table_from_lane(want)
        diff = np.nonzero((got != want).any(axis=1))[0]
        assert diff.size == 0, (op, "quad != lane function", diff.size, [(items[i], got[i].tolist(), want[i].tolist()) for i in diff[:2]])
    if op == "walk":
        # 64 windows are vb_build_table + vb_mul_windowed(nwin = 64, final_t) of the lane code, operation for operation: limb for limb
        idx = np.nonzero(b[:, 8] == 64)[0]
        idx = idx[:-1] if idx.size % 64 == 0 else idx
        want = lane.run("mulw64_t", a[idx], b[idx, :8])
        diff = np.nonzero((got[idx, :36] != want).any(axis=1))[0]
        assert idx.size > 64 and diff.size == 0, (op, "quad != vb_mul_windowed", diff.size, [items[idx[i]] for i in diff[:2]])
    return items, got


@pytest.mark.parametrize("op", list(qr.OPS))
def test_quad_op_edges_and_random(quad, lane, op):
    t0 = time.time()
    edges = qr.edge_set(op)
    _run_and_check(quad, lane, op, edges)
    items = qr.random_set(op, random.Random(0x40AD000 + qr.OPS[op]), N_RANDOM)
    _run_and_check(quad, lane, op, items)
    print("[quad fuzz] %-12s edges %5d  random %6d  %5.1f s" % (op, len(edges), len(items), time.time() - t0))


def test_fixed_base_table_is_the_model(quad):
    """the table the fb ops read, as the product's fixed_table_entry / fixed_table_chain built it on the device: every slot is the
    canonical Niels form of k 2^(8 j) B8, window 0 in the T form"""
    tab = quad.fb[:qr.FB_SLOTS * 32].cpu().numpy().view(np.uint32).reshape(qr.FB_SLOTS, 32)
    assert (tab[:, 27:] == 0).all()
    for s in range(qr.FB_SLOTS):
        want = sum((cr.nform(v) for v in qr.fb_entry(s)), ())
        assert tuple(int(v) for v in tab[s, :27]) == want, s


@pytest.mark.parametrize("op", ["walk", "walk_joint"])
def test_window_count_is_the_wave_maximum(quad, lane, op):
    """workgroups of 16 items whose pairs need different window counts: one item at 250 bits beside items at 1 to 131 bits, a wave
    of one-window items alone, a partly filled last wave.  The jw every lane reports is the largest need of its wave, and every
    item's result is its own u P1 (+ v P2), whatever its neighbours needed: the items shorter than jw lift the identity entry and
    double it"""
    rnd = random.Random(0x3A7E + qr.OPS[op])
    pl = cr.pool()
    waves = [[250] + [1, 2, 3, 126, 127, 130, 131] * 2 + [5],
             [1, 2, 1, 2] * 4,                             # jw = 1: the lifted top window is the result
             [3] + [1, 2] * 7 + [3],
             [131, 130, 127, 126] * 4,
             [2] * 15 + [250],
             [127, 1, 250, 3, 2]]                          # the partly filled last wave
    items, want_jw = [], []
    for wave in waves:
        for bits in wave:
            p, q = pl[rnd.randrange(len(pl))], pl[rnd.randrange(len(pl))]
            u, v = qr._bits_scalar(rnd, bits), qr._bits_scalar(rnd, rnd.randint(1, bits))
            if op == "walk":
                items.append((cr._rand_ext(rnd, p), cr.words(u) + (qr.need_of(bits),)))
            else:
                items.append((cr._rand_ext(rnd, p) + cr._rand_ext(rnd, q), cr.words(u) + cr.words(v) + (qr.need_of(bits),)))
            want_jw.append(max(qr.need_of(x) for x in wave))
    assert len(items) % 16 == 5 and all(qr.in_domain(op, it) for it in items)
    assert set(want_jw) == {63, 1, 2, 34} and qr.wave_jw(items) == want_jw
    a, b = qr.records(op, items)
    got = quad.run(op, a, b)
    assert (got[:, 36:40] == np.array(want_jw, dtype=np.uint32)[:, None]).all()
    assert qr.check(op, items, got) == []
    # the same items, each among neighbours that all need 64 windows: the same points
    wide = [(it[0], it[1][:-1] + (64,)) for it in items]
    a, b = qr.records(op, wide)
    got64 = quad.run(op, a, b)
    assert (got64[:, 36:40] == 64).all() and qr.check(op, wide, got64) == []
    O, W = cr._Rows(got, 4), cr._Rows(got64, 4)
    assert all(cr.peq(O.plain(i)[:3], W.plain(i)[:3]) for i in range(len(items)))
