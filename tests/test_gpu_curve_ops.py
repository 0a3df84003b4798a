"""The group law and the per-lane table, ladder and fixed-table code on the device (csrc/curve.hpp; csrc/bjj_device.hpp:
niels_cneg_lazy, vb_build_table .. vb_mul_windowed, ref_mul_scalar, fixed_table_entry / _chain / _check_slot, var_base_item): the
layer between the field tests (tests/test_gpu_field_ops.py, tests/test_gpu_devfuzz.py) and the byte-for-byte ABI parity tests.

(1) tests/devfuzz/curve.hip runs the functions that ship, one item per lane, on the directed sets of tests/curve_ref.py -- the
exceptional pairs P + (-P), P + P, P + O, the torsion points, the extreme representatives 0, 1, r - 1, 2r - 1, the carry-less
negated entries, the ladder scalars whose recoding carries through every window -- plus 2^14 seeded random items per op, in
both device libraries (raw and packed per-lane tables).  The results are compared bit for bit with the g++ build of the same
dispatcher (tests/emul/emul_curve_ops.cpp: this is what proves the assembler multiplier and hipcc's code on these inputs) and
checked against plain integers.
(2) The same edge points through the C ABI, against the C oracle: bjj_point_add, bjj_proj_add + bjj_proj_affine on operands
scaled by z = 1, r - 1 and one seeded z (the ABI takes plain values: there is no representative to choose), the operands whose
sum has a vanishing denominator, bjj_mul_var_base on every edge point times every edge scalar: one call of the items tiled past
2^14, which runs the variable-base kernel K2 of k_var.hip (vb_build_table + vb_mul_windowed on packed tables;
last_var_base_form 0 or 1), one call of the items as they are and one-item calls, which run the four-lane short-call
kernel of k_small.hip (form 2).  No single point doubles into a vanishing
denominator (tests/test_curve_ops_host.py::test_no_point_doubles_into_a_vanishing_denominator shows why), so that case keeps to
the pair form.
The short-call kernel's own group law, table and ladder -- the four-lane functions of k_small.hip, which part (2) reaches with
canonical affine inputs only -- are driven on raw limbs, with these sets, by tests/test_gpu_quad_ops.py (tests/devfuzz/quad.hip,
tests/quad_ref.py), and compared limb for limb with the lane functions of part (1).  Needs a real MI355X: `pytest -m gpu`."""
import ctypes
import os
import random
import subprocess
import time

import numpy as np
import pytest

import curve_ref as cr
from conftest import ROOT, pack, unpack
from test_curve_ops_host import LAYOUT_OPS, clibs  # noqa: F401  (the fixture that builds the CPU libraries of the same dispatcher)

pytestmark = pytest.mark.gpu

R_MOD = cr.R_MOD
N_RANDOM = 1 << 14                 # seeded random items per op
GUARD = 64


class CurveHarness:
    """ctypes view of tests/devfuzz/libbjj_curve_test.so (layout 0) or libbjj_curve_test_packed.so (layout 1)"""

    def __init__(self, layout):
        d = os.path.join(ROOT, "tests", "devfuzz")
        name = "libbjj_curve_test%s.so" % ("_packed" if layout else "")
        # always through make: it knows the product headers the harness includes, so an edit of csrc/ never runs a stale library
        r = subprocess.run(["make", "-s", name], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        import torch  # noqa: F401  (loads the HIP runtime first, see babyjubjub-rs_amd/_lib.py)
        self.lib = ctypes.CDLL(os.path.join(d, name))
        vp = ctypes.c_void_p
        self.lib.co_run.argtypes = [ctypes.c_int, vp, vp, vp, vp, ctypes.c_size_t, vp]
        self.lib.co_words.argtypes = [ctypes.c_int, ctypes.c_int]
        assert self.lib.co_layout() == layout
        for op, code in cr.OPS.items():
            assert tuple(self.lib.co_words(code, k) for k in range(4)) == cr.WIDTHS[op], op

    def run(self, op, a, b):
        """the op on the device: a, b uint32 records (numpy) -> (n, out words) uint32 (numpy).  Workgroups are one wave wide, so
        more than 64 items run a grid of more than one workgroup; the item count is no multiple of 64."""
        import torch
        n = a.shape[0]
        wa, wb, wo, ws = cr.WIDTHS[op]
        assert n > 64 and n % 64 != 0
        assert a.shape == (n, wa) and ((b is None and wb == 0) or (b is not None and b.shape == (n, wb)))
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32).reshape(-1)).cuda()  # noqa: E731
        d_a = dev(a)
        d_b = dev(b) if b is not None else None
        fill = -0x11111112                                                    # 0xEEEEEEEE
        d_o = torch.full((n * wo + GUARD,), fill, dtype=torch.int32, device="cuda")
        d_s = torch.full((n * ws + GUARD,), fill, dtype=torch.int32, device="cuda") if ws else None
        rc = self.lib.co_run(cr.OPS[op], d_a.data_ptr(), d_b.data_ptr() if d_b is not None else None, d_o.data_ptr(),
                             d_s.data_ptr() if d_s is not None else None, n, None)
        assert rc == 0
        torch.cuda.synchronize()
        o = d_o.cpu().numpy().view(np.uint32)
        assert (o[n * wo:] == 0xEEEEEEEE).all()            # nothing written past the last record
        if d_s is not None:
            assert (d_s[n * ws:].cpu().numpy().view(np.uint32) == 0xEEEEEEEE).all()      # nor past the last item's scratch
        return o[:n * wo].reshape(n, wo)


@pytest.fixture(scope="module")
def harnesses():
    return [CurveHarness(0), CurveHarness(1)]


def _padded(items):
    """the items, with the first ones repeated until there are more than 64 and no multiple of 64"""
    out = list(items)
    k = 0
    while len(out) <= 64 or len(out) % 64 == 0:
        out.append(items[k % len(items)])
        k += 1
    return out


def _run_and_check(harnesses, clibs, op, items):  # noqa: F811
    items = _padded(items)
    a, b = cr.records(op, items)
    checked = None
    for layout in (0, 1):
        got = harnesses[layout].run(op, a, b)
        want = cr.cpu_run(clibs[layout if op in LAYOUT_OPS else 0], op, a, b)
        diff = np.nonzero((got != want).any(axis=1))[0]
        assert diff.size == 0, (op, layout, "device != CPU harness", diff.size, [(items[i], got[i].tolist(), want[i].tolist()) for i in diff[:3]])
        if checked is None or (got != checked).any():      # the same bits were judged already
            bad = cr.check(op, items, got, layout=layout)
            assert bad == [], (op, layout, len(bad), [(items[i], why) for i, why in bad[:3]])
            checked = got
    return got


# ---- (1) the group-law functions on the device -------------------------------------------------------------------------------
@pytest.mark.parametrize("op", list(cr.OPS))
def test_curve_op_edges_and_random(harnesses, clibs, op):  # noqa: F811
    t0 = time.time()
    edges = cr.edge_set(op)
    _run_and_check(harnesses, clibs, op, edges)
    items = cr.random_set(op, random.Random(0xC0DE000 + cr.OPS[op]), N_RANDOM)
    _run_and_check(harnesses, clibs, op, items)
    print("[curve fuzz] %-12s edges %5d  random %6d  %5.1f s" % (op, len(edges), len(items), time.time() - t0))


def test_fixed_table_chain_equals_the_entry_definition(harnesses):
    """on the device: the chain-built table is fixed_table_entry limb for limb for every chain length, the link check counts
    nothing on it and something at the slot of every flipped bit tried"""
    slots = _padded([((s % 9, s // 9, 1 if s < 9 else 0),) for s in range(cr.FT_SLOTS)])
    a, _ = cr.records("fixed_entry", slots)
    entries = harnesses[0].run("fixed_entry", a, None)[:cr.FT_SLOTS]
    chains = _padded(cr.edge_set("fixed_chain"))
    a, _ = cr.records("fixed_chain", chains)
    out = harnesses[0].run("fixed_chain", a, None).reshape(len(chains), cr.FT_SLOTS, 28)
    assert (out[:, :, :27] == entries[None, :, :]).all() and (out[:, :, 27] == 0).all()
    flips = _padded(cr.edge_set("fixed_flip"))
    a, _ = cr.records("fixed_flip", flips)
    assert (harnesses[0].run("fixed_flip", a, None)[:, 0] > 0).all()


# ---- (2) the same edges through the C ABI, against the C oracle ------------------------------------------------------------------
def _rows(vals, per_row):
    return pack(vals).reshape(-1, 32 * per_row)


def test_abi_point_add_every_pair_of_edge_points(gpu_ctx, oracle):
    pts = cr.ref_edge_points()
    pairs = [(p, q) for p in pts for q in pts]
    P, Q = _rows([p for p, _ in pairs], 2), _rows([q for _, q in pairs], 2)
    want = oracle.point_add(P, Q)
    model = _rows([cr.from_m1(cr.add_m1(cr.to_m1(p), cr.to_m1(q))) for p, q in pairs], 2)
    assert (want == model).all()                                              # the oracle and the group law agree
    got = gpu_ctx.point_add(P, Q)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, [pairs[i] for i in bad[:3]]
    for i in range(0, len(pairs), 7):                                         # one-item calls
        assert (gpu_ctx.point_add(P[i:i + 1], Q[i:i + 1]) == want[i:i + 1]).all(), pairs[i]


def test_abi_proj_add_then_affine_on_scaled_edge_points(gpu_ctx, oracle):
    """bjj_proj_add on every ordered pair, the operands scaled by z = 1, r - 1 or one seeded z: x3, y3, z3 are the reference formula's,
    coordinate by coordinate, and bjj_proj_affine of them is the oracle's sum of the affine points"""
    pts = cr.ref_edge_points()
    zs = [1, R_MOD - 1, random.Random(0x2EF).randrange(2, R_MOD)]
    trip, aff = [], []
    for i, p in enumerate(pts):
        for j, q in enumerate(pts):
            for k, z1 in enumerate(zs):
                z2 = zs[(i + j + k) % 3]
                trip.append(((p[0] * z1 % R_MOD, p[1] * z1 % R_MOD, z1), (q[0] * z2 % R_MOD, q[1] * z2 % R_MOD, z2)))
                aff.append((p, q))
    P, Q = _rows([p for p, _ in trip], 3), _rows([q for _, q in trip], 3)
    got = gpu_ctx.proj_add(P, Q)
    assert unpack(got, 3) == [cr.proj_add(p, q) for p, q in trip]
    want = oracle.point_add(_rows([p for p, _ in aff], 2), _rows([q for _, q in aff], 2))
    assert (gpu_ctx.proj_affine(got) == want).all()
    for i in range(0, len(trip), 41):                                         # one-item calls
        assert (gpu_ctx.proj_affine(gpu_ctx.proj_add(P[i:i + 1], Q[i:i + 1])) == want[i:i + 1]).all(), trip[i]


def test_abi_vanishing_denominators(gpu_ctx, oracle):
    """operands with z1, z2 != 0 whose sum has f = 0 or g = 0: z3 = 0 and affine() answers (0, 0); with z = 1 operands the same
    through bjj_point_add, where the oracle answers (0, 0) too"""
    vp = cr.vanishing_pairs()
    P, Q = _rows([p for p, _, _ in vp], 3), _rows([q for _, q, _ in vp], 3)
    got = gpu_ctx.proj_add(P, Q)
    assert unpack(got, 3) == [cr.proj_add(p, q) for p, q, _ in vp]
    assert all(t[2] == 0 for t in unpack(got, 3))
    assert (gpu_ctx.proj_affine(got) == 0).all()
    flat = [(p[:2], q[:2]) for p, q, _ in vp if p[2] == 1 and q[2] == 1]
    assert len(flat) >= 6
    A, B = _rows([p for p, _ in flat], 2), _rows([q for _, q in flat], 2)
    want = oracle.point_add(A, B)
    assert (want == 0).all() and (gpu_ctx.point_add(A, B) == want).all()
    for i in range(len(flat)):
        assert (gpu_ctx.point_add(A[i:i + 1], B[i:i + 1]) == 0).all()


def test_abi_mul_var_base_edge_points_times_edge_scalars(gpu_ctx, oracle):
    """every edge point times every edge scalar, and the operands of the vanishing pairs -- off the curve -- as bases with the
    scalars 2, 3 and a full-width one.  Calls of at most 2^14 items go to the four-lane short-call kernel (k_small.hip), which
    has a ladder of its own; so the items are first sent tiled past 2^14 in one call, which runs K2 (k_var.hip: the kernel that
    calls vb_build_table and vb_mul_windowed on packed per-lane tables), then as they are and one at a time (the short-call
    kernel).  last_var_base_form says which kernel ran: 0 or 1 for K2, 2 for the short-call kernel."""
    pts = cr.ref_edge_points()
    sc = cr.edge_scalars()
    items = [(p, s) for p in pts for s in sc]
    items += [(p[:2], s) for p, q, _ in cr.vanishing_pairs()[:3] for s in (2, 3, (1 << 254) - 1)]
    P, S = _rows([p for p, _ in items], 2), _rows([s for _, s in items], 1)
    want = oracle.mul_var_base(P, S)
    reps = (1 << 14) // len(items) + 1
    assert reps * len(items) > 1 << 14
    got = gpu_ctx.mul_var_base(np.tile(P, (reps, 1)), np.tile(S, (reps, 1)))  # K2
    assert gpu_ctx.info().last_var_base_form in (0, 1)
    bad = np.nonzero((got != np.tile(want, (reps, 1))).any(axis=1))[0]
    assert bad.size == 0, [items[i % len(items)] for i in bad[:3]]
    got = gpu_ctx.mul_var_base(P, S)                                          # the short-call kernel
    assert gpu_ctx.info().last_var_base_form == 2
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, [items[i] for i in bad[:3]]
    # the oracle's answers are the group law's on the curve
    for i in range(0, len(pts) * len(sc), 13):
        p, s = items[i]
        X, Y, Z = cr.smul_known(cr.to_m1(p), s)
        zi = cr.inv(Z)
        assert unpack(want[i], 2)[0] == (X * zi * cr.FINV % R_MOD, Y * zi % R_MOD), items[i]
    step = len(items) // 8 + 1
    for i in list(range(8)) + list(range(step, len(items), step)):            # and eight more, spread over points and scalars
        assert (gpu_ctx.mul_var_base(P[i:i + 1], S[i:i + 1]) == want[i:i + 1]).all(), items[i]
        assert gpu_ctx.info().last_var_base_form == 2
