"""The additive, comparison, conversion, square-root and codec field code on the device (csrc/fr.hpp, csrc/bjj_device.hpp:536-659,
ref_on_curve): the layer between the multiplier fuzz of tests/test_gpu_devfuzz.py and the byte-for-byte ABI parity tests.

(1) tests/devfuzz/field.hip runs the functions that ship, one item per lane, on the edge sets of tests/field_ref.py plus 2^16
seeded random items per op; the results are compared bit for bit with the g++ build of the same dispatcher
(tests/emul/emul_field_ops.cpp) on every item and checked against plain integers.
(2) The same edges through the C ABI where it can reach them: bjj_poseidon5 with inputs at the multiples of r (one call and row
by row: the short-call kernels), bjj_compress_points and bjj_decompress_points on the codec edge sets, against the C oracle and
the model.  Needs a real MI355X: `pytest -m gpu`."""
import ctypes
import os
import random
import subprocess
import time

import numpy as np
import pytest

import field_ref as fr
from conftest import ROOT, pack
from dispatch_forms import LANE, SHORT, lane_ctx, ran  # noqa: F401  (lane_ctx: the fixture)
from test_field_ops_host import flib  # noqa: F401  (the fixture that builds the CPU library of the same dispatcher)

pytestmark = pytest.mark.gpu

R_MOD = fr.R_MOD
N_RANDOM = 1 << 16                 # seeded random items per op


class FieldHarness:
    """ctypes view of tests/devfuzz/libbjj_field_test.so"""

    def __init__(self):
        d = os.path.join(ROOT, "tests", "devfuzz")
        so = os.path.join(d, "libbjj_field_test.so")
        # always through make: it knows the product headers the harness includes, so an edit of csrc/ never runs a stale library
        r = subprocess.run(["make", "-s", "libbjj_field_test.so"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        import torch  # noqa: F401  (loads the HIP runtime first, see babyjubjub-rs_amd/_lib.py)
        self.lib = ctypes.CDLL(so)
        vp = ctypes.c_void_p
        self.lib.fo_run.argtypes = [ctypes.c_int, vp, vp, vp, ctypes.c_size_t, vp]
        self.lib.fo_words.argtypes = [ctypes.c_int, ctypes.c_int]
        for op, code in fr.OPS.items():
            assert tuple(self.lib.fo_words(code, k) for k in range(3)) == fr.WIDTHS[op], op

    def run(self, op, a, b):
        """the op on the device: a, b uint32 records (numpy) -> (n, out words) uint32 (numpy)"""
        import torch
        code = fr.OPS[op]
        n = a.shape[0]
        wa, wb, wo = fr.WIDTHS[op]
        assert a.shape == (n, wa) and ((b is None and wb == 0) or (b is not None and b.shape == (n, wb)))
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32).reshape(-1)).cuda()  # noqa: E731
        d_a = dev(a)
        d_b = dev(b) if b is not None else None
        guard = 64
        d_o = torch.full((n * wo + guard,), -0x11111112, dtype=torch.int32, device="cuda")   # 0xEEEEEEEE
        rc = self.lib.fo_run(code, d_a.data_ptr(), d_b.data_ptr() if d_b is not None else None, d_o.data_ptr(), n, None)
        assert rc == 0
        torch.cuda.synchronize()
        o = d_o.cpu().numpy().view(np.uint32)
        assert (o[n * wo:] == 0xEEEEEEEE).all()            # nothing written past the last record
        return o[:n * wo].reshape(n, wo)


@pytest.fixture(scope="module")
def fo():
    return FieldHarness()


def _run_and_check(fo, flib, op, items):  # noqa: F811
    a, b = fr.records(op, items)
    got = fo.run(op, a, b)
    want = fr.cpu_run(flib, op, a, b)
    diff = np.nonzero((got != want).any(axis=1))[0]
    assert diff.size == 0, (op, "device != CPU harness", diff.size, [(items[i], got[i].tolist(), want[i].tolist()) for i in diff[:3]])
    bad = fr.check(op, items, got)
    assert bad == [], (op, len(bad), [(items[i], why) for i, why in bad[:3]])
    return got


# ---- (1) the field functions on the device ----------------------------------------------------------------------------------
@pytest.mark.parametrize("op", list(fr.OPS))
def test_field_op_edges_and_random(fo, flib, op):  # noqa: F811
    t0 = time.time()
    edges = fr.edge_set(op)
    got_e = _run_and_check(fo, flib, op, edges)
    items = fr.random_set(op, random.Random(0xF1E1D000 + fr.OPS[op]), N_RANDOM)
    got_r = _run_and_check(fo, flib, op, items)
    # a partly filled wave: 65 items alone give what they gave inside the full launches
    got_65 = _run_and_check(fo, flib, op, (edges + items)[:65])
    assert (got_65 == np.concatenate([got_e, got_r])[:65]).all()
    print("[field fuzz] %-12s edges %5d  random %6d  %5.1f s" % (op, len(edges), len(items), time.time() - t0))


# ---- (2) the same edges through the C ABI -----------------------------------------------------------------------------------
def _bytes_rows(vals, per_row):
    return pack(vals).reshape(-1, 32 * per_row)


def poseidon_edge_rows():
    """each edge value in each of the five positions with the other four random, and in all five at once"""
    edge = [0, 1, R_MOD - 1] + [k * R_MOD + d for k in range(1, 6) for d in (-1, 0, 1)] + [(1 << 256) - 1]
    assert all(0 <= v < 1 << 256 for v in edge)
    rnd = random.Random(0xF1E1DA)
    rows = []
    for v in edge:
        for p in range(5):
            row = [rnd.getrandbits(256) if rnd.randrange(2) else rnd.randrange(R_MOD) for _ in range(5)]
            row[p] = v
            rows.append(tuple(row))
        rows.append((v,) * 5)
    return rows


def test_abi_poseidon5_inputs_at_multiples_of_r(gpu_ctx, lane_ctx, oracle):  # noqa: F811
    """inputs >= r are reduced mod r (include/bjj_hip.h): the hash of the row equals the hash of the row reduced in plain
    integers -- the model's expectation -- and the C oracle's hash of the row as it is.  Every call here is a short one, which
    the session's context runs six lanes per hash (last_poseidon_form 1); the rows go through a context whose short calls run
    one hash per lane (0), the kernel of the large calls, as well"""
    rows = poseidon_edge_rows()
    raw = _bytes_rows(rows, 5)
    want = oracle.poseidon5(_bytes_rows([tuple(v % R_MOD for v in row) for row in rows], 5))
    assert (oracle.poseidon5(raw) == want).all()
    for ctx, form in ((gpu_ctx, SHORT), (lane_ctx, LANE)):
        got = ctx.poseidon5(raw)                                              # one call
        ran(ctx, "poseidon", form)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (form, [rows[i] for i in bad[:3]])
    for i in range(len(rows)):                                                # row by row: the short-call kernels
        assert (gpu_ctx.poseidon5(raw[i:i + 1]) == want[i:i + 1]).all(), rows[i]
    for i in range(0, len(rows) - 5, 7):                                      # and a few rows at a time
        assert (gpu_ctx.poseidon5(raw[i:i + 5]) == want[i:i + 5]).all(), i
    ran(gpu_ctx, "poseidon", SHORT)


def test_abi_compress_points_edges(gpu_ctx, oracle):
    pts = fr.compress_edge_values()
    raw = _bytes_rows(pts, 2)
    model = _bytes_rows([fr.compress_model(x, y) for x, y in pts], 1)
    got = gpu_ctx.compress_points(raw)
    bad = np.nonzero((got != model).any(axis=1))[0]
    assert bad.size == 0, [pts[i] for i in bad[:3]]
    canon = np.array([x < R_MOD and y < R_MOD for x, y in pts])
    assert canon.sum() >= 20
    assert (got[canon] == oracle.compress(raw[canon])).all()
    for i in range(len(pts)):                                                 # one-item calls
        assert (gpu_ctx.compress_points(raw[i:i + 1]) == model[i:i + 1]).all(), pts[i]


def test_abi_decompress_points_edges(gpu_ctx, oracle):
    vals = fr.decompress_edge_values()
    raw = _bytes_rows(vals, 1)
    want_pts, want_ok = oracle.decompress(raw)
    assert [bool(v) for v in want_ok] == [fr.decompress_ok(v) for v in vals]            # the oracle and the model agree on Ok / Err
    assert 8 <= int(want_ok.sum()) <= len(vals) - 8

    def judge(pts, ok, idx):
        assert (ok == want_ok[idx]).all() and (pts == want_pts[idx]).all(), idx
        out = np.concatenate([ok.astype(np.uint32).reshape(-1, 1), np.ascontiguousarray(pts).view("<u4").astype(np.uint32)], axis=1)
        items = [(fr.words(vals[i]),) for i in idx]
        assert fr.check("decompress", items, out) == []

    pts, ok = gpu_ctx.decompress_points(raw)
    judge(pts, ok, list(range(len(vals))))
    for i in range(len(vals)):                                                # one-item calls
        pts, ok = gpu_ctx.decompress_points(raw[i:i + 1])
        judge(pts, ok, [i])
