"""The Poseidon permutation on the device as field elements, not verdicts: the layer of the verify, signer and DLEQ kernels between
the multiplier and dot-product fuzz of tests/test_gpu_devfuzz.py and the byte-level ABI tests.

tests/devfuzz/hash.hip runs the functions that ship -- poseidon5_t with its partial rounds one at a time and in pairs, one
poseidon_full_round, dleq_challenge in both forms (hash_ops.hpp, one item per lane) and p5c_hash5, six lanes per hash, in the
launch shape of bjj_k_poseidon5_coop -- on the edge sets of tests/hash_ref.py plus 2^14 seeded random items per op.  The lane ops
are compared BIT FOR BIT with the g++ build of the same dispatcher (tests/emul/emul_hash_ops.cpp, bound assertions live) on
every item; the edges are judged by the plain 68-round model and the C oracle, the random items by the C oracle (the full round:
by the model).  The six-lane form must hold identical limbs on all eight lanes of a group and the model's value mod r.  Every
output is in N-form with a top limb below 2^26; the poseidon.hpp forms stay below 2r, as their header states.
Needs a real MI355X: `pytest -m gpu`."""
import ctypes
import os
import random
import subprocess
import time

import numpy as np
import pytest

import hash_ref as hr
from conftest import ROOT
from test_hash_ops_host import CHALLENGE_OPS, P5_OPS, hlib  # noqa: F401  (hlib: the fixture that builds the CPU library of the same dispatcher)

pytestmark = pytest.mark.gpu

N_RANDOM = 1 << 14                 # seeded random items per op: at most 2^14 hashes per launch
PART_SIZES = (1, 7, 8, 9, 63, 65)  # a group of eight lanes per hash makes 8 the six-lane kernel's boundary, 64 / 65 the lane kernel's wave boundary
GUARD = 64


class HashHarness:
    """ctypes view of tests/devfuzz/libbjj_hash_test.so"""

    def __init__(self):
        d = os.path.join(ROOT, "tests", "devfuzz")
        so = os.path.join(d, "libbjj_hash_test.so")
        # always through make: it knows the product headers the harness includes, so an edit of csrc/ never runs a stale library
        r = subprocess.run(["make", "-s", "libbjj_hash_test.so"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        import torch  # noqa: F401  (loads the HIP runtime first, see babyjubjub-rs_amd/_lib.py)
        self.lib = ctypes.CDLL(so)
        vp = ctypes.c_void_p
        self.lib.ho_run.argtypes = [ctypes.c_int, vp, vp, ctypes.c_size_t, vp]
        self.lib.ho_words.argtypes = [ctypes.c_int, ctypes.c_int]
        self.lib.p5c_run.argtypes = [vp, vp, ctypes.c_size_t, vp]
        for op, code in hr.OPS.items():
            assert tuple(self.lib.ho_words(code, k) for k in range(2)) == hr.WIDTHS[op], op
        self.seconds = 0.0         # spent in upload, launch, sync and download

    def _launch(self, recs, wo, call):
        import torch
        t0 = time.time()
        n = recs.shape[0]
        d_in = torch.from_numpy(np.ascontiguousarray(recs, dtype=np.uint32).view(np.int32).reshape(-1)).cuda()
        d_o = torch.full((n * wo + GUARD,), -0x11111112, dtype=torch.int32, device="cuda")   # 0xEEEEEEEE
        torch.cuda.synchronize()
        assert call(d_in.data_ptr(), d_o.data_ptr(), n) == 0
        torch.cuda.synchronize()
        o = d_o.cpu().numpy().view(np.uint32)
        self.seconds += time.time() - t0
        assert (o[n * wo:] == 0xEEEEEEEE).all()            # nothing written past the last record
        return o[:n * wo].reshape(n, wo)

    def run(self, op, recs):
        """the op of hash_ops.hpp on the device: uint32 records (numpy) -> (n, out words) uint32"""
        wi, wo = hr.WIDTHS[op]
        assert recs.shape[1:] == (wi,)
        return self._launch(recs, wo, lambda i, o, n: self.lib.ho_run(hr.OPS[op], i, o, n, None))

    def six(self, recs):
        """p5c_hash5 on the device: records of 5 x 9 limbs -> (n, 8 lanes x 9 limbs) uint32"""
        assert recs.shape[1:] == (5 * hr.NL,)
        return self._launch(recs, hr.P5C_GROUP * hr.NL, lambda i, o, n: self.lib.p5c_run(i, o, n, None))


@pytest.fixture(scope="module")
def ho():
    return HashHarness()


_SETS, _DEVICE = {}, {}


def _shared(op):
    """the op whose inputs and expectations `op` shares: the two forms of the hash (and the six-lane kernel), the two of the challenge"""
    return "p5_plain" if op in P5_OPS else "challenge_plain" if op in CHALLENGE_OPS else op


def input_set(op):
    """(edges, random items, all records), built once"""
    key = _shared(op)
    if key not in _SETS:
        edges = hr.edge_set(key)
        items = hr.random_set(key, random.Random(0x4A5E000 + hr.OPS[key]), N_RANDOM)
        _SETS[key] = (edges, items, hr.records(key, edges + items))
    return _SETS[key]


def device_results(ho, op):
    """the op's outputs over its whole input set (edges, then random), computed once"""
    if op not in _DEVICE:
        recs = input_set(op)[2]
        ne = len(input_set(op)[0])
        _DEVICE[op] = np.concatenate([ho.run(op, recs[:ne]), ho.run(op, recs[ne:])])       # two launches: at most 2^14 hashes each
    return _DEVICE[op]


_WANT = {}


def wanted(op, oracle):
    """(the model's results on the edges, the C oracle's -- the full round: the model's -- on the random items)"""
    key = _shared(op)
    if key not in _WANT:
        edges, items, _ = input_set(op)
        model = hr.expected(op, edges)
        if op == "full_round":
            _WANT[key] = (model, hr.expected(op, items))
        else:
            assert hr.expected_c(op, edges, oracle) == model               # the model and the C oracle agree on the edges
            _WANT[key] = (model, hr.expected_c(op, items, oracle))
    return _WANT[key]


# ---- the lane forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", list(hr.OPS))
def test_hash_op_edges_and_random(ho, hlib, oracle, op):  # noqa: F811
    edges, items, recs = input_set(op)
    every = edges + items
    t0 = ho.seconds
    got = device_results(ho, op)
    cpu = hr.cpu_run(hlib, op, recs)
    diff = np.nonzero((got != cpu).any(axis=1))[0]
    assert diff.size == 0, (op, "device != CPU harness", diff.size, [(every[i], got[i].tolist(), cpu[i].tolist()) for i in diff[:3]])
    want_e, want_r = wanted(op, oracle)
    bad = hr.check(op, every, got, want_e + want_r)
    assert bad == [], (op, len(bad), [(every[i], why) for i, why in bad[:3]])
    # partly filled launches: the first 1, 7, 8, 9, 63 and 65 items alone give what they gave inside the full launch
    for n in PART_SIZES:
        assert (ho.run(op, recs[:n]) == got[:n]).all(), (op, n)
    k = None if op in CHALLENGE_OPS else 9 if op in P5_OPS else 54
    print("[hash ops] %-15s edges %5d  random %6d  %5.2f s on the GPU%s" % (
        op, len(edges), len(items), ho.seconds - t0, "" if k is None else "  largest output %.4f r" % hr.largest_over_r(got[:, :k])))


@pytest.mark.parametrize("ops", [P5_OPS, CHALLENGE_OPS])
def test_the_two_forms_give_the_same_canonical_words(ho, ops):
    a, b = device_results(ho, ops[0]), device_results(ho, ops[1])
    diff = np.nonzero((a[:, -8:] != b[:, -8:]).any(axis=1))[0]
    assert diff.size == 0, (ops, diff.size, diff[:8].tolist())
    if ops is P5_OPS:       # informative, not asserted: the two forms may return different representatives of the same value
        print("[hash ops] the lane forms' representatives differ on %d of %d items" % (int((a[:, :9] != b[:, :9]).any(axis=1).sum()), len(a)))


# ---- the six-lane form -----------------------------------------------------------------------------------------------------------
def test_six_lane_form_edges_and_random(ho, oracle):
    edges, items, recs = input_set("p5_plain")
    every = edges + items
    ne = len(edges)
    t0 = ho.seconds
    got = np.concatenate([ho.six(recs[:ne]), ho.six(recs[ne:])])
    t1 = ho.seconds
    want_e, want_r = wanted("p5_plain", oracle)
    bad = hr.check_six_lane(every, got, want_e + want_r)
    assert bad == [], (len(bad), [(every[i], why) for i, why in bad[:3]])
    # ... and the value is the lane form's: the canonical words of HO_P5_PLAIN on the same inputs
    lane = device_results(ho, "p5_plain")
    assert [hr.plain(v) for v in hr.vals_of_limbs(got[:, :9])] == hr.vals_of_words(lane[:, 9:])
    for n in PART_SIZES:
        assert (ho.six(recs[:n]) == got[:n]).all(), n
    print("[hash ops] six lanes       edges %5d  random %6d  %5.2f s on the GPU  largest output %.4f r  representative differs from the lane form's on %d items"
          % (ne, len(items), t1 - t0, hr.largest_over_r(got[:, :9]), int((got[:, :9] != lane[:, :9]).any(axis=1).sum())))
