"""The scalar side of the library on the device: integers mod l and mod 8l, the Montgomery products mod l, the signers' digest and
nonce reductions, the wide variable-base scalars, verify's c = v*s mod l and the half-size pair (u, v) of the EdDSA fast path.

(1) tests/devfuzz/scalar.hip runs the functions that ship, one item per lane, on the edge sets of tests/scalar_ref.py plus about
10^6 seeded random inputs per op, and the results are checked against Python integers and, bit for bit, against the g++ build of
the same bodies (tests/emul: emul_scalar_op).  Each bound these functions rest on -- the one conditional subtract of
scalar_mod_l, the 261-bit chunks, fl_mul's "a*b < l*2^261, result < 2l", the (1 - 2^-48) under-estimate of the f64 quotient in
euclid_partial_step -- is then asserted on the device's own code.
(2) The same edges through the C ABI against the C oracle: fixed base at the mod-l boundaries (three window widths, both K1
shapes, one-item calls), verification with s + q*l, variable base with k + q*8l and wide scalars, Schnorr nonces at the
chunk edges.  Needs a real MI355X: `pytest -m gpu`."""
import ctypes
import os
import random
import subprocess
import time

import numpy as np
import pytest

import scalar_ref as sr
from conftest import ROOT, pack, unpack
from dispatch_forms import LANE, SHORT, both, lane_ctx, ran  # noqa: F401  (lane_ctx: the fixture)

pytestmark = pytest.mark.gpu

L, ORDER = sr.L, sr.ORDER
N_RANDOM = 1 << 20                 # seeded random inputs per op
N_PY_SHORT_PAIR = 1 << 17          # of which the Python restatement of the pair selection checks this many (the CPU harness: all)


class ScalarHarness:
    """ctypes view of tests/devfuzz/libbjj_scalar_test.so"""

    def __init__(self):
        d = os.path.join(ROOT, "tests", "devfuzz")
        so = os.path.join(d, "libbjj_scalar_test.so")
        # always through make: it knows the product headers the harness includes, so an edit of csrc/ never runs a stale library
        r = subprocess.run(["make", "-s", "libbjj_scalar_test.so"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        import torch  # noqa: F401  (loads the HIP runtime first, see babyjubjub-rs_amd/_lib.py)
        self.lib = ctypes.CDLL(so)
        vp = ctypes.c_void_p
        self.lib.sc_run.argtypes = [ctypes.c_int, vp, vp, vp, ctypes.c_size_t, ctypes.c_int, vp]
        self.lib.sc_words.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]

    def run(self, op, a, b, nw=0):
        """the op on the device: a, b uint32 records (numpy) -> (n, out words) uint32 (numpy)"""
        import torch
        code = sr.OPS[op]
        n = a.shape[0]
        wa, wb, wo = (self.lib.sc_words(code, nw, k) for k in range(3))
        assert a.shape == (n, wa) and wa == sr.a_words(op, nw) and wo == sr.OUT_WORDS.get(op, 8)
        assert (b is None and wb == 0) or (b is not None and b.shape == (n, wb))
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32).reshape(-1)).cuda()  # noqa: E731
        d_a = dev(a)
        d_b = dev(b) if b is not None else None
        guard = 64
        d_o = torch.full((n * wo + guard,), -0x11111112, dtype=torch.int32, device="cuda")   # 0xEEEEEEEE
        rc = self.lib.sc_run(code, d_a.data_ptr(), d_b.data_ptr() if d_b is not None else None, d_o.data_ptr(), n, nw, None)
        assert rc == 0
        torch.cuda.synchronize()
        o = d_o.cpu().numpy().view(np.uint32)
        assert (o[n * wo:] == 0xEEEEEEEE).all()            # nothing written past the last record
        return o[:n * wo].reshape(n, wo)


@pytest.fixture(scope="module")
def sc():
    return ScalarHarness()


def _run_and_check(sc, cpu, op, items, nw=0, py_limit=None):
    a, b = sr.records(op, items, nw)
    got = sc.run(op, a, b, nw)
    want = sr.cpu_run(cpu, op, a, b, nw)
    diff = np.nonzero((got != want).any(axis=1))[0]
    assert diff.size == 0, (op, nw, "device != CPU harness", diff.size, [items[i] for i in diff[:3]])
    k = len(items) if py_limit is None else min(len(items), py_limit)
    bad = sr.check(op, items[:k], got[:k])
    assert bad == [], (op, nw, len(bad), bad[:3])
    return got


_EUCLID = {}    # "bad": what the device's euclid_partial_step got wrong on the Euclid edge set (empty: nothing)


def _require_exact_euclid(sc):
    """lattice_short_pair loops until the remainder drops below 2^126.  A euclid_partial_step whose quotient can exceed
    floor(r0 / r1) wraps r0 below zero, and that loop then never ends: a hung kernel on a shared GPU, not a failing test.  So
    nothing that runs lattice_short_pair on the device -- the short_pair op, the EdDSA verify calls -- is launched before the
    device's Euclid step has passed its edge set (one launch of a single step, which always terminates; cached per session)."""
    if "bad" not in _EUCLID:
        edges = sr.edge_set("euclid")
        a, b = sr.records("euclid", edges)
        _EUCLID["bad"] = [(edges[i], why) for i, why in sr.check("euclid", edges, sc.run("euclid", a, b))]
    bad = _EUCLID["bad"]
    if bad:
        pytest.fail("not launched: the device's euclid_partial_step fails %d Euclid edge(s), e.g. %s -- lattice_short_pair would "
                    "not terminate" % (len(bad), bad[0][1]), pytrace=False)


# ---- (1) the scalar functions on the device ---------------------------------------------------------------------------------
@pytest.mark.parametrize("emul", [0], indirect=True, ids=["cpu"])
def test_scalar_euclid_step_first(sc, emul):
    """euclid_partial_step on its own, before anything that loops on it (one step per item: a quotient that is too large fails
    here instead of hanging the half-size pair): the quotient used lies in [1, floor(r0 / r1)] -- the (1 - 2^-48)
    under-estimate on the device's own f64 division"""
    t0 = time.time()
    _require_exact_euclid(sc)
    edges = sr.edge_set("euclid")
    _run_and_check(sc, emul, "euclid", edges)
    items = sr.random_set("euclid", random.Random(0x5CA1_0000 + sr.OPS["euclid"]), N_RANDOM)
    _run_and_check(sc, emul, "euclid", items)
    print("[scalar fuzz] %-11s edges %6d  random %8d  %6.1f s" % ("euclid", len(edges), len(items), time.time() - t0))


OPS_FIXED = ["mod_l", "mod_order", "plain_mod_l", "fl_mul", "fl_canon4", "digest", "nonce", "verify_c", "short_pair"]


@pytest.mark.parametrize("emul", [0], indirect=True, ids=["cpu"])
@pytest.mark.parametrize("op", OPS_FIXED)
def test_scalar_op_edges_and_random(sc, emul, op):
    t0 = time.time()
    if op == "short_pair":
        _require_exact_euclid(sc)
    edges = sr.edge_set(op)
    if op == "short_pair":
        assert {sr.pair_outcome(k) for k in edges} == {"odd", "prev", "next", "degenerate"}
    _run_and_check(sc, emul, op, edges)
    rnd = random.Random(0x5CA1_0000 + sr.OPS[op])
    items = sr.random_set(op, rnd, N_RANDOM)
    _run_and_check(sc, emul, op, items, py_limit=N_PY_SHORT_PAIR if op == "short_pair" else None)
    print("[scalar fuzz] %-11s edges %6d  random %8d  %6.1f s" % (op, len(edges), len(items), time.time() - t0))


@pytest.mark.parametrize("emul", [0], indirect=True, ids=["cpu"])
def test_scalar_wide_every_word_count(sc, emul):
    """wide_scalar_mod_order at every word count bjj_mul_var_base_wide admits (scalar_bytes = 32, 64, ..., 4096)"""
    t0 = time.time()
    rnd = random.Random(0x5CA1_0007)
    ne = nr = 0
    for nw in sr.WIDE_WORD_COUNTS:
        edges = sr.edges_wide(nw)
        items = edges + sr.random_set("wide", rnd, max(256, (1 << 19) // nw), nw)
        _run_and_check(sc, emul, "wide", items, nw)
        ne += len(edges)
        nr += len(items) - len(edges)
    print("[scalar fuzz] %-11s edges %6d  random %8d  %6.1f s" % ("wide", ne, nr, time.time() - t0))


# ---- (2) the same edges through the C ABI -----------------------------------------------------------------------------------
def _fixed_base_scalars():
    rnd = random.Random(0xFB)
    return sr.edges_mod_l() + [rnd.getrandbits(256) for _ in range(256)]


def _check_fixed_base(ctx, oracle, vals, one_item=48, forced_k1=False):
    """the values in one call, which is a short one (four lanes per item) unless the context forces a shape of K1, and tiled
    past the short-call threshold of 2^15 items, which runs K1 -- both reduce the scalar mod l on their own"""
    sc_ = pack(vals).reshape(-1, 32)
    assert len(vals) <= 1 << 15
    want = oracle.mul_fixed_base(sc_)
    wantc = oracle.compress(want)
    reps = (1 << 15) // len(vals) + 1
    for tile, form in ((1, LANE if forced_k1 else SHORT),) + (() if forced_k1 else ((reps, LANE),)):
        got = ctx.mul_fixed_base(np.tile(sc_, (tile, 1)))
        ran(ctx, "fixed", form)
        bad = np.nonzero((got != np.tile(want, (tile, 1))).any(axis=1))[0]
        assert bad.size == 0, (form, [vals[i % len(vals)] for i in bad[:4]])
        comp = ctx.mul_fixed_base_compressed(np.tile(sc_, (tile, 1)))
        ran(ctx, "fixed", form)
        bad = np.nonzero((comp != np.tile(wantc, (tile, 1))).any(axis=1))[0]
        assert bad.size == 0, (form, [vals[i % len(vals)] for i in bad[:4]])
    step = max(1, len(vals) // one_item)
    for i in range(0, len(vals), step):                   # one-item calls: the quad kernel
        assert (ctx.mul_fixed_base(sc_[i:i + 1]) == want[i:i + 1]).all(), vals[i]
    ran(ctx, "fixed", LANE if forced_k1 else SHORT)


def test_abi_fixed_base_mod_l_boundaries(gpu_ctx, ctx_w23, oracle):
    vals = _fixed_base_scalars()
    _check_fixed_base(gpu_ctx, oracle, vals)
    _check_fixed_base(ctx_w23, oracle, vals)


@pytest.mark.parametrize("window,k1", [(8, None), (13, None), (23, "1")], ids=["w8", "w13", "w23_k1_variant1"])
def test_abi_fixed_base_mod_l_boundaries_windows(oracle, monkeypatch, window, k1):
    import babyjubjub_rs_amd as bjj
    if k1 is not None:
        monkeypatch.setenv("BJJ_K1_VARIANT", k1)
    ctx = bjj.Context(0, window)
    if k1 is not None:
        monkeypatch.delenv("BJJ_K1_VARIANT")
    try:
        assert ctx.info().window_bits == window
        _check_fixed_base(ctx, oracle, _fixed_base_scalars(), one_item=16, forced_k1=k1 is not None)
    finally:
        ctx.close()


def _eddsa_cases(oracle, nsig):
    """valid signatures with s + q l for every q (s + q l < 2^256): verdict 1; s + q l +- 1: verdict 0"""
    from babyjubjub_rs_amd import workload as w
    A, R, S, msg = w.make_signatures(oracle.mul_fixed_base, oracle.poseidon5, nsig, offset=0x5CA1)
    rows, want = [], []
    for i, s in enumerate(unpack(S)):
        for q in range(44):
            for d in (0, -1, 1):
                v = s + q * L + d
                if 0 <= v < 1 << 256:
                    rows.append((i, v))
                    want.append(1 if d == 0 else 0)
    idx = np.array([i for i, _ in rows])
    return A[idx], R[idx], pack([v for _, v in rows]).reshape(-1, 32), msg[idx], np.array(want, np.uint8)


def test_abi_eddsa_verify_s_plus_multiples_of_l(gpu_ctx, lane_ctx, oracle, sc):  # noqa: F811
    _require_exact_euclid(sc)                                                     # the EdDSA fast path runs lattice_short_pair
    A, R, S, msg, want = _eddsa_cases(oracle, 12)
    assert (oracle.verify(A, R, S, msg) == want).all()
    assert len(want) <= 1 << 13                   # a short call all the same: eight lanes per signature; then K4 on the same batch
    for ctx, form in both(gpu_ctx, lane_ctx):
        assert (ctx.eddsa_verify(A, R, S, msg) == want).all(), form               # one long batch
        ran(ctx, "verify", form)
    for i in range(0, len(want), 37):                                             # short calls
        assert (gpu_ctx.eddsa_verify(A[i:i + 5], R[i:i + 5], S[i:i + 5], msg[i:i + 5]) == want[i:i + 5]).all(), i
    # the wire format: compressed pk, compressed R || s
    pkc, rc = oracle.compress(A), oracle.compress(R)
    sig = np.concatenate([rc, S], axis=1)
    assert (oracle.verify_compressed(pkc, sig, msg) == want).all()
    for ctx, form in both(gpu_ctx, lane_ctx):
        assert (ctx.eddsa_verify_compressed(pkc, sig, msg) == want).all(), form
        ran(ctx, "verify", form)


def test_abi_schnorr_verify_s_plus_multiples_of_l(gpu_ctx, lane_ctx, oracle):  # noqa: F811
    rng = np.random.default_rng(0x5CA1)
    n = 8
    keys = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msgs = rng.integers(0, 256, (n, 32), dtype=np.uint8); msgs[:, 31] &= 0x1f
    nonces = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    r, s, ok = gpu_ctx.sign_schnorr(keys, msgs, nonces)
    assert ok.all()
    pk = gpu_ctx.public_keys(keys)
    ran(gpu_ctx, "fixed", SHORT)
    assert (lane_ctx.public_keys(keys) == pk).all()
    ran(lane_ctx, "fixed", LANE)
    rows, want = [], []
    for i in range(n):
        sl = int.from_bytes(s[i].tobytes(), "little") % L
        for q in range(44):
            for d in (0, -1, 1):
                v = sl + q * L + d
                if 0 <= v < 1 << 256:
                    rows.append((i, v))
                    want.append(1 if d == 0 else 0)
    idx = np.array([i for i, _ in rows])
    sv, want = pack([v for _, v in rows]).reshape(-1, 32), np.array(want, np.uint8)
    assert (oracle.verify_schnorr(pk[idx], r[idx], sv, msgs[idx]) == want).all()
    for ctx, form in both(gpu_ctx, lane_ctx):     # about a thousand signatures: a short call, and K4 on the same batch
        assert (ctx.schnorr_verify(pk[idx], r[idx], sv, msgs[idx]) == want).all(), form
        ran(ctx, "verify", form)


def _group_points(ctx, n, seed):
    from babyjubjub_rs_amd import workload as w
    return ctx.mul_fixed_base(w.scalars_254(n, offset=seed)).copy()


def test_abi_var_base_k_plus_multiples_of_8l(gpu_ctx, lane_ctx, oracle):  # noqa: F811
    """for on-curve points n*P == (n mod 8l)*P: k + q 8l gives k's result, in short calls, in one batch and in bjj_msm"""
    rnd = random.Random(0x88)
    m = 16
    pts = _group_points(gpu_ctx, m, 0x5CA1)
    ks = [0, 1, ORDER - 1, L, L - 1, 2 * L + 1] + [rnd.randrange(ORDER) for _ in range(m - 6)]
    want = oracle.mul_var_base(pts, pack(ks).reshape(-1, 32))
    rows = [(i, k + q * ORDER) for i, k in enumerate(ks) for q in range(6) if k + q * ORDER < 1 << 256]
    idx = np.array([i for i, _ in rows])
    big = pack([v for _, v in rows]).reshape(-1, 32)
    for ctx, form in both(gpu_ctx, lane_ctx):     # four lanes per item and K2: each reduces the scalar mod 8l on its own
        got = ctx.mul_var_base(pts[idx], big)
        ran(ctx, "var", form)
        assert (got == want[idx]).all(), form
    for j in range(0, len(rows), 5):                                                # short calls (quad kernel)
        assert (gpu_ctx.mul_var_base(pts[idx[j:j + 3]], big[j:j + 3]) == want[idx[j:j + 3]]).all(), rows[j]
    # msm: the same sum with every scalar replaced by k + q 8l (the largest q that fits)
    ref = gpu_ctx.msm(pts, pack(ks).reshape(-1, 32))
    acc = want[0:1]
    for i in range(1, m):
        acc = oracle.point_add(acc, want[i:i + 1])
    assert (ref == acc).all()
    for q in range(1, 6):
        kq = [k + q * ORDER if k + q * ORDER < 1 << 256 else k + (q - 1) * ORDER for k in ks]
        assert (gpu_ctx.msm(pts, pack(kq).reshape(-1, 32)) == acc).all(), q


def test_abi_var_base_wide_every_word_count(gpu_ctx, lane_ctx, oracle):  # noqa: F811
    """bjj_mul_var_base_wide on the wide edge set, every scalar_bytes, against the oracle at n mod 8l"""
    pts_all = _group_points(gpu_ctx, 64, 0x71DE)
    for nw in sr.WIDE_WORD_COUNTS:
        vals = sr.edges_wide(nw)
        pts = pts_all[np.arange(len(vals)) % 64]
        scal = sr.words(vals, nw).view(np.uint8).reshape(len(vals), 4 * nw)
        want = oracle.mul_var_base(pts, pack([v % ORDER for v in vals]).reshape(-1, 32))
        # 32-byte scalars in a short call run four lanes per item: those go to K2 as well; wider ones run K2 at every size
        for ctx, form in ((gpu_ctx, SHORT if nw == 8 else LANE),) + (((lane_ctx, LANE),) if nw == 8 else ()):
            got = ctx.mul_var_base_wide(pts, scal, 4 * nw)
            ran(ctx, "var", form)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (nw, form, [hex(vals[i]) for i in bad[:3]])


SCHNORR_NONCES_ELSEWHERE = {0, 1, L - 1, L, (1 << 261) - 1, 1 << 1023, (1 << 1024) - 1}   # tests/test_schnorr.py signs these


def test_abi_sign_schnorr_nonces_at_chunk_edges(gpu_ctx, oracle):
    """nonces at the 261 / 522 / 783-bit chunk edges that tests/test_schnorr.py does not already sign: R = (k mod l) B8,
    s = k + sk*h with one sk per key, and the signature verifies"""
    nonces = [k for k in sr.edges_nonce() if k not in SCHNORR_NONCES_ELSEWHERE]
    n = len(nonces)
    keys = np.tile(np.arange(32, dtype=np.uint8), (n, 1))
    msgs = pack([12345 + (i % 3) for i in range(n)]).reshape(-1, 32)
    kb = np.frombuffer(b"".join(k.to_bytes(128, "little") for k in nonces), np.uint8).reshape(-1, 128)
    r, s, ok = gpu_ctx.sign_schnorr(keys, msgs, kb)
    assert ok.all()
    assert (r == oracle.mul_fixed_base(pack([k % L for k in nonces]).reshape(-1, 32))).all()
    pk = oracle.public_keys(keys[:1])
    h = unpack(oracle.poseidon5(np.concatenate([np.repeat(pk, n, axis=0), r, msgs], axis=1)))
    sks = set()
    for i, k in enumerate(nonces):
        sv = int.from_bytes(s[i].tobytes(), "little") - k
        assert sv >= 0 and sv % h[i] == 0, i
        sks.add(sv // h[i])
    assert len(sks) == 1
    sl = pack([int.from_bytes(s[i].tobytes(), "little") % L for i in range(n)]).reshape(-1, 32)
    assert (oracle.verify_schnorr(np.repeat(pk, n, axis=0), r, sl, msgs) == 1).all()
