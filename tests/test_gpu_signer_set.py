"""bjj_eddsa_verify_set / bjj_schnorr_verify_set on the MI355X (include/bjj_hip_signer_set.h): verification against a set of signers'
tables, the key chosen per item by an index.  Expected values come from the C oracle -- oracle.verify / oracle.verify_schnorr with
the key records gathered by index -- and, at 65 537 items, from the library's own bjj_eddsa_verify / bjj_schnorr_verify and
bjj_*_verify_signer; never from the code under test, and the pure-Python oracle is not used here.  Inputs
(tests/signer_set_cases.py): signatures under every key of the set, interleaved, 1 in 8 with a seeded bit flip, 1 in 16 presented
under another signer's index, the directed items of two keys behind them."""
import ctypes

import numpy as np
import pytest

import signer_set_cases as ssc
from memguard import DeviceArena, HostArena

pytestmark = pytest.mark.gpu

SHAPES = ((1, 4), (2, 5), (3, 8), (65, 4), (300, 8))       # (k, W)
SIZES = (1, 63, 64, 65, 513, 4097)
NMAX = 4097
BAD = 3
E_INVALID = -1


@pytest.fixture(scope="module")
def keys(oracle, golden):
    cache = {}

    def get(k):
        if k not in cache:
            cache[k] = ssc.key_list(oracle, golden, k)
        return cache[k]
    return get


@pytest.fixture(scope="module")
def data(oracle, keys):
    """(k, schnorr) -> the NMAX items of signer_set_cases.dataset, the oracle's verdicts computed once and never rewritten"""
    cache = {}

    def get(k, schnorr):
        if (k, schnorr) not in cache:
            cache[(k, schnorr)] = ssc.dataset(oracle, keys(k), NMAX, schnorr, 0x5E7000 + k)
        return cache[(k, schnorr)]
    return get


@pytest.fixture(scope="module")
def sets(gpu_ctx, ctx_w23, keys):
    """(context name, k, W) -> SignerSet, created on first use and closed with the module"""
    made = {}
    ctxs = {"gpu_ctx": gpu_ctx, "ctx_w23": ctx_w23}

    def get(which, k, W):
        if (which, k, W) not in made:
            made[(which, k, W)] = ctxs[which].signer_set(keys(k)[3], W)
        return made[(which, k, W)]
    yield get
    for t in made.values():
        t.close()


class ByteDeviceArena(DeviceArena):
    """the device arena with byte-granular offsets: d_ok may sit at any address"""
    max_off_step = 1


def _take(d, sel):
    return {name: np.ascontiguousarray(d[name][sel]) for name in ("idx", "R", "S", "msg", "want")}


def _run(sset, d, schnorr):
    fn = sset.verify_schnorr if schnorr else sset.verify
    return fn(d["idx"], d["R"], d["S"], d["msg"])


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schnorr", [False, True], ids=["eddsa", "schnorr"])
@pytest.mark.parametrize("shape", SHAPES, ids=["k%d_w%d" % s for s in SHAPES])
def test_against_the_oracle(sets, data, shape, schnorr):
    k, W = shape
    sset = sets("gpu_ctx", k, W)
    d = data(k, schnorr)
    for pattern in ssc.PATTERNS:
        sel = ssc.arrange(d, k, pattern)
        # the array as built ends with the directed items: every slice of it is taken from its end, and one from the front;
        # the rearranged ones begin with what the pattern is about (round robin: 64 different signers in the first wave)
        slices = [sel[NMAX - n:] for n in SIZES] + [sel[:65]] if pattern == "random" else [sel[:n] for n in SIZES]
        for part in slices:
            p = _take(d, part)
            got = _run(sset, p, schnorr)
            bad = np.nonzero(got != p["want"])[0]
            assert got.shape == (part.size,) and bad.size == 0, (shape, schnorr, pattern, part.size, bad[:8].tolist())
        if pattern == "round_robin" and k >= 64:
            assert len(set(d["idx"][sel[:64]].tolist())) == 64
        if pattern in ("all_equal", "last_signer"):
            assert set(d["idx"][sel].tolist()) == {0 if pattern == "all_equal" else k - 1}


@pytest.mark.parametrize("schnorr", [False, True], ids=["eddsa", "schnorr"])
def test_on_the_default_context(sets, data, schnorr):
    """23-bit windows: the B8 side has 11 windows there, 9 on the 28-bit context"""
    d = data(65, schnorr)
    sset = sets("ctx_w23", 65, 4)
    for n in (65, NMAX):
        p = _take(d, np.arange(NMAX - n, NMAX))
        assert (_run(sset, p, schnorr) == p["want"]).all(), n


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def set768(gpu_ctx, keys):
    """k = 768 at W = 12 (4.4 GB) -> (SignerSet, None), or (None, the reason) when the device refuses the allocation"""
    import babyjubjub_rs_amd as bjj
    from babyjubjub_rs_amd import _lib
    try:
        big = gpu_ctx.signer_set(keys(768)[3], 12)
    except bjj.BjjError as e:
        if e.code != _lib.BJJ_E_NOMEM:
            raise
        yield None, str(e)
        return
    yield big, None
    big.close()


@pytest.mark.parametrize("schnorr", [False, True], ids=["eddsa", "schnorr"])
def test_byte_offsets_beyond_4_gib(oracle, keys, set768, schnorr):
    """k = 768 at W = 12: 22 x 2049 entries of 128 bytes per signer, so the tables of signers 745 .. 767 begin beyond 2^32 bytes"""
    k, W, n = 768, 12, 513
    eps = 22 * 2049
    assert 744 * eps * 128 < (1 << 32) < 745 * eps * 128
    big, refused = set768
    if big is None:
        pytest.skip("the device refused the 4.4 GB of the set (BJJ_E_NOMEM): %s" % refused)
    assert big.info() == (k, W, 22, k * eps * 128)
    d = ssc.dataset(oracle, keys(k), n, schnorr, 0x768, signers=[0] + list(range(743, 768)))
    assert set(d["idx"].tolist()) <= {0} | set(range(743, 768)) and int((d["idx"] >= 745).sum()) > n // 2
    got = _run(big, d, schnorr)
    bad = np.nonzero(got != d["want"])[0]
    assert bad.size == 0, bad[:8].tolist()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schnorr", [False, True], ids=["eddsa", "schnorr"])
def test_out_of_range_indices_are_data(gpu_ctx, oracle, keys, sets, data, schnorr):
    k, W, n = 65, 4, 513
    sset = sets("gpu_ctx", k, W)
    p = _take(data(k, schnorr), np.arange(NMAX - n, NMAX))
    idx = p["idx"].copy()
    where = {0: k, 63: k + 1, 64: (1 << 32) - 1, 200: k, n - 1: (1 << 32) - 1}
    for i, v in where.items():
        idx[i] = v
    want = p["want"].copy()
    want[list(where)] = BAD
    msg = p["msg"].copy()
    msg[63] = ssc.sc.rec([ssc.Q + 7])[0]                    # msg > Q (Schnorr: 2, EdDSA: 0) under an index outside the set: still 3
    under_0 = (oracle.verify_schnorr if schnorr else oracle.verify)(keys(k)[3][:1], p["R"][63:64], p["S"][63:64], msg[63:64])
    assert under_0.tolist() == [2 if schnorr else 0]       # what signer 0, whose tables such an item walks, alone would give
    ok = np.full(n, 0xEE, np.uint8)
    fn = gpu_ctx.lib.bjj_schnorr_verify_set if schnorr else gpu_ctx.lib.bjj_eddsa_verify_set
    rc = fn(gpu_ctx.handle, sset.handle, idx.ctypes.data, p["R"].ctypes.data, p["S"].ctypes.data, msg.ctypes.data, n, ok.ctypes.data)
    assert rc == 0, gpu_ctx.lib.bjj_last_error()
    bad = np.nonzero(ok != want)[0]
    assert bad.size == 0, bad[:8].tolist()
    assert int((ok == BAD).sum()) == len(where)
    # a whole call of such items, on a set of one signer
    one = sets("gpu_ctx", 1, 4)
    p1 = _take(data(1, schnorr), np.arange(65))
    assert (_run(one, dict(p1, idx=np.full(65, 1, np.uint32)), schnorr) == BAD).all()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schnorr", [False, True], ids=["eddsa", "schnorr"])
def test_65537_against_the_generic_verifier(gpu_ctx, keys, sets, data, schnorr):
    n, k = 65537, 300
    d = data(k, schnorr)
    reps = -(-n // NMAX)
    R, S, M = (np.tile(d[name], (reps, 1))[:n].copy() for name in ("R", "S", "msg"))
    idx = np.tile(d["idx"], reps)[:n].copy()
    rng = np.random.default_rng(0x65537)
    rows = rng.integers(0, n, 4096)
    S[rows, rng.integers(0, 31, 4096)] ^= np.uint8(4)     # so that the tiles differ
    records = keys(k)[3]
    pk = np.ascontiguousarray(records[idx])
    sset = sets("gpu_ctx", k, 8)
    if schnorr:
        got, want = sset.verify_schnorr(idx, R, S, M), gpu_ctx.schnorr_verify(pk, R, S, M)
    else:
        got, want = sset.verify(idx, R, S, M), gpu_ctx.eddsa_verify(pk, R, S, M)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, bad[:8].tolist()
    assert int((want == 1).sum()) > n // 4 and int((want == 0).sum()) > n // 16
    for j in (1, 3, k - 1):                                # order 8l, the unreduced record, the last signer
        own = np.nonzero(idx == j)[0]
        assert own.size > 100
        base = gpu_ctx.base(records[j], 8)
        try:
            ref = (base.verify_schnorr if schnorr else base.verify)(R[own], S[own], M[own])
        finally:
            base.close()
        assert (got[own] == ref).all(), j


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schnorr", [False, True], ids=["eddsa", "schnorr"])
def test_forms_agree(gpu_ctx, sets, data, schnorr):
    import torch
    n, k = NMAX, 65
    d = data(k, schnorr)
    sset = sets("gpu_ctx", k, 4)
    pageable = _run(sset, d, schnorr)
    assert (pageable == d["want"]).all()
    name = "bjj_schnorr_verify_set" if schnorr else "bjj_eddsa_verify_set"
    pins = [gpu_ctx.host_empty(n * 4), gpu_ctx.host_empty(n * 64), gpu_ctx.host_empty(n * 32), gpu_ctx.host_empty(n * 32), gpu_ctx.host_empty(n)]
    try:
        pins[0][:] = d["idx"].view(np.uint8)
        pins[1][:] = d["R"].reshape(-1)
        pins[2][:] = d["S"].reshape(-1)
        pins[3][:] = d["msg"].reshape(-1)
        pins[4][:] = 0xEE
        assert all(gpu_ctx.host_is_pinned(p) for p in pins)
        rc = getattr(gpu_ctx.lib, name)(gpu_ctx.handle, sset.handle, *[p.ctypes.data for p in pins[:4]], n, pins[4].ctypes.data)
        assert rc == 0, gpu_ctx.lib.bjj_last_error()
        assert (pins[4] == pageable).all()
    finally:
        for p in pins:
            gpu_ctx.host_free(p)
    dev = torch.device("cuda", 0)
    d_in = [torch.from_numpy(np.ascontiguousarray(d[name_]).view(np.uint8).reshape(-1).copy()).to(dev) for name_ in ("idx", "R", "S", "msg")]
    d_ok = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    fn = gpu_ctx.schnorr_verify_set_dev if schnorr else gpu_ctx.eddsa_verify_set_dev
    fn(sset, *[t.data_ptr() for t in d_in], n, d_ok.data_ptr())
    gpu_ctx.sync()
    assert (d_ok.cpu().numpy() == pageable).all()


def test_two_streams_at_once(gpu_ctx, sets, data):
    import torch
    dev = torch.device("cuda", 0)
    n = NMAX
    cases = [(sets("gpu_ctx", 300, 8), data(300, False), gpu_ctx.eddsa_verify_set_dev),
             (sets("gpu_ctx", 65, 4), data(65, True), gpu_ctx.schnorr_verify_set_dev)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    d_in = [[torch.from_numpy(np.ascontiguousarray(d[name]).view(np.uint8).reshape(-1).copy()).to(dev) for name in ("idx", "R", "S", "msg")]
            for _, d, _ in cases]
    outs = [torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    for rep_ in range(3):
        for s, (sset, _, fn) in enumerate(cases):
            fn(sset, *[t.data_ptr() for t in d_in[s]], n, outs[s].data_ptr(), stream=streams[s].cuda_stream)
        gpu_ctx.sync()
        for s in range(2):
            assert (outs[s].cpu().numpy() == cases[s][1]["want"]).all(), (rep_, s)
            outs[s].fill_(0xEE)
        torch.cuda.synchronize()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schnorr", [False, True], ids=["eddsa", "schnorr"])
@pytest.mark.parametrize("form", ["dev_all_0", "dev_mixed", "host_pageable", "host_pinned"])
def test_memory_contract(gpu_ctx, sets, data, form, schnorr):
    """n = 65 under the guarded arenas: nothing outside ok[0 : n] is written, the inputs are unchanged, the result does not depend
    on what the output held, and n == 0 and a rejected call leave the output as it was"""
    n, k = 65, 3
    sset = sets("gpu_ctx", k, 8)
    p = _take(data(k, schnorr), np.arange(NMAX - n, NMAX))
    idx = p["idx"].copy()
    idx[7] = k                                             # one item without a signer
    want = p["want"].copy()
    want[7] = BAD
    ins = [("idx", idx.view(np.uint8).reshape(n, 4)), ("r", p["R"]), ("s", p["S"]), ("msg", p["msg"])]
    offs = {"dev_all_0": (0, 0, 0, 0, 0), "dev_mixed": (32, 16, 48, 240, 113), "host_pageable": (4, 1, 8, 33, 100),
            "host_pinned": (0, 16, 7, 0, 251)}[form]     # host index arrays stay 4-byte aligned: they are uint32; the device
    # inputs are 16-byte aligned as the _dev contract asks, d_ok in dev_mixed sits at an odd address
    stem = "bjj_schnorr_verify_set" if schnorr else "bjj_eddsa_verify_set"
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    results = []
    for fill in (0, 1):
        i3 = [(name, arr, o) for (name, arr), o in zip(ins, offs)]
        outs = [("ok", n, offs[4])]
        if form.startswith("dev"):
            a = (ByteDeviceArena if form == "dev_mixed" else DeviceArena)(i3, outs, fill=fill)
        else:
            a = HostArena(i3, outs, fill=fill, pinned_ctx=gpu_ctx if form == "host_pinned" else None)
        try:
            args = (a.ptr("idx"), a.ptr("r"), a.ptr("s"), a.ptr("msg"))
            if form.startswith("dev"):
                rc = getattr(lib, stem + "_dev")(h, sset.handle, *args, n, a.ptr("ok"), None)
            else:
                rc = getattr(lib, stem)(h, sset.handle, *args, n, a.ptr("ok"))
            assert rc == 0, lib.bjj_last_error()
            gpu_ctx.sync()
            out = a.check()["ok"]
            assert getattr(lib, stem + "_dev")(h, sset.handle, *args, 0, a.ptr("ok"), None) == 0
            assert getattr(lib, stem)(h, sset.handle, *args, 0, a.ptr("ok")) == 0
            assert getattr(lib, stem)(h, None, *args, n, a.ptr("ok")) == E_INVALID
            assert getattr(lib, stem + "_dev")(h, None, *args, n, a.ptr("ok"), None) == E_INVALID
            gpu_ctx.sync()
            assert (a.check()["ok"] == out).all()
        finally:
            a.close()
        assert (out == want).all(), (form, fill)
        results.append(out)
    assert (results[0] == results[1]).all()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_rejections(gpu_ctx, ctx_w23, keys, sets, data):
    import torch
    import babyjubjub_rs_amd as bjj
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    n, k = 65, 65
    d = data(k, False)
    I, R, S, M = (np.ascontiguousarray(d[name][:n]) for name in ("idx", "R", "S", "msg"))
    ok = np.full(n, 0xEE, np.uint8)
    sset = sets("gpu_ctx", k, 4)
    foreign = sets("ctx_w23", k, 4)
    host = (lib.bjj_eddsa_verify_set, lib.bjj_schnorr_verify_set)
    devf = (lib.bjj_eddsa_verify_set_dev, lib.bjj_schnorr_verify_set_dev)
    p = (I.ctypes.data, R.ctypes.data, S.ctypes.data, M.ctypes.data)
    for f in host:
        assert f(h, None, *p, n, ok.ctypes.data) == E_INVALID
        assert b"set is NULL" in lib.bjj_last_error()
        assert f(h, foreign.handle, *p, n, ok.ctypes.data) == E_INVALID                  # a set of a second context
        assert b"not a signer set of this context" in lib.bjj_last_error()
        for j in range(4):
            q = list(p)
            q[j] = None
            assert f(h, sset.handle, *q, n, ok.ctypes.data) == E_INVALID
        assert f(h, sset.handle, *p, n, None) == E_INVALID
        assert f(h, sset.handle, None, None, None, None, 0, None) == 0                   # n == 0 looks at nothing
    with pytest.raises(bjj.BjjError):
        gpu_ctx._verify_set(lib.bjj_eddsa_verify_set, "eddsa_verify_set", foreign, I, R, S, M)
    gone = gpu_ctx.signer_set(keys(3)[3], 4)
    stale = gone.handle.value
    gone.close()
    for use in (lambda: gone.verify(I, R, S, M), lambda: gone.verify_schnorr(I, R, S, M), gone.check, gone.info):
        with pytest.raises(bjj.BjjError):                  # the binding refuses a closed set ...
            use()
    bad = ctypes.c_uint64(7)
    for f in host:                                         # ... and the library a handle it does not list
        assert f(h, stale, *p, n, ok.ctypes.data) == E_INVALID
    assert lib.bjj_signer_set_check(h, stale, ctypes.byref(bad)) == E_INVALID and bad.value == 7
    assert lib.bjj_signer_set_free(h, stale) == E_INVALID
    assert lib.bjj_signer_set_free(h, foreign.handle) == E_INVALID
    assert lib.bjj_signer_set_free(h, None) == 0
    assert (ok == 0xEE).all()
    dev = torch.device("cuda", 0)
    pad = np.zeros(16, np.uint8)
    d_in = [torch.from_numpy(np.concatenate([a.view(np.uint8).reshape(-1), pad])).to(dev) for a in (I, R, S, M)]
    d_ok = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device=dev)
    dp = [t.data_ptr() for t in d_in]
    for f in devf:
        for j in range(4):
            q = list(dp)
            q[j] += 8                                      # misaligned
            assert f(h, sset.handle, *q, n, d_ok.data_ptr(), None) == E_INVALID
            q[j] = None
            assert f(h, sset.handle, *q, n, d_ok.data_ptr(), None) == E_INVALID
        assert f(h, sset.handle, *dp, n, None, None) == E_INVALID
        assert f(h, None, *dp, n, d_ok.data_ptr(), None) == E_INVALID
        assert f(h, stale, *dp, n, d_ok.data_ptr(), None) == E_INVALID
        assert f(h, foreign.handle, *dp, n, d_ok.data_ptr(), None) == E_INVALID
        assert f(h, sset.handle, *dp, 0, d_ok.data_ptr(), None) == 0
    gpu_ctx.sync()
    assert bool((d_ok == 0xEE).all())
    # d_ok needs no alignment, as in bjj_eddsa_verify_dev
    assert lib.bjj_eddsa_verify_set_dev(h, sset.handle, *dp, n, d_ok.data_ptr() + 3, None) == 0
    gpu_ctx.sync()
    got = d_ok.cpu().numpy()
    assert (got[3:3 + n] == d["want"][:n]).all() and (got[:3] == 0xEE).all() and (got[3 + n:] == 0xEE).all()


def test_create_rejections(gpu_ctx, keys):
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    recs = keys(65)[3]
    out, first = ctypes.c_void_p(0x77), ctypes.c_int64(42)

    def create(ptr, k, W):
        return lib.bjj_signer_set_create(h, ptr, k, W, ctypes.byref(out), ctypes.byref(first))
    assert create(recs.ctypes.data, 0, 4) == E_INVALID                                   # k == 0
    assert create(None, 3, 4) == E_INVALID
    assert lib.bjj_signer_set_create(h, recs.ctypes.data, 3, 4, None, None) == E_INVALID
    for W in (3, 17, -1, 28):
        assert create(recs.ctypes.data, 3, W) == E_INVALID, W
        assert b"window_bits" in lib.bjj_last_error()
    # k = 8192 at W = 16: 16 x 32769 entries per signer, 8192 of them are 2^32 + 131072 slots -- refused before anything is
    # allocated (it would be 550 GB) and before a key is looked at
    b8 = np.ascontiguousarray(np.broadcast_to(keys(3)[3][2].reshape(1, 64), (8192, 64)))
    assert 8192 * 16 * 32769 > (1 << 32) >= 8191 * 16 * 32769
    assert create(b8.ctypes.data, 8192, 16) == E_INVALID
    assert b"2^32" in lib.bjj_last_error()
    assert out.value == 0x77 and first.value == 42
    # an off-curve key at index 5 of 9 (and a second one behind it): refused, named, *out untouched
    nine = recs[:9].copy()
    nine[5, 32] ^= 1
    nine[7, 0] ^= 1
    assert create(nine.ctypes.data, 9, 4) == E_INVALID
    assert first.value == 5 and out.value == 0x77
    assert b"key 5 is not on the curve" in lib.bjj_last_error()
    import babyjubjub_rs_amd as bjj
    with pytest.raises(bjj.BjjError, match="key 5 is not on the curve"):
        gpu_ctx.signer_set(nine, 4)
    # a valid create reports -1, and out_first_off_curve may be NULL
    first.value = 42
    assert create(recs[:9].ctypes.data, 9, 4) == 0 and first.value == -1 and out.value not in (0, 0x77)
    assert lib.bjj_signer_set_free(h, out) == 0
    out2 = ctypes.c_void_p()
    assert lib.bjj_signer_set_create(h, recs.ctypes.data, 2, 0, ctypes.byref(out2), None) == 0
    k_, w_, nw_ = ctypes.c_uint64(), ctypes.c_int(), ctypes.c_int()
    assert lib.bjj_signer_set_info(out2, ctypes.byref(k_), ctypes.byref(w_), ctypes.byref(nw_), None) == 0
    assert (k_.value, w_.value, nw_.value) == (2, 8, 32)                                 # window_bits 0 = 8
    assert lib.bjj_signer_set_free(h, out2) == 0


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def test_check_info_and_the_context_afterwards(gpu_ctx, oracle, sets, data):
    from babyjubjub_rs_amd import workload
    for k, W in SHAPES:
        sset = sets("gpu_ctx", k, W)
        nwin = -(-255 // W)
        assert sset.info() == (k, W, nwin, k * nwin * ((1 << (W - 1)) + 1) * 128), (k, W)
        assert sset.check() == 0, (k, W)
    d = data(300, False)
    assert (_run(sets("gpu_ctx", 300, 8), d, False) == d["want"]).all()
    assert gpu_ctx.check_table() == 0
    A, R, Sg, msg = workload.make_signatures(oracle.mul_fixed_base, oracle.poseidon5, 64)
    workload.corrupt(A, R, Sg, msg, 64)
    assert (gpu_ctx.eddsa_verify(A, R, Sg, msg) == oracle.verify(A, R, Sg, msg)).all()
