"""bjj_eddsa_verify_signer / bjj_schnorr_verify_signer on the MI355X (include/bjj_hip_signer.h): verification against one signer's
fixed-base table.  Expected values come from the C oracle -- oracle.verify / oracle.verify_schnorr with the signer's record
replicated -- and, at 65 537 items, from the library's own bjj_eddsa_verify / bjj_schnorr_verify; never from the code under test,
and the pure-Python oracle is not used here.  Inputs (tests/signer_cases.py): signatures under ONE key, 1 in 8 with a seeded bit
flip in S, msg or R.y, the directed items behind them; every size is a slice of one array per signer and scheme."""
import numpy as np
import pytest

import signer_cases as sc
from conftest import ints, pack
from memguard import DeviceArena, HostArena

pytestmark = pytest.mark.gpu

Q = sc.Q
WIDTHS = (4, 12, 16)
SIZES = (1, 63, 64, 65, 513, 4097)
NMAX = 4097
SIGNERS = ("ordinary", "order8l", "b8", "unreduced")


def rep(pt_rec, n):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(pt_rec, np.uint8).reshape(1, 64), (n, 64)))


@pytest.fixture(scope="module")
def data(oracle, golden):
    """(signer, schnorr) -> dict(rec = the 64-byte record the table is built from, R, S, msg, want): NMAX items, the directed ones
    last; the oracle's verdicts computed once and never rewritten"""
    tors = [ints(t) for t in golden["gpu_expected"]["torsion_points"]]
    keys = {"ordinary": (sc.KEY_SCALAR, None), "order8l": (sc.KEY_SCALAR + 12345, tors[1]), "b8": (1, None),
            "unreduced": (sc.KEY_SCALAR + 999, None)}
    cache = {}

    def get(signer, schnorr):
        if (signer, schnorr) not in cache:
            k, torsion = keys[signer]
            A = sc.key_point(oracle, k, torsion)
            record = pack([(A[0] + Q, A[1]) if signer == "unreduced" else A]).reshape(1, 64)
            nd = len(sc.DIRECTED)
            R, S, M = sc.bulk(oracle, A, k, NMAX - nd, 0xA110 + len(cache), schnorr, torsion is not None)
            R2, S2, M2 = sc.directed(oracle, A, k, 0xD1 + len(cache), schnorr, torsion is not None)
            R, S, M = np.concatenate([R, R2]), np.concatenate([S, S2]), np.concatenate([M, M2])
            want = (oracle.verify_schnorr if schnorr else oracle.verify)(rep(record, NMAX), R, S, M)
            ones, zeros = int((want == 1).sum()), int((want == 0).sum())
            print("[%s %s] oracle: %d ones, %d zeros of %d" % (signer, "schnorr" if schnorr else "eddsa", ones, zeros, NMAX))
            assert ones >= NMAX // 2 and zeros >= NMAX // 16, (signer, schnorr, ones, zeros)   # else the INPUTS are wrong
            for a in (R, S, M, want, record):
                a.setflags(write=False)
            cache[(signer, schnorr)] = dict(rec=record, R=R, S=S, msg=M, want=want)
        return cache[(signer, schnorr)]
    return get


@pytest.fixture(scope="module")
def tables(gpu_ctx, ctx_w23, data):
    """(context name, signer, W) -> FixedBase, created on first use and closed with the module"""
    made = {}
    ctxs = {"gpu_ctx": gpu_ctx, "ctx_w23": ctx_w23}

    def get(which, signer, W):
        if (which, signer, W) not in made:
            made[(which, signer, W)] = ctxs[which].base(data(signer, False)["rec"], W)
        return made[(which, signer, W)]
    yield get
    for b in made.values():
        b.close()


def _run(base, d, schnorr, lo, hi):
    fn = base.verify_schnorr if schnorr else base.verify
    return fn(d["R"][lo:hi], d["S"][lo:hi], d["msg"][lo:hi])


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schnorr", [False, True], ids=["eddsa", "schnorr"])
@pytest.mark.parametrize("signer", SIGNERS)
def test_against_the_oracle(tables, data, signer, schnorr):
    d = data(signer, schnorr)
    for W in WIDTHS:
        base = tables("gpu_ctx", signer, W)
        for n in SIZES:
            lo = NMAX - n                                  # every slice ends with the directed items
            got = _run(base, d, schnorr, lo, NMAX)
            bad = np.nonzero(got != d["want"][lo:])[0]
            assert got.shape == (n,) and bad.size == 0, (signer, schnorr, W, n, bad[:8].tolist())
        got = _run(base, d, schnorr, 0, 65)                # ... and one from the front
        assert (got == d["want"][:65]).all(), (signer, schnorr, W)


@pytest.mark.parametrize("schnorr", [False, True], ids=["eddsa", "schnorr"])
def test_on_the_default_context(tables, data, schnorr):
    """23-bit windows: the B8 side has 11 windows there, 9 on the 28-bit context"""
    for signer, W in (("order8l", 12), ("ordinary", 16)):
        d = data(signer, schnorr)
        base = tables("ctx_w23", signer, W)
        for n in (65, NMAX):
            got = _run(base, d, schnorr, NMAX - n, NMAX)
            assert (got == d["want"][NMAX - n:]).all(), (signer, W, n)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schnorr", [False, True], ids=["eddsa", "schnorr"])
def test_65537_against_the_generic_verifier(gpu_ctx, oracle, tables, data, schnorr):
    n = 65537
    d = data("order8l", schnorr)
    reps = -(-n // NMAX)
    R, S, M = (np.tile(d[k], (reps, 1))[:n].copy() for k in ("R", "S", "msg"))
    rng = np.random.default_rng(0x65537)
    rows = rng.integers(0, n, 4096)
    S[rows, rng.integers(0, 31, 4096)] ^= np.uint8(4)     # so that the tiles differ
    base = tables("gpu_ctx", "order8l", 16)
    pk = rep(d["rec"], n)
    if schnorr:
        got, want = base.verify_schnorr(R, S, M), gpu_ctx.schnorr_verify(pk, R, S, M)
    else:
        got, want = base.verify(R, S, M), gpu_ctx.eddsa_verify(pk, R, S, M)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, bad[:8].tolist()
    assert int((want == 1).sum()) > n // 4 and int((want == 0).sum()) > n // 16


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schnorr", [False, True], ids=["eddsa", "schnorr"])
def test_forms_agree(gpu_ctx, tables, data, schnorr):
    import torch
    n = NMAX
    d = data("ordinary", schnorr)
    base = tables("gpu_ctx", "ordinary", 12)
    pageable = _run(base, d, schnorr, 0, n)
    assert (pageable == d["want"]).all()
    name = "bjj_schnorr_verify_signer" if schnorr else "bjj_eddsa_verify_signer"
    pins = [gpu_ctx.host_empty(n * 64), gpu_ctx.host_empty(n * 32), gpu_ctx.host_empty(n * 32), gpu_ctx.host_empty(n)]
    try:
        pins[0][:] = d["R"].reshape(-1)
        pins[1][:] = d["S"].reshape(-1)
        pins[2][:] = d["msg"].reshape(-1)
        pins[3][:] = 0xEE
        assert all(gpu_ctx.host_is_pinned(p) for p in pins)
        rc = getattr(gpu_ctx.lib, name)(gpu_ctx.handle, base.handle, pins[0].ctypes.data, pins[1].ctypes.data, pins[2].ctypes.data, n,
                                        pins[3].ctypes.data)
        assert rc == 0, gpu_ctx.lib.bjj_last_error()
        assert (pins[3] == pageable).all()
    finally:
        for p in pins:
            gpu_ctx.host_free(p)
    dev = torch.device("cuda", 0)
    d_in = [torch.from_numpy(d[k].reshape(-1).copy()).to(dev) for k in ("R", "S", "msg")]
    d_ok = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    fn = gpu_ctx.schnorr_verify_signer_dev if schnorr else gpu_ctx.eddsa_verify_signer_dev
    fn(base, d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), n, d_ok.data_ptr())
    gpu_ctx.sync()
    assert (d_ok.cpu().numpy() == pageable).all()


def test_two_streams_at_once(gpu_ctx, tables, data):
    import torch
    dev = torch.device("cuda", 0)
    n = NMAX
    cases = [(tables("gpu_ctx", "ordinary", 16), data("ordinary", False), gpu_ctx.eddsa_verify_signer_dev),
             (tables("gpu_ctx", "order8l", 12), data("order8l", True), gpu_ctx.schnorr_verify_signer_dev)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    d_in = [[torch.from_numpy(d[k].reshape(-1).copy()).to(dev) for k in ("R", "S", "msg")] for _, d, _ in cases]
    outs = [torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    for rep_ in range(3):
        for s, (base, _, fn) in enumerate(cases):
            fn(base, d_in[s][0].data_ptr(), d_in[s][1].data_ptr(), d_in[s][2].data_ptr(), n, outs[s].data_ptr(), stream=streams[s].cuda_stream)
        gpu_ctx.sync()
        for s in range(2):
            assert (outs[s].cpu().numpy() == cases[s][1]["want"]).all(), (rep_, s)
            outs[s].fill_(0xEE)
        torch.cuda.synchronize()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schnorr", [False, True], ids=["eddsa", "schnorr"])
@pytest.mark.parametrize("form", ["dev_all_0", "dev_mixed", "host_pageable", "host_pinned"])
def test_memory_contract(gpu_ctx, tables, data, form, schnorr):
    """n = 65 under the guarded arenas: nothing outside ok[0 : n] is written, the inputs are unchanged, the result does not depend
    on what the output held, and n == 0 and a rejected call leave the output as it was"""
    n = 65
    d = data("order8l", schnorr)
    base = tables("gpu_ctx", "order8l", 4)
    lo = NMAX - n
    want = d["want"][lo:]
    ins = [("r", d["R"][lo:], 0), ("s", d["S"][lo:], 0), ("msg", d["msg"][lo:], 0)]
    offs = {"dev_all_0": (0, 0, 0, 0), "dev_mixed": (16, 48, 240, 112), "host_pageable": (1, 8, 33, 100), "host_pinned": (16, 7, 0, 251)}[form]
    stem = "bjj_schnorr_verify_signer" if schnorr else "bjj_eddsa_verify_signer"
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    results = []
    for fill in (0, 1):
        i3 = [(name, arr, o) for (name, arr, _), o in zip(ins, offs)]
        outs = [("ok", n, offs[3])]
        if form.startswith("dev"):
            a = DeviceArena(i3, outs, fill=fill)
        else:
            a = HostArena(i3, outs, fill=fill, pinned_ctx=gpu_ctx if form == "host_pinned" else None)
        try:
            args = (a.ptr("r"), a.ptr("s"), a.ptr("msg"))
            if form.startswith("dev"):
                rc = getattr(lib, stem + "_dev")(h, base.handle, *args, n, a.ptr("ok"), None)
            else:
                rc = getattr(lib, stem)(h, base.handle, *args, n, a.ptr("ok"))
            assert rc == 0, lib.bjj_last_error()
            gpu_ctx.sync()
            out = a.check()["ok"]
            assert getattr(lib, stem + "_dev")(h, base.handle, *args, 0, a.ptr("ok"), None) == 0
            assert getattr(lib, stem)(h, base.handle, *args, 0, a.ptr("ok")) == 0
            assert getattr(lib, stem)(h, None, *args, n, a.ptr("ok")) == -1
            assert getattr(lib, stem + "_dev")(h, None, *args, n, a.ptr("ok"), None) == -1
            gpu_ctx.sync()
            assert (a.check()["ok"] == out).all()
        finally:
            a.close()
        assert (out == want).all(), (form, fill)
        results.append(out)
    assert (results[0] == results[1]).all()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def test_rejections(gpu_ctx, ctx_w23, tables, data):
    import torch
    import babyjubjub_rs_amd as bjj
    from babyjubjub_rs_amd import _lib
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    n = 65
    d = data("ordinary", False)
    R, S, M = (np.ascontiguousarray(d[k][:n]) for k in ("R", "S", "msg"))
    ok = np.full(n, 0xEE, np.uint8)
    base = tables("gpu_ctx", "ordinary", 4)
    foreign = tables("ctx_w23", "ordinary", 16)
    host = (lib.bjj_eddsa_verify_signer, lib.bjj_schnorr_verify_signer)
    devf = (lib.bjj_eddsa_verify_signer_dev, lib.bjj_schnorr_verify_signer_dev)
    p = (R.ctypes.data, S.ctypes.data, M.ctypes.data)
    for f in host:
        assert f(h, None, *p, n, ok.ctypes.data) == _lib.BJJ_E_INVALID
        assert b"signer is NULL" in lib.bjj_last_error()
        assert f(h, foreign.handle, *p, n, ok.ctypes.data) == _lib.BJJ_E_INVALID          # a base of a second context
        assert b"not a base of this context" in lib.bjj_last_error()
        for j in range(3):
            q = list(p)
            q[j] = None
            assert f(h, base.handle, *q, n, ok.ctypes.data) == _lib.BJJ_E_INVALID
        assert f(h, base.handle, *p, n, None) == _lib.BJJ_E_INVALID
        assert f(h, base.handle, None, None, None, 0, None) == 0                         # n == 0 looks at nothing
    with pytest.raises(bjj.BjjError):
        gpu_ctx.eddsa_verify_signer(foreign, R, S, M)
    gone = gpu_ctx.base(d["rec"], 4)
    stale = gone.handle.value
    gone.close()
    with pytest.raises(bjj.BjjError):                      # the binding refuses a closed base ...
        gone.verify(R, S, M)
    with pytest.raises(bjj.BjjError):
        gone.verify_schnorr(R, S, M)
    for f in host:                                         # ... and the library a handle it does not list
        assert f(h, stale, *p, n, ok.ctypes.data) == _lib.BJJ_E_INVALID
    assert (ok == 0xEE).all()
    dev = torch.device("cuda", 0)
    pad = np.zeros(16, np.uint8)
    d_in = [torch.from_numpy(np.concatenate([a.reshape(-1), pad])).to(dev) for a in (R, S, M)]
    d_ok = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device=dev)
    dp = [t.data_ptr() for t in d_in]
    for f in devf:
        for j in range(3):
            q = list(dp)
            q[j] += 8                                      # misaligned
            assert f(h, base.handle, *q, n, d_ok.data_ptr(), None) == _lib.BJJ_E_INVALID
            q[j] = None
            assert f(h, base.handle, *q, n, d_ok.data_ptr(), None) == _lib.BJJ_E_INVALID
        assert f(h, base.handle, *dp, n, None, None) == _lib.BJJ_E_INVALID
        assert f(h, None, *dp, n, d_ok.data_ptr(), None) == _lib.BJJ_E_INVALID
        assert f(h, stale, *dp, n, d_ok.data_ptr(), None) == _lib.BJJ_E_INVALID
        assert f(h, foreign.handle, *dp, n, d_ok.data_ptr(), None) == _lib.BJJ_E_INVALID
        assert f(h, base.handle, *dp, 0, d_ok.data_ptr(), None) == 0
    gpu_ctx.sync()
    assert bool((d_ok == 0xEE).all())
    # d_ok needs no alignment, as in bjj_eddsa_verify_dev
    lib.bjj_eddsa_verify_signer_dev(h, base.handle, *dp, n, d_ok.data_ptr() + 3, None)
    gpu_ctx.sync()
    got = d_ok.cpu().numpy()
    assert (got[3:3 + n] == d["want"][:n]).all() and (got[:3] == 0xEE).all() and (got[3 + n:] == 0xEE).all()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_afterwards_the_context_is_as_before(gpu_ctx, oracle, tables, data):
    from babyjubjub_rs_amd import workload
    base = tables("gpu_ctx", "order8l", 16)
    d = data("order8l", False)
    assert (base.verify(d["R"], d["S"], d["msg"]) == d["want"]).all()
    assert gpu_ctx.check_table() == 0
    A, R, Sg, msg = workload.make_signatures(oracle.mul_fixed_base, oracle.poseidon5, 64)
    workload.corrupt(A, R, Sg, msg, 64)
    assert (gpu_ctx.eddsa_verify(A, R, Sg, msg) == oracle.verify(A, R, Sg, msg)).all()
    assert base.check() == 0
