"""bjj_mul_bases on the MI355X (include/bjj_hip_bases.h): tables for caller-chosen points and out[i] = sum_j scalars[j][i] * P_j in
one launch.  Expected values come from the C oracle -- mul_var_base of the replicated point per term, folded with point_add (the
reference's mul_scalar and PointProjective::add + affine) -- and, at 65 537 items, from the library's own bjj_mul_var_base +
bjj_point_add; the pure-Python oracle is not used here.  The scalars of every size are a slice of ONE array per test, so the
oracle runs once per base and the sizes share its results."""
import ctypes

import numpy as np
import pytest

from bases_cases import base_windows, scalar_array
from conftest import ints, pack
from memguard import DeviceArena, HostArena

pytestmark = pytest.mark.gpu

Q = 21888242871839275222246405745257275088548364400416034343698204186575808495617
B8 = (5299619240641551281634865583518297030282874472190772894086521144482721001553,
      16950150798460657717958625567821834550301663161624707787222815936182638968203)
WIDTHS = (4, 12, 16)
NMAX = 4097
IDENTITY = pack([(0, 1)]).reshape(1, 64)


def rec(pt):
    return pack([pt]).reshape(1, 64)


def rep(pt_rec, n):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(pt_rec, np.uint8).reshape(1, 64), (n, 64)))


@pytest.fixture(scope="module")
def points(gpu_ctx, oracle, golden):
    """name -> 64-byte record: B8, B8 + T8 (order 8l), the torsion points of order 2, 4, 8, the identity, two seeded k * B8 + T"""
    from babyjubjub_rs_amd import workload as w
    tors = pack([ints(t) for t in golden["gpu_expected"]["torsion_points"]]).reshape(8, 64)   # j * T8
    k = w.random_u256(w.SEED_POINTS ^ 0xBA5E, 2)
    kb = oracle.mul_fixed_base(k)
    p = {"b8": rec(B8), "gen": oracle.point_add(rec(B8), tors[1:2]), "ord2": tors[4:5].copy(), "ord4": tors[2:3].copy(),
         "ord8": tors[1:2].copy(), "identity": tors[0:1].copy(), "k1": oracle.point_add(kb[0:1], tors[3:4]),
         "k2": oracle.point_add(kb[1:2], tors[6:7])}
    assert (p["identity"] == IDENTITY).all() and (p["ord2"] == rec((0, Q - 1))).all()
    return p


@pytest.fixture(scope="module")
def S(points):
    """the scalars of the module: [0] the directed ones + seeded random ones, [1..7] seeded random arrays for further bases"""
    arrs = [scalar_array(NMAX, WIDTHS, 0x5CA1A)] + [scalar_array(NMAX, (), 0x5CA1A + j)[::-1].copy() for j in range(1, 8)]
    for a in arrs:
        a.setflags(write=False)
    return arrs


@pytest.fixture(scope="module")
def products(oracle, points, S):
    """(point name, scalar array index) -> the oracle's k * P for every scalar of that array; filled on demand, never rewritten"""
    cache = {}

    def get(name, j=0):
        if (name, j) not in cache:
            neg = name.startswith("-")
            p = points[name.lstrip("-")]
            if neg:
                x, y = ints_of(p)
                p = rec(((Q - x) % Q, y))
            v = oracle.mul_var_base(rep(p, NMAX), S[j])
            v.setflags(write=False)
            cache[(name, j)] = v
        return cache[(name, j)]
    return get


def ints_of(p):
    b = np.asarray(p, np.uint8).tobytes()
    return int.from_bytes(b[:32], "little"), int.from_bytes(b[32:64], "little")


@pytest.fixture(scope="module")
def tables(gpu_ctx, points):
    """(point name, W) -> FixedBase, created on first use and closed with the module"""
    made = {}

    def get(name, W):
        if (name, W) not in made:
            p = points[name.lstrip("-")]
            if name.startswith("-"):
                x, y = ints_of(p)
                p = rec(((Q - x) % Q, y))
            made[(name, W)] = gpu_ctx.base(p, W)
        return made[(name, W)]
    yield get
    for b in made.values():
        b.close()


def fold(add, terms):
    acc = terms[0]
    for t in terms[1:]:
        acc = add(acc, t)
    return acc


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", WIDTHS)
def test_single_base_against_oracle(gpu_ctx, points, tables, products, S, W):
    names = sorted(points) + ["unreduced"]
    for name in names:
        if name == "unreduced":                       # x + r in the record: the table of the reduced point
            x, y = ints_of(points["k1"])
            base, want = gpu_ctx.base(rec((x + Q, y)), W), products("k1")
        else:
            base, want = tables(name, W), products(name)
        try:
            for n, off in ((1, 10), (1, 0), (63, 0), (64, 3), (65, 0), (NMAX, 0)):
                got = base.mul(S[0][off:off + n])
                bad = np.nonzero((got != want[off:off + n]).any(axis=1))[0]
                assert bad.size == 0, (name, W, n, off, bad[:8].tolist())
        finally:
            if name == "unreduced":
                base.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["gpu_ctx", "ctx_w23"])
def test_null_base_is_mul_fixed_base(request, S, which):
    ctx = request.getfixturevalue(which)
    got = ctx.mul_bases([None], [S[0]])
    assert got.shape == (NMAX, 64) and (got == ctx.mul_fixed_base(S[0])).all()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
COMBOS = {
    "null_first": [None, ("gen", 16)],
    "null_last": [("gen", 12), None],
    "same_twice": [("k1", 4), ("k1", 4), ("ord8", 16)],
    "eight": [None, ("gen", 4), ("gen", 12), ("gen", 16), ("k1", 16), ("k2", 12), ("ord2", 4), ("identity", 16)],
}


def _bases(tables, combo):
    return [None if b is None else tables(*b) for b in combo]


@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_several_bases(gpu_ctx, oracle, points, tables, products, S, combo):
    spec = COMBOS[combo]
    bases = _bases(tables, spec)
    assert combo != "same_twice" or bases[0] is bases[1]
    terms = [products("b8" if b is None else b[0], j) for j, b in enumerate(spec)]
    want = fold(oracle.point_add, terms)
    for n in (65, NMAX):
        got = gpu_ctx.mul_bases(bases, [S[j][:n] for j in range(len(spec))])
        bad = np.nonzero((got != want[:n]).any(axis=1))[0]
        assert bad.size == 0, (combo, n, bad[:8].tolist())


def test_p_and_minus_p_cancel(gpu_ctx, tables, S):
    for n in (65, NMAX):
        got = gpu_ctx.mul_bases([tables("k1", 16), tables("-k1", 12)], [S[0][:n], S[0][:n]])
        assert (got == IDENTITY).all(), n


def test_several_bases_65537_against_the_gpu_composition(gpu_ctx, points, tables):
    n = 65537
    spec = COMBOS["eight"]
    sc = [scalar_array(n, WIDTHS, 0xB16 + j) for j in range(len(spec))]
    got = gpu_ctx.mul_bases(_bases(tables, spec), sc)
    terms = [gpu_ctx.mul_var_base(rep(points["b8" if b is None else b[0]], n), sc[j]) for j, b in enumerate(spec)]
    want = fold(lambda p, q: gpu_ctx.point_add(p, q), terms)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, bad[:8].tolist()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_base_check_and_info(gpu_ctx, points, tables):
    for W in (4, 16):
        for name in sorted(points):
            b = tables(name, W)
            assert b.check() == 0, (name, W)
            nwin = -(-255 // W)
            assert b.info() == (W, nwin, ((1 << (W - 1)) + 1) * nwin * 128) and nwin == base_windows(W), (name, W)
    d = gpu_ctx.base(points["gen"])                   # window_bits = 0: 16 bits
    try:
        assert d.info() == (16, 16, ((1 << 15) + 1) * 16 * 128)
    finally:
        d.close()


@pytest.mark.parametrize("W", [5, 15, 17, 20])
def test_width_sweep_against_oracle(gpu_ctx, oracle, points, W):
    """widths that divide 255 (5, 15, 17: the top window is a full W bits wide, of which a scalar below 8l < 2^254 fills W - 1) and
    one above every other caller's table in the suite (20: 13 windows of 2^19 + 1 entries, 0.87 GB); tests/test_bases_host.py
    holds the recoding argument for every width in plain integers"""
    n = 257
    nwin = -(-255 // W)
    assert nwin == base_windows(W) and (255 % W == 0) == (W != 20)
    sc = scalar_array(n, (W,), 0x51DE + W)
    want = oracle.mul_var_base(rep(points["k1"], n), sc)
    base = gpu_ctx.base(points["k1"], W)
    try:
        assert base.info() == (W, nwin, ((1 << (W - 1)) + 1) * nwin * 128)
        assert base.check() == 0
        got = base.mul(sc)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert got.shape == (n, 64) and bad.size == 0, (W, bad[:8].tolist())
    finally:
        base.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def test_rejections(gpu_ctx, points, tables, S):
    import torch
    from babyjubjub_rs_amd import _lib
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    slot = ctypes.c_void_p(0x1234)
    off = points["gen"].copy().reshape(-1)
    off[3] ^= 0x10                                    # one bit of x
    assert lib.bjj_base_create(h, off.ctypes.data, 16, ctypes.byref(slot)) == _lib.BJJ_E_INVALID and slot.value == 0x1234
    assert b"not on the curve" in lib.bjj_last_error()
    good = points["gen"].reshape(-1)
    for W in (3, 29, -1, 1):
        assert lib.bjj_base_create(h, good.ctypes.data, W, ctypes.byref(slot)) == _lib.BJJ_E_INVALID and slot.value == 0x1234, W
    base = tables("gen", 4)
    n = 65
    sc = np.ascontiguousarray(S[0][:n])
    out = np.full(n * 64, 0xEE, np.uint8)
    hb = (ctypes.c_void_p * 9)(*([base.handle.value] * 9))
    hs = (ctypes.c_void_p * 9)(*([sc.ctypes.data] * 9))
    for t in (0, 9, -1):
        assert lib.bjj_mul_bases(h, hb, t, hs, n, out.ctypes.data) == _lib.BJJ_E_INVALID, t
    hs_null = (ctypes.c_void_p * 2)(sc.ctypes.data, None)
    assert lib.bjj_mul_bases(h, hb, 2, hs_null, n, out.ctypes.data) == _lib.BJJ_E_INVALID
    assert lib.bjj_mul_bases(h, hb, 2, hs_null, 0, out.ctypes.data) == 0          # n == 0: nothing is looked at
    assert lib.bjj_mul_bases(h, hb, 1, hs, 0, out.ctypes.data) == 0
    assert (out == 0xEE).all()
    dev = torch.device("cuda", 0)
    d_sc = torch.from_numpy(np.concatenate([sc.reshape(-1), np.zeros(16, np.uint8)])).to(dev)
    d_out = torch.full((n * 64 + 16,), 0xEE, dtype=torch.uint8, device=dev)
    ds = (ctypes.c_void_p * 9)(*([d_sc.data_ptr()] * 9))
    for t in (0, 9):
        assert lib.bjj_mul_bases_dev(h, hb, t, ds, n, d_out.data_ptr(), None) == _lib.BJJ_E_INVALID, t
    ds_mis = (ctypes.c_void_p * 1)(d_sc.data_ptr() + 8)
    assert lib.bjj_mul_bases_dev(h, hb, 1, ds_mis, n, d_out.data_ptr(), None) == _lib.BJJ_E_INVALID
    assert lib.bjj_mul_bases_dev(h, hb, 1, ds, n, d_out.data_ptr() + 8, None) == _lib.BJJ_E_INVALID
    assert lib.bjj_mul_bases_dev(h, hb, 1, (ctypes.c_void_p * 1)(None), n, d_out.data_ptr(), None) == _lib.BJJ_E_INVALID
    assert lib.bjj_mul_bases_dev(h, hb, 1, ds, 0, d_out.data_ptr(), None) == 0
    gpu_ctx.sync()
    assert bool((d_out == 0xEE).all())
    import babyjubjub_rs_amd as bjj
    gone = gpu_ctx.base(points["ord4"], 4)
    stale = (ctypes.c_void_p * 1)(gone.handle.value)
    gone.close()
    with pytest.raises(bjj.BjjError):                 # the binding refuses a closed base ...
        gpu_ctx.mul_bases([gone], [sc])
    assert lib.bjj_mul_bases(h, stale, 1, hs, n, out.ctypes.data) == _lib.BJJ_E_INVALID   # ... and the library a handle it does not list
    assert lib.bjj_base_free(h, stale[0]) == _lib.BJJ_E_INVALID
    assert (out == 0xEE).all()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_forms_agree(gpu_ctx, oracle, tables, products, S):
    import torch
    n = NMAX
    bases = [tables("gen", 16), tables("k2", 12)]
    want = oracle.point_add(products("gen", 0), products("k2", 1))
    pageable = gpu_ctx.mul_bases(bases, [S[0], S[1]])
    assert (pageable == want).all()
    pins = [gpu_ctx.host_empty(n * 32), gpu_ctx.host_empty(n * 32), gpu_ctx.host_empty(n * 64)]
    try:
        pins[0][:] = S[0].reshape(-1)
        pins[1][:] = S[1].reshape(-1)
        pins[2][:] = 0xEE
        assert all(gpu_ctx.host_is_pinned(p) for p in pins)
        hb = (ctypes.c_void_p * 2)(bases[0].handle.value, bases[1].handle.value)
        hs = (ctypes.c_void_p * 2)(pins[0].ctypes.data, pins[1].ctypes.data)
        assert gpu_ctx.lib.bjj_mul_bases(gpu_ctx.handle, hb, 2, hs, n, pins[2].ctypes.data) == 0, gpu_ctx.lib.bjj_last_error()
        assert (pins[2].reshape(n, 64) == pageable).all()
    finally:
        for p in pins:
            gpu_ctx.host_free(p)
    dev = torch.device("cuda", 0)
    d_s = [torch.from_numpy(S[j].reshape(-1).copy()).to(dev) for j in range(2)]
    d_out = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    gpu_ctx.mul_bases_dev(bases, [t.data_ptr() for t in d_s], n, d_out.data_ptr())
    gpu_ctx.sync()
    assert (d_out.cpu().numpy().reshape(n, 64) == pageable).all()


def test_two_streams_at_once(gpu_ctx, oracle, tables, products, S):
    import torch
    dev = torch.device("cuda", 0)
    n = NMAX
    cases = [([tables("gen", 16), None], [0, 1], oracle.point_add(products("gen", 0), products("b8", 1))),
             ([tables("k1", 12), tables("ord8", 16)], [2, 3], oracle.point_add(products("k1", 2), products("ord8", 3)))]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    d_s = {j: torch.from_numpy(S[j].reshape(-1).copy()).to(dev) for j in range(4)}
    outs = [torch.zeros(n * 64, dtype=torch.uint8, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    for rep_ in range(3):
        for s, (bases, idx, _) in enumerate(cases):
            gpu_ctx.mul_bases_dev(bases, [d_s[j].data_ptr() for j in idx], n, outs[s].data_ptr(), stream=streams[s].cuda_stream)
        gpu_ctx.sync()
        for s in range(2):
            assert (outs[s].cpu().numpy().reshape(n, 64) == cases[s][2]).all(), (rep_, s)
            outs[s].zero_()
        torch.cuda.synchronize()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_lifetime(oracle, points, products, S):
    import babyjubjub_rs_amd as bjj
    from babyjubjub_rs_amd import workload
    ctx = bjj.Context(0, 16)
    try:
        before = ctx.info()
        n = 257
        b = ctx.base(points["gen"], 12)
        assert (b.mul(S[0][:n]) == products("gen")[:n]).all()
        b.close()
        assert b.handle is None
        b = ctx.base(points["gen"], 5)                   # again, at another width, on the same context
        assert b.info()[:2] == (5, 51) and b.check() == 0
        assert (b.mul(S[0][:n]) == products("gen")[:n]).all()
        keep = ctx.base(points["k1"], 16)
        assert (ctx.mul_bases([None, keep, b], [S[1][:n], S[0][:n], S[0][:n]])
                == fold(oracle.point_add, [products("b8", 1)[:n], products("k1")[:n], products("gen")[:n]])).all()
        b.close()
        after = ctx.info()
        assert (after.window_bits, after.n_windows, after.table_bytes) == (before.window_bits, before.n_windows, before.table_bytes)
        assert ctx.check_table() == 0
        sc = workload.scalars_254(256)
        assert (ctx.mul_fixed_base(sc) == oracle.mul_fixed_base(sc)).all()
        A, R, Sg, msg = workload.make_signatures(oracle.mul_fixed_base, oracle.poseidon5, 64)
        workload.corrupt(A, R, Sg, msg, 64)
        assert (ctx.eddsa_verify(A, R, Sg, msg) == oracle.verify(A, R, Sg, msg)).all()
        assert keep.handle is not None                   # still live: the context releases it
    finally:
        ctx.close()
    assert keep.handle is None or ctx.handle is None
    ctx2 = bjj.Context(0, 16)                            # the device is as usable as before
    try:
        assert (ctx2.base(points["ord4"], 4).mul(S[0][:65]) == products("ord4")[:65]).all()
        raw = ctypes.c_void_p()                          # a handle the binding does not know of: bjj_free itself releases it
        assert ctx2.lib.bjj_base_create(ctx2.handle, points["gen"].ctypes.data, 12, ctypes.byref(raw)) == 0 and raw.value
    finally:
        ctx2.close()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["dev_all_0", "dev_mixed", "host_pageable", "host_pinned"])
def test_memory_contract(gpu_ctx, oracle, tables, products, S, form):
    """n = 65, t = 3 under the guarded arenas: nothing outside out[0 : n * 64] is written, the inputs are unchanged, and the result
    does not depend on what the output region held"""
    n = 65
    bases = [tables("gen", 12), None, tables("ord2", 4)]
    want = fold(oracle.point_add, [products("gen", 0)[:n], products("b8", 1)[:n], products("ord2", 2)[:n]])
    hb = (ctypes.c_void_p * 3)(bases[0].handle.value, None, bases[2].handle.value)
    ins = [("scalars0", S[0][:n], 0), ("scalars1", S[1][:n], 0), ("scalars2", S[2][:n], 0)]
    offs = {"dev_all_0": (0, 0, 0, 0), "dev_mixed": (16, 48, 240, 112), "host_pageable": (1, 8, 33, 100), "host_pinned": (16, 7, 0, 250)}[form]
    results = []
    for fill in (0, 1):
        i3 = [(name, arr, o) for (name, arr, _), o in zip(ins, offs)]
        outs = [("out_xy", n * 64, offs[3])]
        if form.startswith("dev"):
            a = DeviceArena(i3, outs, fill=fill)
        else:
            a = HostArena(i3, outs, fill=fill, pinned_ctx=gpu_ctx if form == "host_pinned" else None)
        try:
            hs = (ctypes.c_void_p * 3)(a.ptr("scalars0"), a.ptr("scalars1"), a.ptr("scalars2"))
            if form.startswith("dev"):
                rc = gpu_ctx.lib.bjj_mul_bases_dev(gpu_ctx.handle, hb, 3, hs, n, a.ptr("out_xy"), None)
            else:
                rc = gpu_ctx.lib.bjj_mul_bases(gpu_ctx.handle, hb, 3, hs, n, a.ptr("out_xy"))
            assert rc == 0, gpu_ctx.lib.bjj_last_error()
            gpu_ctx.sync()
            out = a.check()["out_xy"]
            # n == 0 and a rejected call leave the output as it is
            assert gpu_ctx.lib.bjj_mul_bases_dev(gpu_ctx.handle, hb, 3, hs, 0, a.ptr("out_xy"), None) == 0
            assert gpu_ctx.lib.bjj_mul_bases(gpu_ctx.handle, hb, 9, hs, n, a.ptr("out_xy")) == -1
            gpu_ctx.sync()
            assert (a.check()["out_xy"] == out).all()
        finally:
            a.close()
        assert (out.reshape(n, 64) == want).all(), (form, fill)
        results.append(out)
    assert (results[0] == results[1]).all()
