"""bjj_dlog on the GPU (include/bjj_hip_dlog.h): tables of 4, 8 and 12 baby bits for B8 and of 8 for a point of order 8l, the
directed and random cases of tests/dlog_cases.py through the host form at four range widths and five batch sizes, the _dev form on
the context's stream and on two caller streams at once, pinned and pageable arrays, guarded memory, a call cut into several
launches, the rejections, and an ElGamal round trip.  The test chooses m; P = m * G comes from the C oracle."""
import ctypes
import os

import numpy as np
import pytest

import dlog_cases as dc
from conftest import ints, pack, unpack
from memguard import DeviceArena, HostArena

pytestmark = pytest.mark.gpu

E_INVALID = -1
NMAX = 1000
SIZES = (1, 63, 64, 65, NMAX)
TABLES = [("b8", 4), ("b8", 8), ("b8", 12), ("order_8l", 8)]
B8 = (5299619240641551281634865583518297030282874472190772894086521144482721001553,
      16950150798460657717958625567821834550301663161624707787222815936182638968203)


def ranges_of(b):
    return [b - 2, b, b + 1, b + 8]


class ByteDeviceArena(DeviceArena):
    """the device arena with byte-granular offsets: d_ok may sit at any address"""
    max_off_step = 1


@pytest.fixture(scope="module")
def points(oracle, golden):
    """the bases and, per table, the interleaved cases as (records (n, 64) uint8, cases) -- computed once, by the C oracle"""
    from babyjubjub_rs_amd import _lib
    assert _lib.BJJ_E_INVALID == E_INVALID
    tors = [ints(t) for t in golden["gpu_expected"]["torsion_points"]]

    def mul(P, ks):
        out = oracle.mul_var_base(np.tile(pack([P]), len(ks)), pack([k for k in ks]))
        return unpack(out, 2)

    def add(p, q):
        return unpack(oracle.point_add(pack([p]), pack([q])), 2)[0]
    bases = {"b8": B8, "order_8l": add(mul(B8, [0x1234567])[0], tors[1])}
    assert mul(bases["order_8l"], [dc.SUBORDER])[0] != (0, 1) and mul(bases["order_8l"], [dc.ORDER])[0] == (0, 1)
    out = {"bases": bases, "torsion": tors, "mul": mul, "add": add}
    for name, b in TABLES:
        n_dir = len(dc.build(mul, add, bases[name], b, ranges_of(b), tors[1], 1, n_random=0))
        cases = dc.interleave(dc.build(mul, add, bases[name], b, ranges_of(b), tors[1], 0xD106 + b, n_random=NMAX - n_dir))
        assert len(cases) == NMAX
        out[(name, b)] = (pack([rec for rec, _ in cases]).reshape(NMAX, 64), cases)
    return out


@pytest.fixture(scope="module")
def tables(gpu_ctx, points):
    made = {}

    def get(name, b):
        if (name, b) not in made:
            made[(name, b)] = gpu_ctx.dlog_table(None if name == "b8" else points["bases"][name], b)
        return made[(name, b)]
    yield get
    for t in made.values():
        t.close()


def _want(cases, n, rb):
    m, ok = dc.expected(cases[:n], rb)
    return np.array(m, dtype=np.uint64), np.array(ok, dtype=np.uint8)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,b", TABLES)
def test_tables_are_sound(tables, points, name, b):
    t = tables(name, b)
    assert t.info() == (b, (1 << b) + 1, 1 << (b + 5))
    assert t.check() == 0
    assert t.base() == points["bases"][name]
    assert t.max_range_bits() == b + 17


def test_the_default_table_and_a_record_with_x_beyond_r(gpu_ctx, points):
    """baby_bits = 0 is the documented default, 24 bits: 2^24 + 1 entries in 2^29 bytes.  A base given as (x + r, y) is the base (x, y)."""
    recs, cases = points[("b8", 12)]
    t = gpu_ctx.dlog_table()
    try:
        assert t.info() == (24, (1 << 24) + 1, 1 << 29) and t.max_range_bits() == 41 and t.base() == B8
        m, ok = t.dlog(recs[:65], 20)
        wm, wok = _want(cases, 65, 20)
        assert (m == wm).all() and (ok == wok).all()
    finally:
        t.close()
    G = points["bases"]["order_8l"]
    recs, cases = points[("order_8l", 8)]
    t = gpu_ctx.dlog_table((G[0] + dc.Q, G[1]), 8)
    try:
        assert t.base() == G and t.check() == 0
        m, ok = t.dlog(recs[:65], 16)
        wm, wok = _want(cases, 65, 16)
        assert (m == wm).all() and (ok == wok).all()
    finally:
        t.close()


@pytest.mark.parametrize("name,b", TABLES)
def test_against_the_oracle(tables, points, name, b):
    t = tables(name, b)
    recs, cases = points[(name, b)]
    for rb in ranges_of(b):
        for n in SIZES:
            m, ok = t.dlog(recs[:n], rb)
            wm, wok = _want(cases, n, rb)
            bad = [(i, int(ok[i]), int(m[i]), int(wok[i]), int(wm[i])) for i in np.nonzero((ok != wok) | (m != wm))[0][:8]]
            assert not bad, (name, b, rb, n, bad)
    assert set(_want(cases, NMAX, b + 8)[1]) == {0, 1, 2}


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
def test_forms_agree(gpu_ctx, tables, points):
    import torch
    t = tables("b8", 8)
    recs, cases = points[("b8", 8)]
    n, rb = NMAX, 16
    pm, pok = t.dlog(recs, rb)
    wm, wok = _want(cases, n, rb)
    assert (pm == wm).all() and (pok == wok).all()
    pins = [gpu_ctx.host_empty(n * 64), gpu_ctx.host_empty(n * 8), gpu_ctx.host_empty(n)]
    try:
        pins[0][:] = recs.reshape(-1)
        pins[1][:] = 0xEE
        pins[2][:] = 0xEE
        assert all(gpu_ctx.host_is_pinned(p) for p in pins)
        rc = gpu_ctx.lib.bjj_dlog(gpu_ctx.handle, t.handle, pins[0].ctypes.data, n, rb, pins[1].ctypes.data, pins[2].ctypes.data)
        assert rc == 0, gpu_ctx.lib.bjj_last_error()
        assert bytes(pins[1]) == pm.tobytes() and bytes(pins[2]) == pok.tobytes()
    finally:
        for p in pins:
            gpu_ctx.host_free(p)
    dev = torch.device("cuda", 0)
    d_pts = torch.from_numpy(recs.reshape(-1).copy()).to(dev)
    d_m = torch.full((n * 8,), 0xEE, dtype=torch.uint8, device=dev)
    d_ok = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    gpu_ctx.dlog_dev(t, d_pts.data_ptr(), n, rb, d_m.data_ptr(), d_ok.data_ptr())
    gpu_ctx.sync()
    assert d_m.cpu().numpy().tobytes() == pm.tobytes() and d_ok.cpu().numpy().tobytes() == pok.tobytes()


def test_two_streams_at_once(gpu_ctx, tables, points):
    import torch
    dev = torch.device("cuda", 0)
    n = NMAX
    jobs = [(tables("b8", 12), points[("b8", 12)], 20), (tables("order_8l", 8), points[("order_8l", 8)], 16)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    d_pts = [torch.from_numpy(recs.reshape(-1).copy()).to(dev) for _, (recs, _), _ in jobs]
    d_m = [torch.full((n * 8,), 0xEE, dtype=torch.uint8, device=dev) for _ in range(2)]
    d_ok = [torch.full((n,), 0xEE, dtype=torch.uint8, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    for rep_ in range(3):
        for s, (t, _, rb) in enumerate(jobs):
            gpu_ctx.dlog_dev(t, d_pts[s].data_ptr(), n, rb, d_m[s].data_ptr(), d_ok[s].data_ptr(), stream=streams[s].cuda_stream)
        gpu_ctx.sync()
        for s, (t, (_, cases), rb) in enumerate(jobs):
            wm, wok = _want(cases, n, rb)
            assert d_m[s].cpu().numpy().tobytes() == wm.tobytes() and d_ok[s].cpu().numpy().tobytes() == wok.tobytes(), (rep_, s)
            d_m[s].fill_(0xEE)
            d_ok[s].fill_(0xEE)
        torch.cuda.synchronize()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["dev_all_0", "dev_mixed", "host_pageable", "host_pinned"])
def test_memory_contract(gpu_ctx, tables, points, form):
    """n = 65 under the guarded arenas: nothing outside out_m[0 : n] and ok[0 : n] is written, the inputs are unchanged, the result
    does not depend on what the outputs held, and n == 0 and a rejected call leave the outputs as they were"""
    n, rb = 65, 12
    t = tables("b8", 8)
    recs, cases = points[("b8", 8)]
    wm, wok = _want(cases, n, rb)
    offs = {"dev_all_0": (0, 0, 0), "dev_mixed": (48, 16, 113), "host_pageable": (1, 8, 100), "host_pinned": (16, 0, 251)}[form]
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    results = []
    for fill in (0, 1):
        ins = [("pts", recs[:n], offs[0])]
        outs = [("m", n * 8, offs[1]), ("ok", n, offs[2])]
        if form.startswith("dev"):
            a = (ByteDeviceArena if form == "dev_mixed" else DeviceArena)(ins, outs, fill=fill)
        else:
            a = HostArena(ins, outs, fill=fill, pinned_ctx=gpu_ctx if form == "host_pinned" else None)
        try:
            def call(table, count, bits):
                if form.startswith("dev"):
                    return lib.bjj_dlog_dev(h, table, a.ptr("pts"), count, bits, a.ptr("m"), a.ptr("ok"), None)
                return lib.bjj_dlog(h, table, a.ptr("pts"), count, bits, a.ptr("m"), a.ptr("ok"))
            assert call(t.handle, n, rb) == 0, lib.bjj_last_error()
            gpu_ctx.sync()
            out = a.check()
            assert call(t.handle, 0, rb) == 0
            assert call(None, n, rb) == E_INVALID
            assert call(t.handle, n, 0) == E_INVALID
            assert call(t.handle, n, 8 + 18) == E_INVALID               # one beyond baby_bits + 1 + 16
            gpu_ctx.sync()
            again = a.check()
            assert (again["m"] == out["m"]).all() and (again["ok"] == out["ok"]).all()
        finally:
            a.close()
        assert out["m"].tobytes() == wm.tobytes() and out["ok"].tobytes() == wok.tobytes(), (form, fill)
        results.append(out)
    assert results[0]["m"].tobytes() == results[1]["m"].tobytes()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_a_call_cut_into_several_launches(points):
    """BJJ_DLOG_LAUNCH_STEPS, read at bjj_init: a context whose launches perform at most 4096 giant steps cuts n = 1000 items x 128
    steps into 16 chunks of 64 items x 2 launches of 64 steps; one with 64 into chunks of one item.  Same bytes as the uncut call."""
    import babyjubjub_rs_amd as bjj
    recs, cases = points[("b8", 8)]
    results = {}
    for bound, n, rb in ((None, NMAX, 16), ("4096", NMAX, 16), ("64", 65, 16), ("1000", NMAX, 12)):
        old = os.environ.get("BJJ_DLOG_LAUNCH_STEPS")
        if bound is None:
            os.environ.pop("BJJ_DLOG_LAUNCH_STEPS", None)
        else:
            os.environ["BJJ_DLOG_LAUNCH_STEPS"] = bound
        try:
            ctx = bjj.Context(0, 16)
        finally:
            if old is None:
                os.environ.pop("BJJ_DLOG_LAUNCH_STEPS", None)
            else:
                os.environ["BJJ_DLOG_LAUNCH_STEPS"] = old
        try:
            t = ctx.dlog_table(None, 8)
            m, ok = t.dlog(recs[:n], rb)
            wm, wok = _want(cases, n, rb)
            assert (m == wm).all() and (ok == wok).all(), bound
            results[bound] = (m.tobytes(), ok.tobytes())
        finally:
            ctx.close()
    assert results[None] == results["4096"]


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def test_create_rejections(gpu_ctx, points):
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    out = ctypes.c_void_p(0x77)
    tors = points["torsion"]

    def create(point, b):
        rec = None if point is None else pack([point])
        return lib.bjj_dlog_table_create(h, None if rec is None else rec.ctypes.data, b, ctypes.byref(out))
    assert create((B8[0], (B8[1] + 1) % dc.Q), 4) == E_INVALID and b"not on the curve" in lib.bjj_last_error()
    assert create((0, 0), 4) == E_INVALID
    assert create((0, 1), 4) == E_INVALID and b"identity" in lib.bjj_last_error()      # the identity
    for T in tors:                                                                      # every point of order <= 8
        assert create(T, 4) == E_INVALID, T
    for b in (3, 29, -1, 1):
        assert create(None, b) == E_INVALID and b"baby_bits" in lib.bjj_last_error(), b
        assert create(B8, b) == E_INVALID
    assert lib.bjj_dlog_table_create(h, None, 4, None) == E_INVALID
    assert out.value == 0x77
    # a point of order 2l is a base: 8 G is not the identity
    G2 = points["add"](points["mul"](B8, [77])[0], tors[4])
    assert create(G2, 4) == 0 and out.value not in (0, 0x77)
    assert lib.bjj_dlog_table_free(h, out) == 0
    assert lib.bjj_dlog_table_free(h, out) == E_INVALID                                # freed: no longer a table of this context
    assert lib.bjj_dlog_table_free(h, None) == 0


def test_call_rejections(gpu_ctx, ctx_w23, tables, points):
    import torch
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    t = tables("b8", 8)
    recs, cases = points[("b8", 8)]
    n = 16
    m = np.full(n, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    ok = np.full(n, 0xEE, dtype=np.uint8)
    p = np.ascontiguousarray(recs[:n])
    for rb in (0, -3, 26, 46, 64):                                                      # the cap of an 8-bit table is 25
        assert lib.bjj_dlog(h, t.handle, p.ctypes.data, n, rb, m.ctypes.data, ok.ctypes.data) == E_INVALID, rb
        assert b"range_bits" in lib.bjj_last_error()
    assert lib.bjj_dlog(h, t.handle, p.ctypes.data, n, 25, m.ctypes.data, None) == E_INVALID
    assert lib.bjj_dlog(h, t.handle, p.ctypes.data, n, 25, None, ok.ctypes.data) == E_INVALID
    assert lib.bjj_dlog(h, t.handle, None, n, 25, m.ctypes.data, ok.ctypes.data) == E_INVALID
    assert lib.bjj_dlog(h, None, p.ctypes.data, n, 12, m.ctypes.data, ok.ctypes.data) == E_INVALID
    # a NULL table or a bad range_bits is refused whatever else is wrong with the call
    assert lib.bjj_dlog(h, None, None, n, 0, None, None) == E_INVALID and b"table is NULL" in lib.bjj_last_error()
    assert lib.bjj_dlog_dev(h, None, 0, n, 12, 0, 0, None) == E_INVALID and b"table is NULL" in lib.bjj_last_error()
    # a table of another context
    assert lib.bjj_dlog(ctx_w23.handle, t.handle, p.ctypes.data, n, 12, m.ctypes.data, ok.ctypes.data) == E_INVALID
    assert b"of this context" in lib.bjj_last_error()
    bad = ctypes.c_uint64(7)
    assert lib.bjj_dlog_table_check(ctx_w23.handle, t.handle, ctypes.byref(bad)) == E_INVALID and bad.value == 7
    assert lib.bjj_dlog_table_free(ctx_w23.handle, t.handle) == E_INVALID
    assert (m == 0xEEEEEEEEEEEEEEEE).all() and (ok == 0xEE).all()
    # the device form: misaligned or NULL pointers
    dev = torch.device("cuda", 0)
    d_pts = torch.from_numpy(np.concatenate([p.reshape(-1), np.zeros(64, np.uint8)])).to(dev)
    d_m = torch.full((n * 8 + 64,), 0xEE, dtype=torch.uint8, device=dev)
    d_ok = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device=dev)
    for args in ((d_pts.data_ptr() + 8, d_m.data_ptr(), d_ok.data_ptr()), (d_pts.data_ptr(), d_m.data_ptr() + 8, d_ok.data_ptr()),
                 (0, d_m.data_ptr(), d_ok.data_ptr()), (d_pts.data_ptr(), 0, d_ok.data_ptr()), (d_pts.data_ptr(), d_m.data_ptr(), 0)):
        assert lib.bjj_dlog_dev(h, t.handle, args[0], n, 12, args[1], args[2], None) == E_INVALID, args
    assert lib.bjj_dlog_dev(h, t.handle, d_pts.data_ptr(), n, 26, d_m.data_ptr(), d_ok.data_ptr(), None) == E_INVALID
    gpu_ctx.sync()
    assert (d_m.cpu().numpy() == 0xEE).all() and (d_ok.cpu().numpy() == 0xEE).all()
    # d_ok at an odd address is fine, and the widest range of the table works: 2^16 giant steps for the items that are not found,
    # which the per-item cap of a launch cuts into 128 launches of 512
    assert lib.bjj_dlog_dev(h, t.handle, d_pts.data_ptr(), 2, 25, d_m.data_ptr(), d_ok.data_ptr() + 3, None) == 0
    gpu_ctx.sync()
    wm, wok = _want(cases, 2, 25)
    got = d_ok.cpu().numpy()
    assert (got[3:5] == wok).all() and (got[:3] == 0xEE).all() and (got[5:] == 0xEE).all()
    assert d_m.cpu().numpy()[:16].tobytes() == wm.tobytes()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_elgamal_round_trip(gpu_ctx, tables):
    rng = np.random.default_rng(0xE16A)
    n = 500
    sk = int.from_bytes(rng.bytes(31), "little") % dc.SUBORDER
    ms = [int(v) for v in rng.integers(0, 1 << 16, n)]
    ms[:4] = [0, 1, (1 << 16) - 1, 1 << 15]
    rs = [int.from_bytes(rng.bytes(31), "little") for _ in range(n)]
    pk = tuple(unpack(gpu_ctx.mul_fixed_base(pack([sk])), 2)[0])
    base = gpu_ctx.base(pk, 8)
    try:
        c1 = gpu_ctx.mul_fixed_base(pack(rs))
        c2 = gpu_ctx.mul_bases([None, base], [pack(ms), pack(rs)])
    finally:
        base.close()
    t = tables("b8", 8)
    m, ok = gpu_ctx.elgamal_decrypt(t, sk, c1, c2, 16)
    assert (ok == 1).all() and [int(v) for v in m] == ms
    from babyjubjub_rs_amd import api
    edge = [(0, 1), (1, 5), (dc.Q - 1, 7), (1 << 32, 0), ((1 << 224) - 1, 9)]
    assert unpack(api._negate_x(pack(edge).reshape(-1, 64)), 2) == [((dc.Q - x) % dc.Q, y) for x, y in edge]
    m, ok = gpu_ctx.elgamal_decrypt(t, sk + 1, c1, c2, 16)
    assert (ok == 0).all() and (m == np.uint64(dc.UINT64_MAX)).all()
