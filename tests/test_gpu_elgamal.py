"""bjj_elgamal_encrypt on the MI355X (include/bjj_hip_elgamal.h): c1 = A1 + r G, c2 = A2 + m G + r PK in one launch.  Expected values
come from the C oracle -- mul_var_base of the replicated point per term, folded with point_add, as tests/test_gpu_bases.py builds
them -- and from the library's own composition (bjj_mul_bases twice, bjj_point_add twice); the pure-Python oracle is not used here.
The scalars of every size are slices of ONE r array and ONE m array, so the oracle runs once per term and the sizes share it."""
import ctypes

import numpy as np
import pytest

from bases_cases import L, scalar_array
from conftest import ints, pack

pytestmark = pytest.mark.gpu

Q = 21888242871839275222246405745257275088548364400416034343698204186575808495617
B8 = (5299619240641551281634865583518297030282874472190772894086521144482721001553,
      16950150798460657717958625567821834550301663161624707787222815936182638968203)
NMAX = 1025          # the workgroup is 512 lanes: 513 and 1025 cross a workgroup and leave a ragged wave
WIDTHS = (4, 5, 12, 13, 16, 23, 28)     # every table width of this module, the two contexts' included
M64 = (1 << 64) - 1
SIZES = ((1, 0), (1, 10), (63, 0), (64, 3), (65, 0), (513, 0), (1025, 0))
# (g, pk width): g = None is the context's B8 table, otherwise the table of `gen` at that width
COMBOS = {"null_w12": (None, 12), "null_w4": (None, 4), "g16_w12": (16, 12), "g5_w13": (5, 13)}
PKS = ("sub", "full", "ord8")


def rec(pt):
    return pack([pt]).reshape(1, 64)


def rep(pt_rec, n):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(pt_rec, np.uint8).reshape(1, 64), (n, 64)))


def m_pattern(W, digit):
    n = -(-65 // W)
    while True:
        v = sum(digit << (W * j) for j in range(n))
        if v <= M64:
            return v
        n -= 1


def m_edges(W):
    h = 1 << (W - 1)
    return [0, 1, h, h + 1, 1 << 63, M64, m_pattern(W, h), m_pattern(W, h + 1)]


@pytest.fixture(scope="module")
def points(oracle, golden):
    """sub: in the prime-order subgroup; full = B8 + T8 (order 8l); ord8 = T8; gen: another point of order 8l (the G of a table)"""
    from babyjubjub_rs_amd import workload as w
    tors = pack([ints(t) for t in golden["gpu_expected"]["torsion_points"]]).reshape(8, 64)   # j * T8
    kb = oracle.mul_fixed_base(w.random_u256(w.SEED_POINTS ^ 0xE16A, 2))
    return {"b8": rec(B8), "sub": kb[0:1].copy(), "full": oracle.point_add(rec(B8), tors[1:2]), "ord8": tors[1:2].copy(),
            "gen": oracle.point_add(kb[1:2], tors[3:4])}


@pytest.fixture(scope="module")
def R():
    a = scalar_array(NMAX, WIDTHS, 0xE16A)
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def M():
    """(NMAX,) uint64: the edge values of every width first, seeded random values behind them"""
    edges = [m for W in WIDTHS for m in m_edges(W)]
    rnd = np.random.default_rng(0xE16B).integers(0, 1 << 64, size=NMAX - len(edges), dtype=np.uint64)
    a = np.concatenate([np.array(edges, dtype=np.uint64), rnd])
    a.setflags(write=False)
    return a


def as_scalars(m):
    """uint64 values widened to 32-byte little-endian scalars, as the composition takes them"""
    out = np.zeros((m.size, 32), np.uint8)
    out[:, :8] = np.ascontiguousarray(m, dtype="<u8").view(np.uint8).reshape(-1, 8)
    return out


@pytest.fixture(scope="module")
def products(oracle, points, R, M):
    """(point name, 'r' / 'm') -> the oracle's k * P for every scalar of that array; filled on demand, never rewritten"""
    cache = {}
    M32 = as_scalars(M)

    def get(name, which):
        if (name, which) not in cache:
            v = oracle.mul_var_base(rep(points[name], NMAX), R if which == "r" else M32)
            v.setflags(write=False)
            cache[(name, which)] = v
        return cache[(name, which)]
    return get


@pytest.fixture(scope="module")
def tables(points):
    """(context, point name, W) -> FixedBase, created on first use and closed with the module"""
    made = {}

    def get(ctx, name, W):
        if (id(ctx), name, W) not in made:
            made[(id(ctx), name, W)] = ctx.base(points[name], W)
        return made[(id(ctx), name, W)]
    yield get
    for b in made.values():
        if b.ctx.handle:
            b.close()


def want_pair(oracle, products, gname, pkname):
    return products(gname, "r"), oracle.point_add(products(gname, "m"), products(pkname, "r"))


def mismatches(got, want):
    return np.nonzero((np.asarray(got).reshape(-1, 64) != np.asarray(want).reshape(-1, 64)).any(axis=1))[0][:8].tolist()


# ---- 1: against the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", sorted(COMBOS))
@pytest.mark.parametrize("which", ["gpu_ctx", "ctx_w23"])
def test_against_the_oracle(request, oracle, tables, products, R, M, which, combo):
    ctx = request.getfixturevalue(which)
    gw, pw = COMBOS[combo]
    g = None if gw is None else tables(ctx, "gen", gw)
    gname = "b8" if gw is None else "gen"
    for pkname in PKS:
        pk = tables(ctx, pkname, pw)
        w1, w2 = want_pair(oracle, products, gname, pkname)
        for n, off in SIZES:
            c1, c2 = ctx.elgamal_encrypt(pk, M[off:off + n], R[off:off + n], g=g)
            assert c1.shape == (n, 64) and c2.shape == (n, 64)
            assert not mismatches(c1, w1[off:off + n]) and not mismatches(c2, w2[off:off + n]), (
                pkname, n, off, mismatches(c1, w1[off:off + n]), mismatches(c2, w2[off:off + n]))
        c1, c2 = pk.encrypt(M, R, g=g)                                         # the FixedBase form
        assert (c1 == w1).all() and (c2 == w2).all()


# ---- 2: against the library's own composition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_against_the_composition_with_add_arrays(gpu_ctx, tables, products, R, M, combo):
    gw, pw = COMBOS[combo]
    g = None if gw is None else tables(gpu_ctx, "gen", gw)
    pk = tables(gpu_ctx, "full", pw)
    a1, a2 = products("sub", "m"), products("full", "r")                       # any curve points, subgroup and not
    c1, c2, ok = gpu_ctx.elgamal_encrypt(pk, M, R, g=g, add=(a1, a2))
    w1 = gpu_ctx.point_add(a1, gpu_ctx.mul_bases([g], [R]))
    w2 = gpu_ctx.point_add(a2, gpu_ctx.mul_bases([g, pk], [as_scalars(M), R]))
    assert (ok == 1).all() and not mismatches(c1, w1) and not mismatches(c2, w2)
    p1, p2 = gpu_ctx.elgamal_encrypt(pk, M, R, g=g)                            # without add arrays: the two products themselves
    assert (p1 == gpu_ctx.mul_bases([g], [R])).all() and (p2 == gpu_ctx.mul_bases([g, pk], [as_scalars(M), R])).all()


# ---- 3: the add forms ---------------------------------------------------------------------------------------------------------------
def test_bad_addends_refuse_their_own_item_only(gpu_ctx, oracle, tables, products, R, M):
    n = NMAX
    g, pk = tables(gpu_ctx, "gen", 16), tables(gpu_ctx, "sub", 12)
    w1, w2 = want_pair(oracle, products, "gen", "sub")
    a1, a2 = products("full", "r").copy(), products("sub", "m").copy()
    off1, off2, zero1, zero2, both = [0, 63, 511, 700], [1, 64, 512, 1024], [5, 513], [6, 1000], [100]
    for i in off1 + both:
        a1[i, 3] ^= 0x10                                                        # one bit of x: off the curve
    for i in off2:
        a2[i, 40] ^= 0x01                                                       # one bit of y
    a1[zero1] = 0
    a2[zero2 + both] = 0                                                        # (0, 0), the error output of the other calls
    bad = sorted(off1 + off2 + zero1 + zero2 + both)
    c1, c2, ok = gpu_ctx.elgamal_encrypt(pk, M, R, g=g, add=(a1, a2))
    want_ok = np.ones(n, np.uint8)
    want_ok[bad] = 2
    assert (ok == want_ok).all(), np.nonzero(ok != want_ok)[0][:8].tolist()
    e1, e2 = oracle.point_add(products("full", "r"), w1).copy(), oracle.point_add(products("sub", "m"), w2).copy()
    e1[bad] = 0
    e2[bad] = 0
    assert not mismatches(c1, e1) and not mismatches(c2, e2)


def test_ok_may_be_null_without_add_arrays_and_m_none_is_m_zero(gpu_ctx, oracle, tables, products, R, M):
    n = 513
    pk = tables(gpu_ctx, "full", 12)
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    r = np.ascontiguousarray(R[:n])
    m = np.ascontiguousarray(M[:n])
    c1, c2 = np.full(n * 64, 0xEE, np.uint8), np.full(n * 64, 0xEE, np.uint8)
    assert lib.bjj_elgamal_encrypt(h, None, pk.handle.value, m.ctypes.data, r.ctypes.data, None, None, n, c1.ctypes.data, c2.ctypes.data, None) == 0
    w1, w2 = want_pair(oracle, products, "b8", "full")
    assert (c1.reshape(n, 64) == w1[:n]).all() and (c2.reshape(n, 64) == w2[:n]).all()
    ok = np.full(n, 0xEE, np.uint8)
    assert lib.bjj_elgamal_encrypt(h, None, pk.handle.value, m.ctypes.data, r.ctypes.data, None, None, n, c1.ctypes.data, c2.ctypes.data,
                                   ok.ctypes.data) == 0 and (ok == 1).all()                         # if given, it is filled with 1
    z1, z2 = gpu_ctx.elgamal_encrypt(pk, np.zeros(n, np.uint64), r)
    n1, n2 = gpu_ctx.elgamal_encrypt(pk, None, r)
    assert (n1 == z1).all() and (n2 == z2).all() and (n2 == products("full", "r")[:n]).all() and (n1 == w1[:n]).all()
    a1, a2 = products("sub", "r")[:n], products("full", "m")[:n]
    za = gpu_ctx.elgamal_encrypt(pk, np.zeros(n, np.uint64), r, add=(a1, a2))
    na = gpu_ctx.elgamal_rerandomize(pk, a1, a2, r)
    assert all((x == y).all() for x, y in zip(za, na)) and (na[2] == 1).all()


def test_in_place_equals_out_of_place(gpu_ctx, tables, products, R, M):
    import torch
    dev = torch.device("cuda", 0)
    n = NMAX
    g, pk = tables(gpu_ctx, "gen", 5), tables(gpu_ctx, "full", 13)
    a1, a2 = products("sub", "r").copy(), products("full", "m").copy()
    a1[7] = 0                                                                   # one refused item: its zeros land in place too
    a2[600, 1] ^= 4
    d_m, d_r = torch.from_numpy(M.view(np.uint8).copy()).to(dev), torch.from_numpy(R.reshape(-1).copy()).to(dev)
    for m_ptr in (d_m.data_ptr(), None):
        d_a1, d_a2 = torch.from_numpy(a1.reshape(-1)).to(dev), torch.from_numpy(a2.reshape(-1)).to(dev)
        d_c1, d_c2 = torch.zeros(n * 64, dtype=torch.uint8, device=dev), torch.zeros(n * 64, dtype=torch.uint8, device=dev)
        d_ok, d_ok2 = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()   # the arrays above were filled on torch's stream; the library launches on its own
        gpu_ctx.elgamal_encrypt_dev(pk, m_ptr, d_r.data_ptr(), n, d_c1.data_ptr(), d_c2.data_ptr(), g=g, d_add_c1=d_a1.data_ptr(),
                                    d_add_c2=d_a2.data_ptr(), d_ok=d_ok.data_ptr())
        gpu_ctx.sync()
        assert (d_a1.cpu().numpy() == a1.reshape(-1)).all() and (d_a2.cpu().numpy() == a2.reshape(-1)).all()
        gpu_ctx.elgamal_encrypt_dev(pk, m_ptr, d_r.data_ptr(), n, d_a1.data_ptr(), d_a2.data_ptr(), g=g, d_add_c1=d_a1.data_ptr(),
                                    d_add_c2=d_a2.data_ptr(), d_ok=d_ok2.data_ptr())
        gpu_ctx.sync()
        assert bool((d_a1 == d_c1).all()) and bool((d_a2 == d_c2).all()) and bool((d_ok == d_ok2).all())
        ok = d_ok.cpu().numpy()
        assert ok[7] == 2 and ok[600] == 2 and (np.delete(ok, [7, 600]) == 1).all()
        host = gpu_ctx.elgamal_encrypt(pk, None if m_ptr is None else M, R, g=g, add=(a1, a2))
        assert (host[0].reshape(-1) == d_c1.cpu().numpy()).all() and (host[1].reshape(-1) == d_c2.cpu().numpy()).all() and (host[2] == ok).all()


# ---- 4: round trip ------------------------------------------------------------------------------------------------------------------
def test_round_trip_through_decrypt(gpu_ctx, oracle, R):
    n, bits = 257, 16
    sk = 0x1F2E3D4C5B6A79881726354453627180_0F1E2D3C4B5A6978 % L
    pk_point = oracle.mul_fixed_base(pack([sk]).reshape(1, 32))
    pk = gpu_ctx.base(pk_point, 12)
    t = gpu_ctx.dlog_table(None, 8)
    try:
        rng = np.random.default_rng(0xE16C)
        m = rng.integers(0, 1 << (bits - 1), size=n, dtype=np.uint64)
        m[:4] = [0, 1, (1 << (bits - 1)) - 1, 2]
        m2 = rng.integers(0, 1 << (bits - 1), size=n, dtype=np.uint64)
        r, r2 = np.ascontiguousarray(R[n:2 * n]), np.ascontiguousarray(R[:n])     # r2: the directed scalars, 0 and l among them
        c1, c2 = gpu_ctx.elgamal_encrypt(pk, m, r)
        got, ok = gpu_ctx.decrypt(t, sk, c1, c2, bits)
        assert (ok == 1).all() and (got == m).all()
        s1, s2, oks = gpu_ctx.elgamal_encrypt(pk, m2, r2, add=(c1, c2))        # adding a second ciphertext: m + m2
        got, ok = gpu_ctx.decrypt(t, sk, s1, s2, bits)
        assert (oks == 1).all() and (ok == 1).all() and (got == m + m2).all()
        x1, x2, okx = gpu_ctx.elgamal_rerandomize(pk, c1, c2, r2)
        got, ok = gpu_ctx.decrypt(t, sk, x1, x2, bits)
        assert (okx == 1).all() and (ok == 1).all() and (got == m).all()
        moved = np.array([int.from_bytes(bytes(x), "little") % L != 0 for x in r2])
        assert 0 < (~moved).sum() <= 8                                           # r = 0, l, 8l leave a ciphertext as it is
        assert ((x1 != c1).any(axis=1) == moved).all() and ((x2 != c2).any(axis=1) == moved).all()
    finally:
        t.close()
        pk.close()


# ---- 5: beyond one resident grid ----------------------------------------------------------------------------------------------------
def test_second_and_third_trip_against_the_composition(gpu_ctx, tables, points):
    import torch
    dev = torch.device("cuda", 0)
    cus = gpu_ctx.info().compute_units
    n1, n3 = cus * 512 + 1, 2 * cus * 512 + 65
    g, pk = tables(gpu_ctx, "gen", 16), tables(gpu_ctx, "full", 16)
    r = scalar_array(n3, WIDTHS, 0xE16D)
    rng = np.random.default_rng(0xE16E)
    m = rng.integers(0, 1 << 64, size=n3, dtype=np.uint64)
    m[:len(WIDTHS) * 8] = [x for W in WIDTHS for x in m_edges(W)]
    d_r, d_m = torch.from_numpy(r.reshape(-1)).to(dev), torch.from_numpy(m.view(np.uint8)).to(dev)
    d_m32 = torch.from_numpy(as_scalars(m).reshape(-1)).to(dev)
    d_p1, d_p2 = torch.zeros(n3 * 64, dtype=torch.uint8, device=dev), torch.zeros(n3 * 64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()   # the arrays above were filled on torch's stream; the library launches on its own
    gpu_ctx.mul_bases_dev([g], [d_r.data_ptr()], n3, d_p1.data_ptr())
    gpu_ctx.mul_bases_dev([g, pk], [d_m32.data_ptr(), d_r.data_ptr()], n3, d_p2.data_ptr())
    d_c1, d_c2 = torch.zeros(n3 * 64, dtype=torch.uint8, device=dev), torch.zeros(n3 * 64, dtype=torch.uint8, device=dev)
    for n in (n3, n1):
        d_c1.zero_(); d_c2.zero_()
        torch.cuda.synchronize()   # the arrays above were filled on torch's stream; the library launches on its own
        gpu_ctx.elgamal_encrypt_dev(pk, d_m.data_ptr(), d_r.data_ptr(), n, d_c1.data_ptr(), d_c2.data_ptr(), g=g)
        gpu_ctx.sync()
        assert bool((d_c1[:n * 64] == d_p1[:n * 64]).all()) and bool((d_c2[:n * 64] == d_p2[:n * 64]).all()), n
        assert not bool(d_c1[n * 64:].any()) and not bool(d_c2[n * 64:].any())
    # with add arrays (the products of the other array, shifted by one item), one off-curve addend in the last wave
    d_a1, d_a2 = torch.roll(d_p2, 64), torch.roll(d_p1, 64)
    d_w1, d_w2 = torch.zeros_like(d_p1), torch.zeros_like(d_p2)
    torch.cuda.synchronize()   # the arrays above were filled on torch's stream; the library launches on its own
    gpu_ctx.point_add_dev(d_a1.data_ptr(), d_p1.data_ptr(), n3, d_w1.data_ptr())
    gpu_ctx.point_add_dev(d_a2.data_ptr(), d_p2.data_ptr(), n3, d_w2.data_ptr())
    gpu_ctx.sync()
    bad = n3 - 3
    d_a2[bad * 64 + 2] ^= 1
    d_w1[bad * 64:(bad + 1) * 64] = 0
    d_w2[bad * 64:(bad + 1) * 64] = 0
    d_ok = torch.zeros(n3, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()   # the arrays above were filled on torch's stream; the library launches on its own
    gpu_ctx.elgamal_encrypt_dev(pk, d_m.data_ptr(), d_r.data_ptr(), n3, d_c1.data_ptr(), d_c2.data_ptr(), g=g, d_add_c1=d_a1.data_ptr(),
                                d_add_c2=d_a2.data_ptr(), d_ok=d_ok.data_ptr())
    gpu_ctx.sync()
    assert bool((d_c1 == d_w1).all()) and bool((d_c2 == d_w2).all())
    ok = d_ok.cpu().numpy()
    assert ok[bad] == 2 and (np.delete(ok, bad) == 1).all()


# ---- 6: the forms agree; two streams at once ---------------------------------------------------------------------------------------
def test_pageable_pinned_and_dev_forms_agree(gpu_ctx, oracle, tables, products, R, M):
    import torch
    n = NMAX
    g, pk = tables(gpu_ctx, "gen", 16), tables(gpu_ctx, "sub", 12)
    a1, a2 = products("full", "r"), products("sub", "m")
    pageable = gpu_ctx.elgamal_encrypt(pk, M, R, g=g, add=(a1, a2))
    w1, w2 = want_pair(oracle, products, "gen", "sub")
    assert (pageable[0] == oracle.point_add(a1, w1)).all() and (pageable[1] == oracle.point_add(a2, w2)).all()
    sizes = [n * 8, n * 32, n * 64, n * 64, n * 64, n * 64, n]
    pins = [gpu_ctx.host_empty(s) for s in sizes]
    try:
        for p, src in zip(pins, (M.view(np.uint8), R.reshape(-1), a1.reshape(-1), a2.reshape(-1))):
            p[:] = src
        for p in pins[4:]:
            p[:] = 0xEE
        assert all(gpu_ctx.host_is_pinned(p) for p in pins)
        assert gpu_ctx.lib.bjj_elgamal_encrypt(gpu_ctx.handle, g.handle.value, pk.handle.value, *[p.ctypes.data for p in pins[:4]], n,
                                               *[p.ctypes.data for p in pins[4:]]) == 0, gpu_ctx.lib.bjj_last_error()
        for p, want in zip(pins[4:], pageable):
            assert (np.asarray(p) == want.reshape(-1)).all()
    finally:
        for p in pins:
            gpu_ctx.host_free(p)
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(np.ascontiguousarray(x).reshape(-1).view(np.uint8).copy()).to(dev) for x in (M, R, a1, a2)]
    outs = [torch.zeros(s, dtype=torch.uint8, device=dev) for s in sizes[4:]]
    torch.cuda.synchronize()   # the arrays above were filled on torch's stream; the library launches on its own
    gpu_ctx.elgamal_encrypt_dev(pk, d[0].data_ptr(), d[1].data_ptr(), n, outs[0].data_ptr(), outs[1].data_ptr(), g=g, d_add_c1=d[2].data_ptr(),
                                d_add_c2=d[3].data_ptr(), d_ok=outs[2].data_ptr())
    gpu_ctx.sync()
    for o, want in zip(outs, pageable):
        assert (o.cpu().numpy() == want.reshape(-1)).all()


def test_two_streams_at_once_with_different_keys(gpu_ctx, oracle, tables, products, R, M):
    import torch
    dev = torch.device("cuda", 0)
    n = NMAX
    cases = [(tables(gpu_ctx, "gen", 16), tables(gpu_ctx, "sub", 12), want_pair(oracle, products, "gen", "sub")),
             (None, tables(gpu_ctx, "full", 4), want_pair(oracle, products, "b8", "full"))]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    d_m, d_r = torch.from_numpy(M.view(np.uint8).copy()).to(dev), torch.from_numpy(R.reshape(-1).copy()).to(dev)
    outs = [[torch.zeros(n * 64, dtype=torch.uint8, device=dev) for _ in range(2)] for _ in range(2)]
    torch.cuda.synchronize()
    for rep_ in range(3):
        for s, (g, pk, _) in enumerate(cases):
            gpu_ctx.elgamal_encrypt_dev(pk, d_m.data_ptr(), d_r.data_ptr(), n, outs[s][0].data_ptr(), outs[s][1].data_ptr(), g=g,
                                        stream=streams[s].cuda_stream)
        gpu_ctx.sync()
        for s in range(2):
            for k in range(2):
                assert (outs[s][k].cpu().numpy().reshape(n, 64) == cases[s][2][k]).all(), (rep_, s, k)
                outs[s][k].zero_()
        torch.cuda.synchronize()


# ---- 7: rejections ------------------------------------------------------------------------------------------------------------------
def test_rejections(gpu_ctx, ctx_w23, points, tables, R, M):
    import torch
    import babyjubjub_rs_amd as bjj
    from babyjubjub_rs_amd import _lib
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    E = _lib.BJJ_E_INVALID
    n = 65
    pk, g = tables(gpu_ctx, "sub", 12).handle.value, tables(gpu_ctx, "gen", 5).handle.value
    foreign = tables(ctx_w23, "sub", 12).handle.value
    gone = gpu_ctx.base(points["ord8"], 4)
    stale = gone.handle.value
    gone.close()
    with pytest.raises(bjj.BjjError):                 # the binding refuses a closed base ...
        gpu_ctx.elgamal_encrypt(gone, M[:n], R[:n])
    with pytest.raises(bjj.BjjError):
        gone.encrypt(M[:n], R[:n])
    with pytest.raises(bjj.BjjError):
        gpu_ctx.elgamal_encrypt(None, M[:n], R[:n])
    r, m = np.ascontiguousarray(R[:n]), np.ascontiguousarray(M[:n])
    a = np.ascontiguousarray(rep(points["sub"], n))
    c1, c2, ok = np.full(n * 64, 0xEE, np.uint8), np.full(n * 64, 0xEE, np.uint8), np.full(n, 0xEE, np.uint8)
    P = lambda x: None if x is None else x.ctypes.data

    def host(g_, pk_, m_, r_, a1_, a2_, n_, c1_, c2_, ok_):
        return lib.bjj_elgamal_encrypt(h, g_, pk_, P(m_), P(r_), P(a1_), P(a2_), n_, P(c1_), P(c2_), P(ok_))
    assert host(g, pk, m, r, a, None, n, c1, c2, ok) == E and b"both or neither" in lib.bjj_last_error()
    assert host(g, pk, m, r, None, a, n, c1, c2, ok) == E
    assert host(g, None, m, r, None, None, n, c1, c2, ok) == E and b"pk is NULL" in lib.bjj_last_error()
    assert host(g, stale, m, r, None, None, n, c1, c2, ok) == E          # ... and the library a handle it does not list
    assert host(stale, pk, m, r, None, None, n, c1, c2, ok) == E
    assert host(g, foreign, m, r, None, None, n, c1, c2, ok) == E and b"not a base of this context" in lib.bjj_last_error()
    assert host(foreign, pk, m, r, None, None, n, c1, c2, ok) == E
    assert host(g, pk, m, None, None, None, n, c1, c2, ok) == E
    assert host(g, pk, m, r, None, None, n, None, c2, ok) == E
    assert host(g, pk, m, r, None, None, n, c1, None, ok) == E
    assert host(g, pk, m, r, a, a, n, c1, c2, None) == E and b"ok is NULL" in lib.bjj_last_error()
    assert host(g, pk, m, r, None, None, 1 << 32, c1, c2, ok) == E
    assert host(g, pk, None, None, None, None, 0, None, None, None) == 0  # n == 0: nothing is looked at
    assert (c1 == 0xEE).all() and (c2 == 0xEE).all() and (ok == 0xEE).all()

    dev = torch.device("cuda", 0)
    pad = np.zeros(16, np.uint8)
    d_r = torch.from_numpy(np.concatenate([r.reshape(-1), pad])).to(dev)
    d_m = torch.from_numpy(np.concatenate([m.view(np.uint8), pad])).to(dev)
    d_a = torch.from_numpy(np.concatenate([a.reshape(-1), pad])).to(dev)
    d_c1, d_c2 = (torch.full((n * 64 + 16,), 0xEE, dtype=torch.uint8, device=dev) for _ in range(2))
    d_ok = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device=dev)
    pm, pr, pa, p1, p2, pok = (t.data_ptr() for t in (d_m, d_r, d_a, d_c1, d_c2, d_ok))

    def devf(g_, pk_, m_, r_, a1_, a2_, n_, c1_, c2_, ok_):
        return lib.bjj_elgamal_encrypt_dev(h, g_, pk_, m_, r_, a1_, a2_, n_, c1_, c2_, ok_, None)
    torch.cuda.synchronize()   # the arrays above were filled on torch's stream; the library launches on its own
    assert devf(g, pk, pm, pr, pa, None, n, p1, p2, pok) == E
    assert devf(g, pk, pm, pr, None, pa, n, p1, p2, pok) == E
    assert devf(g, None, pm, pr, None, None, n, p1, p2, pok) == E
    assert devf(g, stale, pm, pr, None, None, n, p1, p2, pok) == E
    assert devf(g, foreign, pm, pr, None, None, n, p1, p2, pok) == E
    for bad in ((pm + 8, pr, None, None, p1, p2), (pm, pr + 8, None, None, p1, p2), (pm, pr, pa + 8, pa, p1, p2), (pm, pr, pa, pa + 8, p1, p2),
                (pm, pr, None, None, p1 + 8, p2), (pm, pr, None, None, p1, p2 + 8), (pm, None, None, None, p1, p2), (pm, pr, None, None, None, p2),
                (pm, pr, None, None, p1, None)):
        assert devf(g, pk, bad[0], bad[1], bad[2], bad[3], n, bad[4], bad[5], pok) == E, bad
    assert devf(g, pk, pm, pr, pa, pa, n, p1, p2, None) == E
    assert devf(g, pk, None, None, None, None, 0, None, None, None) == 0
    gpu_ctx.sync()
    assert bool((d_c1 == 0xEE).all()) and bool((d_c2 == 0xEE).all()) and bool((d_ok == 0xEE).all())
    assert devf(g, pk, pm, pr, None, None, n, p1, p2, pok + 1) == 0       # d_ok: any address
    gpu_ctx.sync()
    assert bool((d_ok[0] == 0xEE).all()) and bool((d_ok[1:n + 1] == 1).all()) and bool((d_ok[n + 1:] == 0xEE).all())
    assert bool((d_c1[n * 64:] == 0xEE).all()) and bool((d_c2[n * 64:] == 0xEE).all())
