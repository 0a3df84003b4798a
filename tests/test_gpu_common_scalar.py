"""bjj_mul_common, bjj_in_subgroup and bjj_elgamal_decrypt on the GPU (include/bjj_hip_common_scalar.h), both forced forms of the
kernel and the rule's choice.  The yardstick is what the library already had: bjj_mul_var_base with the scalar replicated, followed
by bjj_point_add (negating with api._negate_x for a subtraction), byte for byte on the on-curve items; ok = 2 and (0, 0) on the
others; Context.elgamal_decrypt for the one-call decryption."""
import os

import numpy as np
import pytest

from conftest import ints, pack, unpack

pytestmark = pytest.mark.gpu

E_INVALID = -1
Q = 21888242871839275222246405745257275088548364400416034343698204186575808495617
L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
ORDER8 = 8 * L
NMAX = 1000
SIZES = (1, 63, 64, 65, 255, 256, 257, NMAX)       # wave, tile and ragged-tail boundaries
FORMS = ("naf", "table", "rule")
SCALARS = [0, 1, 2, 8, L - 1, L, L + 1, ORDER8 - 1, ORDER8, ORDER8 + 1, 1 << 253, (1 << 254) - 1, (1 << 256) - 1,
           int("AA" * 32, 16), int("55" * 32, 16), (1 << 255) - 1, 0xD1B54A32D192ED03, 0x9E3779B97F4A7C15F39CC0605CEDC834,
           0x0B3C9F1E5D7A2C48E6F1093B5A7D2C4E8F6A1B3C5D7E9F0A1B2C3D4E5F60718, 0x2A6D5E0F1B3C7A9948D1C0E2F3B4A59687766554433221100FFEEDDCCBBAA998]
FULL = SCALARS[-1]


def on_curve(p):
    x, y = p[0] % Q, p[1] % Q
    return (168700 * x * x + y * y - 1 - 168696 * x * x * y * y) % Q == 0


def context_with_form(form, extra_env=None):
    """BJJ_COMMON_FORM is read once, at bjj_init"""
    import babyjubjub_rs_amd as bjj
    env = dict(extra_env or {})
    if form != "rule":
        env["BJJ_COMMON_FORM"] = form
    old = {k: os.environ.get(k) for k in list(env) + ["BJJ_COMMON_FORM"]}
    os.environ.pop("BJJ_COMMON_FORM", None)
    os.environ.update(env)
    try:
        return bjj.Context(0, 16)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctxs():
    made = {f: context_with_form(f) for f in FORMS}
    yield made
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def data(gpu_ctx, oracle, golden):
    """NMAX points -- B8, the identity, orders 2, 4, 8, subgroup points, subgroup + torsion, a coordinate >= r, off-curve, (0, 0), in
    turn -- and as many addends of the same kinds in another order; per scalar the products by bjj_mul_var_base.  Computed once."""
    rng = np.random.default_rng(0xC5C5)
    tors = [ints(t) for t in golden["gpu_expected"]["torsion_points"]]
    low = sorted(set(tors) | {(0, 1)})
    assert len(low) == 8 and (0, 1) in low and (0, Q - 1) in low
    sub = unpack(oracle.mul_fixed_base(pack([int.from_bytes(rng.bytes(31), "little") for _ in range(NMAX)])), 2)
    nontrivial = [t for t in low if t != (0, 1)]

    def shifted(i):
        return unpack(oracle.point_add(pack([sub[i]]), pack([nontrivial[i % 7]])), 2)[0]
    b8 = unpack(oracle.mul_fixed_base(pack([1])), 2)[0]

    def kind(i, j):
        k = j % 16
        if k == 0:
            return b8
        if k == 1:
            return (0, 1)
        if k in (2, 3, 4):
            return [(0, Q - 1), nontrivial[i % 7], nontrivial[(3 * i + 1) % 7]][k - 2]      # order 2, and the seven of order 2, 4, 8 in turn
        if k in (5, 6, 7, 8, 9):
            return sub[i]
        if k in (10, 11, 12):
            return shifted(i)
        if k == 13:
            return (sub[i][0] + Q, sub[i][1])            # x >= r, < 2^256
        if k == 14:
            return (sub[i][0] ^ 1, sub[i][1])            # off the curve
        return (0, 0)
    pts = [kind(i, i) for i in range(NMAX)]
    add = [kind(i, 5 * i + 7) for i in range(NMAX)]     # every kind of addend meets every kind of point (5 is odd: coprime to 16)
    P, A = pack(pts).reshape(NMAX, 64), pack(add).reshape(NMAX, 64)
    p_on = np.array([on_curve(p) for p in pts])
    a_on = np.array([on_curve(p) for p in add])
    assert 100 < (~p_on).sum() < 140 and (p_on & ~a_on).sum() > 50 and not on_curve(pts[14]) and pts[15] == (0, 0)
    prod = {k: gpu_ctx.mul_var_base(P, np.tile(pack([k]), NMAX)) for k in SCALARS}
    for a in (P, A, p_on, a_on, *prod.values()):
        a.setflags(write=False)
    return {"P": P, "A": A, "p_on": p_on, "a_on": a_on, "prod": prod, "low": low, "sub": sub, "nontrivial": nontrivial, "b8": b8}


def want_of(gpu_ctx, data, k, n, with_add, subtract):
    """(out, ok): bjj_mul_var_base then bjj_point_add on the on-curve items, (0, 0) / 2 on the others"""
    from babyjubjub_rs_amd import api
    on = data["p_on"][:n] & (data["a_on"][:n] if with_add else True)
    t = np.array(data["prod"][k][:n])
    t[~data["p_on"][:n]] = 0                             # what the variable-base kernel wrote for an off-curve point does not matter
    if subtract:
        t = api._negate_x(t)
    if with_add:
        t = gpu_ctx.point_add(np.ascontiguousarray(data["A"][:n]), t)
    out = np.array(t).reshape(n, 64)
    out[~on] = 0
    return out, np.where(on, 1, 2).astype(np.uint8)


VARIANTS = [(False, False), (True, True), (False, True), (True, False)]   # (with_add, subtract)


# ---- bjj_mul_common ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_host_form_every_scalar(gpu_ctx, ctxs, data, form):
    ctx = ctxs[form]
    n = NMAX
    for k in SCALARS:
        for with_add, subtract in VARIANTS:
            out, ok = ctx.mul_common(k, data["P"], data["A"] if with_add else None, subtract)
            wout, wok = want_of(gpu_ctx, data, k, n, with_add, subtract)
            assert (ok == wok).all(), (form, hex(k), with_add, subtract)
            assert (out == wout).all(), (form, hex(k), with_add, subtract, np.nonzero((out != wout).any(axis=1))[0][:8])
        if k % ORDER8 == 0:                              # k == 0 (mod 8l): A itself, and the identity without an addend
            out, ok = ctx.mul_common(k, data["P"], None, False)
            assert all(tuple(v) == (0, 1) for v, on in zip(unpack(out, 2), data["p_on"]) if on)


@pytest.fixture(scope="module")
def random_scalars(gpu_ctx, data):
    """a seeded thousand random scalars over the first 32 records of the mix (every kind twice); the yardsticks in three batched
    calls: bjj_mul_var_base over all 32 000 pairs, and bjj_point_add of the addends to the products and to their negations"""
    from babyjubjub_rs_amd import api
    rng = np.random.default_rng(0xC5CA)
    ks = [int.from_bytes(rng.bytes(32), "little") for _ in range(1000)]
    m = 32
    P, A = np.tile(data["P"][:m], (len(ks), 1)), np.tile(data["A"][:m], (len(ks), 1))
    prod = gpu_ctx.mul_var_base(P, np.repeat(pack(ks).reshape(-1, 32), m, axis=0))
    prod[np.tile(~data["p_on"][:m], len(ks))] = 0
    want = {(False, False): prod, (False, True): api._negate_x(prod)}
    for sub in (False, True):
        want[(True, sub)] = gpu_ctx.point_add(A, want[(False, sub)])
    return ks, m, {k: v.reshape(len(ks), m, 64) for k, v in want.items()}


@pytest.mark.parametrize("form", FORMS)
def test_a_thousand_random_scalars(ctxs, data, random_scalars, form):
    ctx = ctxs[form]
    ks, m, want = random_scalars
    P, A = np.ascontiguousarray(data["P"][:m]), np.ascontiguousarray(data["A"][:m])
    for j, k in enumerate(ks):
        with_add, subtract = VARIANTS[j % 4]
        on = data["p_on"][:m] & (data["a_on"][:m] if with_add else True)
        out, ok = ctx.mul_common(k, P, A if with_add else None, subtract)
        assert (ok == np.where(on, 1, 2)).all(), (form, j, hex(k))
        assert (out[on] == want[(with_add, subtract)][j][on]).all() and (out[~on] == 0).all(), (form, j, hex(k), with_add, subtract)


@pytest.mark.parametrize("form", FORMS)
def test_device_form_every_size(gpu_ctx, ctxs, data, form):
    import torch
    ctx = ctxs[form]
    dev = torch.device("cuda", 0)
    d_p = torch.from_numpy(data["P"].reshape(-1).copy()).to(dev)
    d_a = torch.from_numpy(data["A"].reshape(-1).copy()).to(dev)
    for n in SIZES:
        for k in (FULL, 8, L - 1):
            for with_add, subtract in VARIANTS[:2]:
                d_out = torch.full((n * 64 + 64,), 0xEE, dtype=torch.uint8, device=dev)
                d_ok = torch.full((n + 7,), 0xEE, dtype=torch.uint8, device=dev)
                ctx.mul_common_dev(k, d_p.data_ptr(), d_a.data_ptr() if with_add else None, n, d_out.data_ptr(), d_ok.data_ptr() + 3, subtract)
                ctx.sync()
                wout, wok = want_of(gpu_ctx, data, k, n, with_add, subtract)
                out, ok = d_out.cpu().numpy(), d_ok.cpu().numpy()
                assert (ok[3:3 + n] == wok).all() and (ok[:3] == 0xEE).all() and (ok[3 + n:] == 0xEE).all(), (form, n, hex(k), with_add)
                assert (out[:n * 64].reshape(n, 64) == wout).all() and (out[n * 64:] == 0xEE).all(), (form, n, hex(k), with_add)


@pytest.mark.parametrize("form", FORMS)
def test_every_off_curve_position_within_a_wave(ctxs, data, form):
    """the batched inversion passes a skipped lane by wherever it sits: the other 64 results do not move"""
    import torch
    ctx = ctxs[form]
    dev = torch.device("cuda", 0)
    n = 65
    good = pack([data["sub"][i] for i in range(n)]).reshape(n, 64)
    base, ok = ctx.mul_common(FULL, good, good[::-1].copy(), True)
    assert (ok == 1).all()
    d_out = torch.empty(n * 64, dtype=torch.uint8, device=dev)
    d_ok = torch.empty(n, dtype=torch.uint8, device=dev)
    for pos in range(64):
        bad = good.copy()
        bad[pos, 0] ^= 1
        d_p = torch.from_numpy(bad.reshape(-1)).to(dev)
        d_a = torch.from_numpy(good[::-1].copy().reshape(-1)).to(dev)
        ctx.mul_common_dev(FULL, d_p.data_ptr(), d_a.data_ptr(), n, d_out.data_ptr(), d_ok.data_ptr(), True)
        ctx.sync()
        out, ok = d_out.cpu().numpy().reshape(n, 64), d_ok.cpu().numpy()
        keep = np.arange(n) != pos
        assert ok[pos] == 2 and (out[pos] == 0).all() and (ok[keep] == 1).all() and (out[keep] == base[keep]).all(), (form, pos)


# ---- bjj_in_subgroup ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_in_subgroup(gpu_ctx, oracle, ctxs, data, form):
    import torch
    ctx = ctxs[form]
    sub, low, nontrivial = data["sub"], data["low"], data["nontrivial"]
    translates = [unpack(oracle.point_add(pack([sub[0]]), pack([t])), 2)[0] for t in nontrivial]
    pts = sub[:40] + translates + low + [(sub[1][0] ^ 1, sub[1][1]), (0, 0), (sub[2][0] + Q, sub[2][1]), data["b8"]]
    want = [1] * 40 + [0] * 7 + [1 if t == (0, 1) else 0 for t in low] + [2, 2, 1, 1]
    P = pack(pts).reshape(-1, 64)
    n = len(pts)
    lrep = np.tile(pack([L]), n)
    identity = pack([(0, 1)]).tobytes()
    for ref in (gpu_ctx.mul_var_base(P, lrep), oracle.mul_var_base(P, lrep)):     # the composition, and the oracle
        by_mul = [2 if not on_curve(p) else 1 if bytes(ref.reshape(n, 64)[i]) == identity else 0 for i, p in enumerate(pts)]
        assert by_mul == want
    assert ctx.in_subgroup(P).tolist() == want
    big = np.concatenate([P] * 18)[:NMAX]                                           # the same records over every size
    wbig = (want * 18)[:NMAX]
    dev = torch.device("cuda", 0)
    d_p = torch.from_numpy(big.reshape(-1).copy()).to(dev)
    for m in SIZES:
        d_ok = torch.full((m + 5,), 0xEE, dtype=torch.uint8, device=dev)
        ctx.in_subgroup_dev(d_p.data_ptr(), m, d_ok.data_ptr() + 1)
        ctx.sync()
        got = d_ok.cpu().numpy()
        assert got[1:1 + m].tolist() == wbig[:m] and (got[:1] == 0xEE).all() and (got[1 + m:] == 0xEE).all(), (form, m)
    assert ctx.in_subgroup(big).tolist() == wbig


# ---- bjj_elgamal_decrypt -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ciphertexts(gpu_ctx):
    """(C1, C2) = (r B8, m B8 + r PK) for 16-bit m, PK = sk B8, with an off-curve C1 and an off-curve C2 among them"""
    rng = np.random.default_rng(0xE16B)
    n = NMAX
    sk = int.from_bytes(rng.bytes(31), "little") % L
    ms = [int(v) for v in rng.integers(0, 1 << 16, n)]
    ms[:6] = [0, 1, (1 << 16) - 1, 1 << 15, 63, 64]
    rs = [int.from_bytes(rng.bytes(31), "little") for _ in range(n)]
    pk = tuple(unpack(gpu_ctx.mul_fixed_base(pack([sk])), 2)[0])
    base = gpu_ctx.base(pk, 8)
    try:
        c1 = gpu_ctx.mul_fixed_base(pack(rs)).reshape(n, 64).copy()
        c2 = gpu_ctx.mul_bases([None, base], [pack(ms), pack(rs)]).reshape(n, 64).copy()
    finally:
        base.close()
    c1[70, 0] ^= 1
    c2[130, 32] ^= 1
    c2[257] = 0
    for a in (c1, c2):
        a.setflags(write=False)
    return {"sk": sk, "ms": ms, "c1": c1, "c2": c2, "bad": [70, 130, 257]}


UMAX = (1 << 64) - 1


@pytest.mark.parametrize("form", FORMS)
def test_decrypt_equals_the_four_call_composition(ctxs, ciphertexts, form):
    import torch
    ctx = ctxs[form]
    c = ciphertexts
    n = NMAX
    dev = torch.device("cuda", 0)
    d_c1 = torch.from_numpy(c["c1"].reshape(-1).copy()).to(dev)
    d_c2 = torch.from_numpy(c["c2"].reshape(-1).copy()).to(dev)
    for b in (8, 12):                                    # two table widths
        t = ctx.dlog_table(None, b)
        try:
            for key, rb in ((c["sk"], 16), (c["sk"] + 1, 16), (c["sk"], 6), (c["sk"] + ORDER8, 17)):   # 6: range_bits below baby_bits
                wm, wok = ctx.elgamal_decrypt(t, key % ORDER8, c["c1"], c["c2"], rb)
                m, ok = ctx.decrypt(t, key, c["c1"], c["c2"], rb)
                assert (m == wm).all() and (ok == wok).all(), (form, b, rb)
                right = key % L == c["sk"]
                for i in range(n):
                    if i in c["bad"]:
                        assert ok[i] == 2 and int(m[i]) == UMAX
                    elif right and c["ms"][i] < 1 << rb:
                        assert ok[i] == 1 and int(m[i]) == c["ms"][i]
                    else:
                        assert ok[i] == 0 and int(m[i]) == UMAX      # a wrong key: none found, never a wrong m
                for cnt in (1, 65, 257, n):
                    d_m = torch.full((cnt * 8 + 16,), 0xEE, dtype=torch.uint8, device=dev)
                    d_ok = torch.full((cnt + 4,), 0xEE, dtype=torch.uint8, device=dev)
                    ctx.decrypt_dev(t, key, d_c1.data_ptr(), d_c2.data_ptr(), cnt, rb, d_m.data_ptr(), d_ok.data_ptr() + 1)
                    ctx.sync()
                    gm, gok = d_m.cpu().numpy(), d_ok.cpu().numpy()
                    assert gm[:cnt * 8].tobytes() == wm[:cnt].tobytes() and (gm[cnt * 8:] == 0xEE).all(), (form, b, rb, cnt)
                    assert gok[1:1 + cnt].tobytes() == wok[:cnt].tobytes() and gok[0] == 0xEE and (gok[1 + cnt:] == 0xEE).all()
        finally:
            t.close()


def test_decrypt_cut_into_several_launches(ctxs, ciphertexts):
    """BJJ_DLOG_LAUNCH_STEPS = 4096: n = 1000 items x 128 giant steps are cut into chunks of items and launches of steps, over the
    context's block of decrypted points.  Same bytes as the uncut call."""
    c = ciphertexts
    cut = context_with_form("rule", {"BJJ_DLOG_LAUNCH_STEPS": "4096"})
    try:
        t0, t1 = ctxs["rule"].dlog_table(None, 8), cut.dlog_table(None, 8)
        for key in (c["sk"], c["sk"] + 5):
            wm, wok = ctxs["rule"].decrypt(t0, key, c["c1"], c["c2"], 16)
            m, ok = cut.decrypt(t1, key, c["c1"], c["c2"], 16)
            assert (m == wm).all() and (ok == wok).all()
            em, eok = cut.elgamal_decrypt(t1, key, c["c1"], c["c2"], 16)
            assert (m == em).all() and (ok == eok).all()
        t0.close()
    finally:
        cut.close()


def test_decrypt_two_streams_at_once(ctxs, ciphertexts):
    import torch
    ctx = ctxs["rule"]
    c = ciphertexts
    n = NMAX
    dev = torch.device("cuda", 0)
    t = ctx.dlog_table(None, 8)
    try:
        keys = (c["sk"], c["sk"] + 3)
        want = [ctx.decrypt(t, k, c["c1"], c["c2"], 16) for k in keys]
        streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        d_c1 = [torch.from_numpy(c["c1"].reshape(-1).copy()).to(dev) for _ in range(2)]
        d_c2 = [torch.from_numpy(c["c2"].reshape(-1).copy()).to(dev) for _ in range(2)]
        d_m = [torch.full((n * 8,), 0xEE, dtype=torch.uint8, device=dev) for _ in range(2)]
        d_ok = [torch.full((n,), 0xEE, dtype=torch.uint8, device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        for rep_ in range(3):
            for s in range(2):
                ctx.decrypt_dev(t, keys[s], d_c1[s].data_ptr(), d_c2[s].data_ptr(), n, 16, d_m[s].data_ptr(), d_ok[s].data_ptr(),
                                stream=streams[s].cuda_stream)
            ctx.sync()
            for s in range(2):
                assert d_m[s].cpu().numpy().tobytes() == want[s][0].tobytes() and d_ok[s].cpu().numpy().tobytes() == want[s][1].tobytes(), (rep_, s)
                d_m[s].fill_(0xEE)
                d_ok[s].fill_(0xEE)
            torch.cuda.synchronize()
    finally:
        t.close()


# ---- rejections with a live context --------------------------------------------------------------------------------------------------
def test_call_rejections(ctxs, ctx_w23, ciphertexts, data):
    import torch
    ctx = ctxs["rule"]
    lib, h = ctx.lib, ctx.handle
    c = ciphertexts
    n = 16
    t = ctx.dlog_table(None, 8)
    foreign = ctx_w23.dlog_table(None, 8)
    freed = ctx.dlog_table(None, 4)
    freed_handle = freed.handle.value
    freed.close()
    k = pack([c["sk"]])
    c1, c2 = np.ascontiguousarray(c["c1"][:n]), np.ascontiguousarray(c["c2"][:n])
    m = np.full(n, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    ok = np.full(n, 0xEE, dtype=np.uint8)
    out = np.full(n * 64, 0xEE, dtype=np.uint8)
    try:
        def dec(table, sk=k.ctypes.data, a=c1.ctypes.data, b=c2.ctypes.data, rb=16, pm=m.ctypes.data, pok=ok.ctypes.data):
            return lib.bjj_elgamal_decrypt(h, table, sk, a, b, n, rb, pm, pok)
        assert dec(None) == E_INVALID and b"table is NULL" in lib.bjj_last_error()
        assert dec(foreign.handle) == E_INVALID and b"of this context" in lib.bjj_last_error()
        assert dec(freed_handle) == E_INVALID and b"of this context" in lib.bjj_last_error()
        for rb in (0, -3, 26, 46, 64):                   # the cap of an 8-bit table is 25
            assert dec(t.handle, rb=rb) == E_INVALID and b"range_bits" in lib.bjj_last_error(), rb
        for kw in ({"sk": None}, {"a": None}, {"b": None}, {"pm": None}, {"pok": None}):
            assert dec(t.handle, **kw) == E_INVALID, kw
        assert lib.bjj_elgamal_decrypt_dev(h, None, k.ctypes.data, 0, 0, n, 16, 0, 0, None) == E_INVALID and b"table is NULL" in lib.bjj_last_error()
        assert lib.bjj_mul_common(h, None, c1.ctypes.data, None, 0, n, out.ctypes.data, ok.ctypes.data) == E_INVALID
        assert lib.bjj_mul_common(h, k.ctypes.data, None, None, 0, n, out.ctypes.data, ok.ctypes.data) == E_INVALID
        assert lib.bjj_mul_common(h, k.ctypes.data, c1.ctypes.data, None, 0, n, None, ok.ctypes.data) == E_INVALID
        assert lib.bjj_mul_common(h, k.ctypes.data, c1.ctypes.data, None, 0, n, out.ctypes.data, None) == E_INVALID
        assert lib.bjj_in_subgroup(h, None, n, ok.ctypes.data) == E_INVALID and lib.bjj_in_subgroup(h, c1.ctypes.data, n, None) == E_INVALID
        assert (m == 0xEEEEEEEEEEEEEEEE).all() and (ok == 0xEE).all() and (out == 0xEE).all()
        # n == 0 touches nothing, whatever the pointers
        assert dec(t.handle) == 0 and lib.bjj_elgamal_decrypt(h, t.handle, k.ctypes.data, None, None, 0, 16, None, None) == 0
        assert lib.bjj_mul_common(h, k.ctypes.data, None, None, 1, 0, None, None) == 0 and lib.bjj_in_subgroup(h, None, 0, None) == 0
        # the device forms: misaligned or NULL pointers
        dev = torch.device("cuda", 0)
        d_p = torch.from_numpy(np.concatenate([c1.reshape(-1), np.zeros(64, np.uint8)])).to(dev)
        d_o = torch.full((n * 64 + 64,), 0xEE, dtype=torch.uint8, device=dev)
        d_k = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device=dev)
        p, o, f = d_p.data_ptr(), d_o.data_ptr(), d_k.data_ptr()
        for args in ((p + 8, None, o, f), (0, None, o, f), (p, p + 8, o, f), (p, None, o + 8, f), (p, None, 0, f), (p, None, o, 0)):
            assert lib.bjj_mul_common_dev(h, k.ctypes.data, args[0], args[1], 0, n, args[2], args[3], None) == E_INVALID, args
        assert lib.bjj_mul_common_dev(h, None, p, None, 0, n, o, f, None) == E_INVALID
        for args in ((p + 8, f), (0, f), (p, 0)):
            assert lib.bjj_in_subgroup_dev(h, args[0], n, args[1], None) == E_INVALID, args
        for args in ((p + 8, p, o, f), (p, p + 8, o, f), (0, p, o, f), (p, 0, o, f), (p, p, o + 8, f), (p, p, 0, f), (p, p, o, 0)):
            assert lib.bjj_elgamal_decrypt_dev(h, t.handle, k.ctypes.data, args[0], args[1], n, 16, args[2], args[3], None) == E_INVALID, args
        assert lib.bjj_elgamal_decrypt_dev(h, t.handle, None, p, p, n, 16, o, f, None) == E_INVALID
        ctx.sync()
        assert (d_o.cpu().numpy() == 0xEE).all() and (d_k.cpu().numpy() == 0xEE).all()
    finally:
        t.close()
        foreign.close()
