"""include/bjj_hip_dleq.h on the MI355X: bjj_mul_pair, bjj_dleq_verify and bjj_dleq_prove, host and _dev forms, at n = 1, 63, 64, 65,
257 and 1000.  Expected values come from the plain-integer model of tests/dleq_ref.py run over the C oracle (CBackend: mul_var_base,
point_add, poseidon5 -- the pure-Python oracle is not used here) and from the library's own composition in the same process
(bjj_mul_var_base, bjj_point_add, bjj_mul_bases, bjj_mul_common, bjj_poseidon5).  The inputs of every size are slices of ONE array
per argument with the directed sets in front, so the model runs once and the sizes share it.  Every comparison is byte for byte."""
import os
import random
import re

import numpy as np
import pytest

import dleq_ref as dr
from conftest import ROOT, ints

pytestmark = pytest.mark.gpu

NMAX = 1000
SIZES = (1, 63, 64, 65, 257, 1000)      # a lane, a wave less one, a wave, a wave and one, a workgroup and one, four workgroups less 24
SK, SK2, LABEL = dr.L + 0x1F2E3D4C5B6A7988, 0xABCDEF0123456789, 3
# G (None: the context's B8 table; else a point of dleq_ref.world), its table width, the width of PK's table
SETUPS = {"b8_pk12": (None, 0, 12), "gen13_pk5": ("s2", 13, 5)}
CSRC = os.path.join(ROOT, "babyjubjub-rs_amd", "csrc")


def P(x):
    return dr.pack_points(x)


def S(x):
    return dr.pack_scalars(x)


def frozen(a):
    a.setflags(write=False)
    return a


def rows_differ(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return np.nonzero((got.reshape(len(want), -1) != want.reshape(len(want), -1)).any(axis=1))[0][:8].tolist()


def dev_call(ctx, fn, ins, outs, n, stream=None):
    """uploads `ins` (arrays or None), runs fn(*input pointers, n, *output pointers, stream) on zeroed outputs of the byte sizes
    `outs` with 64 sentinel bytes behind each, syncs -> the outputs"""
    import torch
    dev = torch.device("cuda", 0)
    d_in = [None if a is None else torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(dev) for a in ins]
    d_out = [torch.full((s + 64,), 0xEE, dtype=torch.uint8, device=dev) for s in outs]
    torch.cuda.synchronize()   # the arrays above were filled on torch's stream; the library launches on its own
    fn(*[None if t is None else t.data_ptr() for t in d_in], n, *[t.data_ptr() for t in d_out], stream=stream or 0)
    ctx.sync()
    if stream:
        torch.cuda.synchronize()
    res = [t.cpu().numpy() for t in d_out]
    for r, s in zip(res, outs):
        assert (r[s:] == 0xEE).all()
    return [r[:s] for r, s in zip(res, outs)]


@pytest.fixture(scope="module")
def be(oracle):
    return dr.CBackend(oracle)


@pytest.fixture(scope="module")
def world(be, golden):
    return dr.world(be, [ints(t) for t in golden["gpu_expected"]["torsion_points"]])


# ---- bjj_mul_pair -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair_case(be, world):
    """NMAX items: the directed set, then seeded random ones -> the five input arrays, the model's (out, ok), the names"""
    d = dr.pair_directed(be, world)
    r = dr.random_pair(be, world, NMAX - len(d[0]), 0xD1F0)
    Pp, a, Qp, b, A = (list(d[i]) + list(r[i]) for i in range(5))
    out, ok = dr.mul_pair(be, Pp, a, Qp, b, A)
    assert ok.count(2) == 6 and len(Pp) == NMAX
    return {"in": [frozen(x) for x in (P(Pp), S(a), P(Qp), S(b), P(A))], "out": frozen(P(out)), "ok": frozen(np.array(ok, np.uint8)),
            "names": d[5]}


@pytest.mark.parametrize("form", ["host", "dev"])
def test_mul_pair_against_the_model(gpu_ctx, pair_case, form):
    c = pair_case
    for n in SIZES:
        ins = [x[:n] for x in c["in"]]
        if form == "host":
            out, ok = gpu_ctx.mul_pair(ins[0], ins[1], ins[2], ins[3], add=ins[4])
        else:
            out, ok = dev_call(gpu_ctx, gpu_ctx.mul_pair_dev, ins, [n * 64, n], n)
        assert not rows_differ(out, c["out"][:n]) and (np.asarray(ok) == c["ok"][:n]).all(), (form, n, rows_differ(out, c["out"][:n]))
    # add_xy == NULL is the identity
    idn = np.nonzero((c["in"][4] == P([dr.IDENTITY])).all(axis=1))[0]
    assert idn.size >= 8
    ins = [np.ascontiguousarray(x[idn]) for x in c["in"][:4]]
    out, ok = gpu_ctx.mul_pair(*ins) if form == "host" else dev_call(gpu_ctx, gpu_ctx.mul_pair_dev, ins + [None], [idn.size * 64, idn.size], idn.size)
    assert not rows_differ(out, c["out"][idn]) and (np.asarray(ok) == c["ok"][idn]).all()


def test_mul_pair_against_the_composition(gpu_ctx, pair_case):
    c = pair_case
    Pp, a, Qp, b, A = c["in"]
    out, ok = gpu_ctx.mul_pair(Pp, a, Qp, b, add=A)
    comp = gpu_ctx.point_add(gpu_ctx.point_add(A, gpu_ctx.mul_var_base(Pp, a)), gpu_ctx.mul_var_base(Qp, b))
    on = ok == 1
    assert on.sum() == NMAX - 6 and not rows_differ(out[on], comp[on])
    assert not out[~on].any() and (ok[~on] == 2).all()


# ---- the statements -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def statements(gpu_ctx, be, world):
    made, out = [], {}
    for name, (gname, gw, pw) in SETUPS.items():
        G = dr.B8 if gname is None else world[gname]
        PK, PK2 = be.mul([G, G], [SK % dr.L, SK2])
        g = None if gname is None else gpu_ctx.base(G, gw)
        pk, pk2 = gpu_ctx.base(PK, pw), gpu_ctx.base(PK2, pw)
        made += [x for x in (g, pk, pk2) if x is not None]
        tag = dr.dleq_tag(be, G, PK, LABEL)
        assert int.from_bytes(gpu_ctx.dleq_tag(G, PK, LABEL).tobytes(), "little") == tag       # Context.dleq_tag is the model's tag
        out[name] = dict(G=G, PK=PK, PK2=PK2, g=g, pk=pk, pk2=pk2, tag=tag)
    yield out
    for b in made:
        if b.ctx.handle:
            b.close()


@pytest.fixture(scope="module")
def proofs(be, world, statements):
    """per setup, NMAX items: the directed cases, then the model's proofs for seeded ciphertexts, every eighth of them with one field
    changed -> the five arrays, the model's verdicts (for PK, for the wrong tag, for the wrong key), the names"""
    out = {}
    for name, s in statements.items():
        cases = dr.dleq_directed(be, world, s["G"], SK, SK2, s["tag"])
        rng = random.Random(0xD1F1)
        m = NMAX - len(cases)
        C1 = be.mul([dr.B8] * m, [rng.randrange(1, dr.L) for _ in range(m)])
        w = [rng.getrandbits(256) for _ in range(m)]
        D, A, B, z, ok = dr.dleq_prove(be, s["G"], SK, s["tag"], C1, w)
        assert ok == [1] * m
        for i in range(5, m, 8):
            k = (i // 8) % 5
            if k == 0:
                z[i] ^= 1 << (i % 250)
            elif k == 1:
                A[i] = (A[i][0], A[i][1] ^ (1 << (i % 250)))
            elif k == 2:
                B[i] = B[(i + 1) % m]
            elif k == 3:
                D[i] = be.add([D[i]], [world["s3"]])[0]
            else:
                C1[i] = (C1[i][0] ^ 2, C1[i][1])
        arrays = [[c[j] for c in cases] + list(v) for j, v in zip(range(1, 6), (C1, D, A, B, z))]
        want = dr.dleq_verify(be, s["G"], s["PK"], s["tag"], *arrays)
        for c, v in zip(cases, want):
            assert c[6] is None or c[6] == v, c[0]
        out[name] = {"in": [frozen(P(x)) for x in arrays[:4]] + [frozen(S(arrays[4]))], "ok": frozen(np.array(want, np.uint8)),
                     "ok_tag": np.array(dr.dleq_verify(be, s["G"], s["PK"], (s["tag"] + 1) % dr.Q, *arrays), np.uint8),
                     "ok_pk2": np.array(dr.dleq_verify(be, s["G"], s["PK2"], s["tag"], *arrays), np.uint8), "names": [c[0] for c in cases]}
        assert set(np.unique(want)) == {0, 1, 2} and (want.count(1) > 800)
    return out


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("setup", sorted(SETUPS))
def test_dleq_verify_against_the_model(gpu_ctx, statements, proofs, setup, form):
    s, c = statements[setup], proofs[setup]

    def run(pk, tag, ins, n):
        if form == "host":
            return gpu_ctx.dleq_verify(pk, tag, *ins, g=s["g"])
        return dev_call(gpu_ctx, lambda *a, stream=0: gpu_ctx.dleq_verify_dev(pk, tag, *a, g=s["g"], stream=stream), ins, [n], n)[0]
    for n in SIZES:
        ok = run(s["pk"], s["tag"], [x[:n] for x in c["in"]], n)
        bad = np.nonzero(ok != c["ok"][:n])[0][:8].tolist()
        assert not bad, (form, n, bad, [c["names"][i] for i in bad if i < len(c["names"])])
    assert (run(s["pk"], (s["tag"] + 1) % dr.Q, c["in"], NMAX) == c["ok_tag"]).all() and not (c["ok_tag"] == 1).any()       # a wrong tag
    assert (run(s["pk2"], s["tag"], c["in"], NMAX) == c["ok_pk2"]).all() and not (c["ok_pk2"] == 1).any()                  # the wrong PK table
    if s["tag"] + dr.Q <= dr.M256:
        assert (run(s["pk"], s["tag"] + dr.Q, c["in"], NMAX) == c["ok"]).all()                                            # the tag is reduced mod r


# ---- bjj_dleq_prove -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prove_case(be, world, statements):
    rng = random.Random(0xD1F2)
    C1 = be.mul([dr.B8] * NMAX, [rng.randrange(1, dr.L) for _ in range(NMAX)])
    w = [rng.getrandbits(256) for _ in range(NMAX)]
    w[:4] = [0, dr.L, dr.M256, dr.ORDER8 - 1]
    C1[5], C1[6], C1[7], C1[8] = world["off"], (0, 0), world["big"], world["full"]
    C1[700], C1[999] = world["off_y"], world["torsion"][3]
    out = {}
    for name, s in statements.items():
        want = dr.dleq_prove(be, s["G"], SK, s["tag"], C1, w)
        out[name] = [frozen(P(want[0])), frozen(P(want[1])), frozen(P(want[2])), frozen(S(want[3])), frozen(np.array(want[4], np.uint8))]
    return {"c1": frozen(P(C1)), "w": frozen(S(w)), "want": out, "off": [5, 6, 700], "outside": [8, 999]}


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("setup", sorted(SETUPS))
def test_dleq_prove_against_the_model_and_round_trip(gpu_ctx, statements, prove_case, setup, form):
    s, c = statements[setup], prove_case
    want = c["want"][setup]
    for n in SIZES:
        if form == "host":
            got = gpu_ctx.dleq_prove(SK, s["tag"], c["c1"][:n], c["w"][:n], g=s["g"])
        else:
            got = dev_call(gpu_ctx, lambda *a, stream=0: gpu_ctx.dleq_prove_dev(SK, s["tag"], *a, g=s["g"], stream=stream),
                           [c["c1"][:n], c["w"][:n]], [n * 64, n * 64, n * 64, n * 32, n], n)
        for k, (g_, w_) in enumerate(zip(got, want)):
            assert not rows_differ(g_, w_[:n]), (form, n, k, rows_differ(g_, w_[:n]))
    D, A, B, z, ok = gpu_ctx.dleq_prove(SK % dr.L, s["tag"], c["c1"], c["w"], g=s["g"])         # sk >= l is sk mod l
    assert all(not rows_differ(g_, w_) for g_, w_ in zip((D, A, B, z, ok), want))
    # the round trip: every proof of a ciphertext in the subgroup is accepted; an off-curve C1 is 2 on both sides
    v = gpu_ctx.dleq_verify(s["pk"], s["tag"], c["c1"], D, A, B, z, g=s["g"])
    sound = np.ones(NMAX, bool)
    sound[c["off"] + c["outside"]] = False
    assert (v[sound] == 1).all() and (v[c["off"]] == 2).all() and (ok[c["off"]] == 2).all() and (ok[sound] == 1).all()
    assert (gpu_ctx.in_subgroup(c["c1"])[sound] == 1).all()
    # the prover's D is what bjj_elgamal_decrypt subtracts: bjj_mul_common(sk, C1)
    Dc, okc = gpu_ctx.mul_common(SK % dr.L, c["c1"])
    assert not rows_differ(D, Dc) and (ok == okc).all()


# ---- the forms agree -------------------------------------------------------------------------------------------------------------------
def test_pinned_and_pageable_host_arrays_give_identical_results(gpu_ctx, statements, pair_case, proofs, prove_case):
    s, lib, h = statements["gen13_pk5"], gpu_ctx.lib, gpu_ctx.handle
    n = NMAX
    g, pk = s["g"].handle.value, s["pk"].handle.value
    tag = np.frombuffer(dr.le(s["tag"]), np.uint8).copy()
    sk = np.frombuffer(dr.le(SK), np.uint8).copy()
    calls = [
        (lambda i, o: lib.bjj_mul_pair(h, i[0], i[1], i[2], i[3], i[4], n, o[0], o[1]), pair_case["in"], [n * 64, n],
         [pair_case["out"], pair_case["ok"]]),
        (lambda i, o: lib.bjj_dleq_verify(h, g, pk, tag.ctypes.data, i[0], i[1], i[2], i[3], i[4], n, o[0]), proofs["gen13_pk5"]["in"], [n],
         [proofs["gen13_pk5"]["ok"]]),
        (lambda i, o: lib.bjj_dleq_prove(h, g, sk.ctypes.data, tag.ctypes.data, i[0], i[1], n, o[0], o[1], o[2], o[3], o[4]),
         [prove_case["c1"], prove_case["w"]], [n * 64, n * 64, n * 64, n * 32, n], prove_case["want"]["gen13_pk5"]),
    ]
    for fn, ins, outs, want in calls:
        for pinned in (False, True):
            bufs = [gpu_ctx.host_empty(x.size) if pinned else np.empty(x.size, np.uint8) for x in ins]
            res = [gpu_ctx.host_empty(sz) if pinned else np.empty(sz, np.uint8) for sz in outs]
            try:
                for b_, x in zip(bufs, ins):
                    b_[:] = x.reshape(-1)
                for r in res:
                    r[:] = 0xEE
                assert all(bool(gpu_ctx.host_is_pinned(b_)) == pinned for b_ in bufs + res)
                assert fn([b_.ctypes.data for b_ in bufs], [r.ctypes.data for r in res]) == 0, lib.bjj_last_error()
                for r, w_ in zip(res, want):
                    assert (np.asarray(r) == np.asarray(w_).reshape(-1)).all(), pinned
            finally:
                if pinned:
                    for b_ in bufs + res:
                        gpu_ctx.host_free(b_)


def test_a_non_default_stream(gpu_ctx, statements, pair_case, proofs, prove_case):
    import torch
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    s, n = statements["b8_pk12"], 257
    out, ok = dev_call(gpu_ctx, gpu_ctx.mul_pair_dev, [x[:n] for x in pair_case["in"]], [n * 64, n], n, stream=st.cuda_stream)
    assert not rows_differ(out, pair_case["out"][:n]) and (ok == pair_case["ok"][:n]).all()
    c = proofs["b8_pk12"]
    v = dev_call(gpu_ctx, lambda *a, stream=0: gpu_ctx.dleq_verify_dev(s["pk"], s["tag"], *a, g=s["g"], stream=stream), [x[:n] for x in c["in"]], [n], n,
                 stream=st.cuda_stream)[0]
    assert (v == c["ok"][:n]).all()
    got = dev_call(gpu_ctx, lambda *a, stream=0: gpu_ctx.dleq_prove_dev(SK, s["tag"], *a, g=s["g"], stream=stream),
                   [prove_case["c1"][:n], prove_case["w"][:n]], [n * 64, n * 64, n * 64, n * 32, n], n, stream=st.cuda_stream)
    assert all(not rows_differ(g_, w_[:n]) for g_, w_ in zip(got, prove_case["want"]["b8_pk12"]))


# ---- a second trip of each capped grid ----------------------------------------------------------------------------------------------
def _define(name, text):
    m = re.search(r"^#define %s (\d+)\b" % name, text, flags=re.M)
    assert m, name
    return int(m.group(1))


def test_a_second_trip_of_each_capped_grid(gpu_ctx, statements):
    """The grids, from the sources: bjj_k_mul_pair* and bjj_k_dleq_verify are launched with at most BJJ_DLEQ_BLOCK * BJJ_DLEQ_MIN_BLOCKS
    = 512 lanes per CU (their launch bounds leave no room for more), bjj_k_dleq_nonce / bjj_k_dleq_respond with whole BJJ_BLOCK-lane
    workgroups, of which a CU holds at most 2 048 lanes.  So n1 = 512 CUs' worth + 1 items need a second trip of the first two and
    n2 = 2 048 CUs' worth + 1 a second trip of the small kernels (and a fifth of the others).  Expected values: the composition run
    on the GPU, compared on the GPU."""
    import torch
    dev = torch.device("cuda", 0)
    src = open(os.path.join(CSRC, "k_dleq.hip")).read()
    assert _define("BJJ_DLEQ_BLOCK", src) * _define("BJJ_DLEQ_MIN_BLOCKS", src) == 512
    assert "capped_grid(n, BJJ_DLEQ_BLOCK, (size_t)cus * (size_t)(lanes_per_cu / BJJ_DLEQ_BLOCK))" in src
    assert _define("BJJ_BLOCK", open(os.path.join(CSRC, "bjj_launch.hpp")).read()) == 256
    cus = gpu_ctx.info().compute_units
    n1, n2 = cus * 512 + 1, cus * 2048 + 1
    s = statements["gen13_pk5"]
    rng = np.random.default_rng(0xD1F3)
    w = rng.integers(0, 256, size=(n2, 32), dtype=np.uint8)                            # any 256-bit values
    k = rng.integers(0, 256, size=(n2, 32), dtype=np.uint8)
    k[:, 31] &= 0x03
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev)   # noqa: E731
    zeros = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)   # noqa: E731
    d_w, d_k = up(w), up(k)
    d_c1 = zeros(n2 * 64)
    torch.cuda.synchronize()   # the arrays above were filled on torch's stream; the library launches on its own
    gpu_ctx.mul_fixed_base_dev(d_k.data_ptr(), n2, d_c1.data_ptr())                   # the ciphertexts' C1 = k B8
    gpu_ctx.sync()

    # bjj_mul_pair at n1: P = C1, Q = the next item's C1, A = the item after; a = w, b = k
    d_q, d_a = torch.roll(d_c1, -64), torch.roll(d_c1, -128)
    d_t1, d_t2, d_s1, d_want = (zeros(n1 * 64) for _ in range(4))
    d_out, d_ok = zeros(n1 * 64 + 64), zeros(n1 + 64)
    torch.cuda.synchronize()
    gpu_ctx.mul_var_base_dev(d_c1.data_ptr(), d_w.data_ptr(), n1, d_t1.data_ptr())
    gpu_ctx.mul_var_base_dev(d_q.data_ptr(), d_k.data_ptr(), n1, d_t2.data_ptr())
    gpu_ctx.point_add_dev(d_a.data_ptr(), d_t1.data_ptr(), n1, d_s1.data_ptr())
    gpu_ctx.point_add_dev(d_s1.data_ptr(), d_t2.data_ptr(), n1, d_want.data_ptr())
    gpu_ctx.mul_pair_dev(d_c1.data_ptr(), d_w.data_ptr(), d_q.data_ptr(), d_k.data_ptr(), d_a.data_ptr(), n1, d_out.data_ptr(), d_ok.data_ptr())
    gpu_ctx.sync()
    assert bool((d_out[:n1 * 64] == d_want).all()) and bool((d_ok[:n1] == 1).all())
    assert not bool(d_out[n1 * 64:].any()) and not bool(d_ok[n1:].any())
    del d_q, d_a, d_t1, d_t2, d_s1, d_want, d_out

    # bjj_dleq_prove at n2 against its parts: D by bjj_mul_common, A by bjj_mul_bases, B by bjj_mul_var_base over w mod l, the hash by
    # bjj_poseidon5 twice; z in integers on the host
    wl = [v % dr.L for v in dr.unpack_scalars(w)]
    d_wl = up(S(wl))
    d_D, d_A, d_B, d_z = zeros(n2 * 64 + 64), zeros(n2 * 64 + 64), zeros(n2 * 64 + 64), zeros(n2 * 32 + 64)
    d_ok = zeros(n2 + 64)
    e_D, e_A, e_B, e_ok = zeros(n2 * 64), zeros(n2 * 64), zeros(n2 * 64), zeros(n2)
    torch.cuda.synchronize()
    gpu_ctx.dleq_prove_dev(SK, s["tag"], d_c1.data_ptr(), d_w.data_ptr(), n2, d_D.data_ptr(), d_A.data_ptr(), d_B.data_ptr(), d_z.data_ptr(),
                           d_ok.data_ptr(), g=s["g"])
    gpu_ctx.mul_common_dev(SK % dr.L, d_c1.data_ptr(), None, n2, e_D.data_ptr(), e_ok.data_ptr())
    gpu_ctx.mul_bases_dev([s["g"]], [d_wl.data_ptr()], n2, e_A.data_ptr())
    gpu_ctx.mul_var_base_dev(d_c1.data_ptr(), d_wl.data_ptr(), n2, e_B.data_ptr())
    gpu_ctx.sync()
    assert bool((d_D[:n2 * 64] == e_D).all()) and bool((d_A[:n2 * 64] == e_A).all()) and bool((d_B[:n2 * 64] == e_B).all())
    assert bool((d_ok[:n2] == 1).all()) and not any(bool(t[m:].any()) for t, m in ((d_D, n2 * 64), (d_A, n2 * 64), (d_B, n2 * 64), (d_z, n2 * 32), (d_ok, n2)))
    tagrec = torch.from_numpy(np.frombuffer(dr.le(s["tag"]), np.uint8).copy()).to(dev)
    h_in = torch.cat([tagrec.repeat(n2, 1), d_c1.view(n2, 64), e_D.view(n2, 64)], dim=1).contiguous()
    d_h, d_c = zeros(n2 * 32), zeros(n2 * 32)
    torch.cuda.synchronize()
    gpu_ctx.poseidon5_dev(h_in.data_ptr(), n2, d_h.data_ptr())
    gpu_ctx.sync()
    h_in = torch.cat([d_h.view(n2, 32), e_A.view(n2, 64), e_B.view(n2, 64)], dim=1).contiguous()
    torch.cuda.synchronize()
    gpu_ctx.poseidon5_dev(h_in.data_ptr(), n2, d_c.data_ptr())
    gpu_ctx.sync()
    skl = SK % dr.L
    want_z = S([(a_ + (c_ % dr.L) * skl) % dr.L for a_, c_ in zip(wl, dr.unpack_scalars(d_c.cpu().numpy()))])
    z = d_z[:n2 * 32].cpu().numpy().reshape(n2, 32)
    assert not rows_differ(z, want_z)

    # bjj_dleq_verify at n2: every proof above is accepted; with one bit of z flipped in every seventh item, those and only those are not
    d_v = zeros(n2 + 64)
    torch.cuda.synchronize()
    gpu_ctx.dleq_verify_dev(s["pk"], s["tag"], d_c1.data_ptr(), d_D.data_ptr(), d_A.data_ptr(), d_B.data_ptr(), d_z.data_ptr(), n2, d_v.data_ptr(),
                            g=s["g"])
    gpu_ctx.sync()
    assert bool((d_v[:n2] == 1).all()) and not bool(d_v[n2:].any())
    d_z.view(-1)[3:n2 * 32:7 * 32] ^= 0x10
    torch.cuda.synchronize()
    gpu_ctx.dleq_verify_dev(s["pk"], s["tag"], d_c1.data_ptr(), d_D.data_ptr(), d_A.data_ptr(), d_B.data_ptr(), d_z.data_ptr(), n2, d_v.data_ptr(),
                            g=s["g"])
    gpu_ctx.sync()
    v = d_v[:n2].cpu().numpy()
    assert (v[0::7] == 0).all() and (np.delete(v, np.arange(0, n2, 7)) == 1).all() and (v[cus * 512:] == (np.arange(cus * 512, n2) % 7 != 0)).all()


# ---- rejections with a live context ------------------------------------------------------------------------------------------------
def test_rejections(gpu_ctx, ctx_w23, statements, pair_case, proofs, prove_case):
    import babyjubjub_rs_amd as bjj
    from babyjubjub_rs_amd import _lib
    lib, h, E = gpu_ctx.lib, gpu_ctx.handle, _lib.BJJ_E_INVALID
    s, n = statements["gen13_pk5"], 65
    g, pk = s["g"].handle.value, s["pk"].handle.value
    foreign = ctx_w23.base(s["PK"], 5)
    gone = gpu_ctx.base(s["PK2"], 4)
    stale = gone.handle.value
    gone.close()
    ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
    pin = [np.ascontiguousarray(x[:n]) for x in pair_case["in"]]
    vin = [np.ascontiguousarray(x[:n]) for x in proofs["gen13_pk5"]["in"]]
    c1, w = np.ascontiguousarray(prove_case["c1"][:n]), np.ascontiguousarray(prove_case["w"][:n])
    tag, sk = np.frombuffer(dr.le(s["tag"]), np.uint8).copy(), np.frombuffer(dr.le(SK), np.uint8).copy()
    o = [np.full(n * 64, 0xEE, np.uint8) for _ in range(4)]
    ok = np.full(n, 0xEE, np.uint8)
    try:
        with pytest.raises(bjj.BjjError):
            gpu_ctx.dleq_verify(gone, s["tag"], *vin)
        with pytest.raises(bjj.BjjError):
            gpu_ctx.dleq_verify(None, s["tag"], *vin)
        with pytest.raises(bjj.BjjError):
            gpu_ctx.dleq_prove(SK, s["tag"], c1, w, g=gone)
        for k in range(4):                                                                    # a NULL array (add_xy alone may be NULL)
            a = [ptr(x) for x in pin]
            a[k] = None
            assert lib.bjj_mul_pair(h, *a, n, ptr(o[0]), ptr(ok)) == E
        assert lib.bjj_mul_pair(h, *[ptr(x) for x in pin], n, None, ptr(ok)) == E
        assert lib.bjj_mul_pair(h, *[ptr(x) for x in pin], n, ptr(o[0]), None) == E
        assert lib.bjj_mul_pair(h, *[ptr(x) for x in pin], 1 << 32, ptr(o[0]), ptr(ok)) == E
        v = [ptr(x) for x in vin]
        assert lib.bjj_dleq_verify(h, g, None, ptr(tag), *v, n, ptr(ok)) == E and b"pk is NULL" in lib.bjj_last_error()
        assert lib.bjj_dleq_verify(h, g, stale, ptr(tag), *v, n, ptr(ok)) == E
        assert lib.bjj_dleq_verify(h, stale, pk, ptr(tag), *v, n, ptr(ok)) == E
        assert lib.bjj_dleq_verify(h, g, foreign.handle.value, ptr(tag), *v, n, ptr(ok)) == E and b"not a base of this context" in lib.bjj_last_error()
        assert lib.bjj_dleq_verify(h, g, pk, None, *v, n, ptr(ok)) == E and b"tag is NULL" in lib.bjj_last_error()
        assert lib.bjj_dleq_verify(h, g, pk, ptr(tag), *v, n, None) == E
        for k in range(5):
            a = list(v)
            a[k] = None
            assert lib.bjj_dleq_verify(h, g, pk, ptr(tag), *a, n, ptr(ok)) == E
        outs = [ptr(x) for x in o[:3]] + [ptr(o[3])]
        assert lib.bjj_dleq_prove(h, stale, ptr(sk), ptr(tag), ptr(c1), ptr(w), n, *outs, ptr(ok)) == E
        assert lib.bjj_dleq_prove(h, g, None, ptr(tag), ptr(c1), ptr(w), n, *outs, ptr(ok)) == E and b"sk is NULL" in lib.bjj_last_error()
        assert lib.bjj_dleq_prove(h, g, ptr(sk), None, ptr(c1), ptr(w), n, *outs, ptr(ok)) == E
        assert lib.bjj_dleq_prove(h, g, ptr(sk), ptr(tag), None, ptr(w), n, *outs, ptr(ok)) == E
        assert lib.bjj_dleq_prove(h, g, ptr(sk), ptr(tag), ptr(c1), None, n, *outs, ptr(ok)) == E
        assert lib.bjj_dleq_prove(h, g, ptr(sk), ptr(tag), ptr(c1), ptr(w), n, *outs, None) == E
        for k in range(4):
            a = list(outs)
            a[k] = None
            assert lib.bjj_dleq_prove(h, g, ptr(sk), ptr(tag), ptr(c1), ptr(w), n, *a, ptr(ok)) == E
        # n == 0: nothing is looked at
        assert lib.bjj_mul_pair(h, None, None, None, None, None, 0, None, None) == 0
        assert lib.bjj_dleq_verify(h, g, pk, ptr(tag), None, None, None, None, None, 0, None) == 0
        assert lib.bjj_dleq_prove(h, g, ptr(sk), ptr(tag), None, None, 0, None, None, None, None, None) == 0
        assert all((x == 0xEE).all() for x in o) and (ok == 0xEE).all()
        # _dev: a misaligned array is refused, d_ok may sit at any address
        import torch
        dev = torch.device("cuda", 0)
        d = [torch.from_numpy(np.concatenate([x.reshape(-1), np.zeros(16, np.uint8)])).to(dev) for x in pin]
        d_out, d_ok = torch.full((n * 64 + 16,), 0xEE, dtype=torch.uint8, device=dev), torch.full((n + 16,), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        p = [t.data_ptr() for t in d]
        for k in range(5):
            a = list(p)
            a[k] += 8
            assert lib.bjj_mul_pair_dev(h, *a, n, d_out.data_ptr(), d_ok.data_ptr(), None) == E, k
        assert lib.bjj_mul_pair_dev(h, *p, n, d_out.data_ptr() + 8, d_ok.data_ptr(), None) == E
        assert lib.bjj_mul_pair_dev(h, *p, n, d_out.data_ptr(), None, None) == E
        gpu_ctx.sync()
        assert bool((d_out == 0xEE).all()) and bool((d_ok == 0xEE).all())
        assert lib.bjj_mul_pair_dev(h, *p, n, d_out.data_ptr(), d_ok.data_ptr() + 1, None) == 0
        gpu_ctx.sync()
        got_ok = d_ok.cpu().numpy()
        assert got_ok[0] == 0xEE and (got_ok[1:n + 1] == pair_case["ok"][:n]).all() and (got_ok[n + 1:] == 0xEE).all()
        assert (d_out.cpu().numpy()[:n * 64].reshape(n, 64) == pair_case["out"][:n]).all()
    finally:
        foreign.close()


# ---- overlapping launches, and the other users of the per-lane table block ---------------------------------------------------------
def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(torch.device("cuda", 0))


def _zeros(sizes):
    import torch
    return [torch.zeros(s, dtype=torch.uint8, device=torch.device("cuda", 0)) for s in sizes]


def _ptrs(tensors):
    return [None if t is None else t.data_ptr() for t in tensors]


def _same(outs, want, what):
    for k, (o, w_) in enumerate(zip(outs, want)):
        w_ = np.ascontiguousarray(w_).reshape(-1).view(np.uint8)
        bad = np.nonzero(o.cpu().numpy() != w_)[0]
        assert bad.size == 0, (what, k, bad[:8].tolist())


def _dleq_launches(ctx, statements, pair_case, proofs, prove_case, n):
    """name -> (enqueue(outputs, stream), output sizes in bytes, the model's arrays) for the three _dev entry points on the first n
    items of the module's cases, the inputs uploaded once (the closures keep them alive)"""
    d_pair = [_up(x[:n]) for x in pair_case["in"]]
    d_c1, d_w = _up(prove_case["c1"][:n]), _up(prove_case["w"][:n])
    out = {"pair": (lambda o, st: ctx.mul_pair_dev(*_ptrs(d_pair), n, *_ptrs(o), stream=st), [n * 64, n],
                    [pair_case["out"][:n], pair_case["ok"][:n]])}
    for name, s in statements.items():
        d_v = [_up(x[:n]) for x in proofs[name]["in"]]
        out["verify_" + name] = (lambda o, st, s=s, d_v=d_v: ctx.dleq_verify_dev(s["pk"], s["tag"], *_ptrs(d_v), n, *_ptrs(o), g=s["g"], stream=st),
                                 [n], [proofs[name]["ok"][:n]])
        out["prove_" + name] = (lambda o, st, s=s: ctx.dleq_prove_dev(SK, s["tag"], d_c1.data_ptr(), d_w.data_ptr(), n, *_ptrs(o), g=s["g"], stream=st),
                                [n * 64, n * 64, n * 64, n * 32, n], [w_[:n] for w_ in prove_case["want"][name]])
    return out


def test_two_streams_at_once(gpu_ctx, statements, pair_case, proofs, prove_case):
    """two launches on two streams with nothing between them, three times each pairing: bjj_mul_pair beside bjj_dleq_verify (both size
    and index the per-lane table block of their scratch set), bjj_dleq_prove beside bjj_dleq_verify, and bjj_dleq_prove beside
    bjj_dleq_prove with another G -- the five-launch chain on both scratch sets at once.  Every output against the model at n = NMAX"""
    import torch
    n = NMAX
    L = _dleq_launches(gpu_ctx, statements, pair_case, proofs, prove_case, n)
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(2)]
    for names in (("pair", "verify_gen13_pk5"), ("prove_b8_pk12", "verify_b8_pk12"), ("prove_b8_pk12", "prove_gen13_pk5")):
        outs = [_zeros(L[k][1]) for k in names]
        torch.cuda.synchronize()
        for rep_ in range(3):
            for k, o, st in zip(names, outs, streams):
                L[k][0](o, st.cuda_stream)
            gpu_ctx.sync()
            for k, o in zip(names, outs):
                _same(o, L[k][2], (names, k, rep_))
                for t in o:
                    t.zero_()
            torch.cuda.synchronize()


@pytest.fixture(scope="module")
def other_users(oracle):
    """the entry points that share the per-lane table block with the DLEQ kernels, by the C oracle: 4 097 signatures (1 in 64
    corrupted) with their verdicts, 257 points (one off the curve) and scalars with their products"""
    from babyjubjub_rs_amd import workload as w
    n = 4097
    A, R, S_, msg = w.make_signatures(oracle.mul_fixed_base, oracle.poseidon5, n)
    bad = w.corrupt(A, R, S_, msg, n)
    verdict = oracle.verify(A, R, S_, msg)
    assert (verdict[~bad] == 1).all() and (verdict[bad] != 1).all() and bad[:64].any() and bad[:257].sum() >= 2
    pts, sc = oracle.mul_fixed_base(w.scalars_254(257, offset=0x9d)).copy(), w.scalars_254(257, offset=0x5c)
    pts[32, 7] ^= 4                                                     # off the curve: the exact kernel's item, in both sizes used
    vb = oracle.mul_var_base(pts, sc)
    return {"sig": [frozen(x) for x in (A, R, S_, msg)], "verdict": frozen(verdict), "pts": frozen(pts), "sc": frozen(sc), "vb": frozen(vb)}


def _other_launches(ctx, other_users, nv, nb):
    """(enqueue(outputs, stream), sizes, expected) for bjj_eddsa_verify_dev on nv signatures and bjj_mul_var_base_dev on nb points"""
    u = other_users
    d_sig = [_up(x[:nv]) for x in u["sig"]]
    d_vb = [_up(u["pts"][:nb]), _up(u["sc"][:nb])]
    return {"eddsa": (lambda o, st: ctx.eddsa_verify_dev(*_ptrs(d_sig), nv, *_ptrs(o), stream=st), [nv], [u["verdict"][:nv]]),
            "var_base": (lambda o, st: ctx.mul_var_base_dev(*_ptrs(d_vb), nb, *_ptrs(o), stream=st), [nb * 64], [u["vb"][:nb]])}


def test_back_to_back_with_the_other_users_of_the_table_block(gpu_ctx, statements, pair_case, proofs, prove_case, other_users):
    """bjj_dleq.inc sizes the per-lane table block for cus * lanes_dleq lanes whatever n is, and says "K2 and verify use a prefix":
    on ONE stream, with no synchronisation in between, bjj_mul_pair, bjj_eddsa_verify, bjj_dleq_verify, bjj_mul_var_base,
    bjj_dleq_prove and bjj_mul_pair again at n = 257, each against its known result"""
    import torch
    n = 257
    L = dict(_dleq_launches(gpu_ctx, statements, pair_case, proofs, prove_case, n), **_other_launches(gpu_ctx, other_users, n, n))
    order = ("pair", "eddsa", "verify_gen13_pk5", "var_base", "prove_gen13_pk5", "pair")
    outs = [_zeros(L[k][1]) for k in order]
    torch.cuda.synchronize()
    for k, o in zip(order, outs):
        L[k][0](o, 0)
    gpu_ctx.sync()
    for i, (k, o) in enumerate(zip(order, outs)):
        _same(o, L[k][2], (i, k))


def test_first_call_of_a_fresh_context_is_dleq(statements, pair_case, proofs, other_users):
    """the growth orders tests/test_gpu_scratch_growth.py predates DLEQ for: in a context of its own the FIRST call is bjj_mul_pair at
    n = 1 (the table block is sized by the DLEQ rule before any other user has touched it), then bjj_eddsa_verify at 4 097,
    bjj_dleq_verify at 64 and bjj_mul_var_base at 65, each against its known result"""
    import torch
    import babyjubjub_rs_amd as bjj
    ctx = bjj.Context(0, 16)
    try:
        def run(launch):
            fn, sizes, want = launch
            o = _zeros(sizes)
            torch.cuda.synchronize()
            fn(o, 0)
            ctx.sync()
            return o, want

        d_pair = [_up(x[:1]) for x in pair_case["in"]]
        o, want = run((lambda o, st: ctx.mul_pair_dev(*_ptrs(d_pair), 1, *_ptrs(o), stream=st), [64, 1], [pair_case["out"][:1], pair_case["ok"][:1]]))
        _same(o, want, "mul_pair at 1")
        others = _other_launches(ctx, other_users, 4097, 65)
        o, want = run(others["eddsa"])
        _same(o, want, "eddsa_verify at 4097")
        s, c = statements["b8_pk12"], proofs["b8_pk12"]                 # G = B8: the context's own table; PK's table is made here
        pk = ctx.base(s["PK"], SETUPS["b8_pk12"][2])
        d_v = [_up(x[:64]) for x in c["in"]]
        o, want = run((lambda o, st: ctx.dleq_verify_dev(pk, s["tag"], *_ptrs(d_v), 64, *_ptrs(o), stream=st), [64], [c["ok"][:64]]))
        _same(o, want, "dleq_verify at 64")
        assert set(np.unique(c["ok"][:64])) == {0, 1, 2}
        o, want = run(others["var_base"])
        _same(o, want, "mul_var_base at 65")
    finally:
        ctx.close()
