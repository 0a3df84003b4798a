"""Parity of the HIP path (through the C ABI of libbjj_hip.so) with the oracle: bit-exact on
every output byte.  Needs a real MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest

from conftest import pack, unpack
from dispatch_forms import LANE, SHORT, both, lane_ctx, ran  # noqa: F401  (lane_ctx: the fixture)

pytestmark = pytest.mark.gpu

Q = 21888242871839275222246405745257275088548364400416034343698204186575808495617
L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
ORDER = 8 * L


def hexint(x):
    return int(x, 16) if isinstance(x, str) else int(x)


def rows(cases, key):
    return pack([tuple(c[key]) if isinstance(c[key], (list, tuple)) else c[key] for c in cases])


# ---------------------------------------------------------------- golden fixtures
# The golden vectors and the seeded batches below are short calls: the session's context runs them on the several-lanes-per-item
# kernels of k_small.hip, `lane_ctx` on the one-item-per-lane kernels; every test says which form each call took.
def test_golden_fixed_base(gpu_ctx, lane_ctx, golden):  # noqa: F811
    fb = golden["oracle_vectors"]["fixed_base"]
    for ctx, form in both(gpu_ctx, lane_ctx):
        got = ctx.mul_fixed_base(rows(fb, "n"))
        ran(ctx, "fixed", form)
        assert (got.reshape(-1) == rows(fb, "out")).all()


def test_golden_var_base_incl_off_curve(gpu_ctx, lane_ctx, golden):  # noqa: F811
    vb = golden["oracle_vectors"]["var_base"]
    assert any(not c["on_curve"] for c in vb) and any(c["on_curve"] for c in vb)
    for ctx, form in both(gpu_ctx, lane_ctx):
        got = ctx.mul_var_base(rows(vb, "p"), rows(vb, "n"))
        ran(ctx, "var", form)
        want = rows(vb, "out").reshape(-1, 64)
        bad = [i for i in range(len(vb)) if (got[i] != want[i]).any()]
        assert not bad, (form, [vb[i] for i in bad[:3]])


def test_golden_poseidon(gpu_ctx, lane_ctx, golden):  # noqa: F811
    ps = golden["oracle_vectors"]["poseidon5"] + [
        {"in": c["in"], "out": c["out"]} for c in golden["reference_kats"]["poseidon_public"]["cases"]]
    for ctx, form in both(gpu_ctx, lane_ctx):
        got = ctx.poseidon5(rows(ps, "in"))
        ran(ctx, "poseidon", form)
        assert (got.reshape(-1) == rows(ps, "out")).all()


def test_golden_point_add(gpu_ctx, golden):
    ad = golden["oracle_vectors"]["point_add"]
    got = gpu_ctx.point_add(rows(ad, "p"), rows(ad, "q"))
    assert (got.reshape(-1) == rows(ad, "out")).all()


def test_golden_verify_edge_semantics(gpu_ctx, lane_ctx, golden):  # noqa: F811
    ve = golden["oracle_vectors"]["verify"]
    for ctx, form in both(gpu_ctx, lane_ctx):
        got = ctx.eddsa_verify(rows(ve, "pk"), rows(ve, "r_b8"), rows(ve, "s"), rows(ve, "msg"))
        ran(ctx, "verify", form)
        for c, g in zip(ve, got):
            assert bool(g) == c["ok"], (form, c["note"])


# ---------------------------------------------------------------- seeded random vs oracle
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4096])
def test_fixed_base_random_and_ragged(gpu_ctx, lane_ctx, oracle, n):  # noqa: F811
    from babyjubjub_rs_amd import workload
    sc = workload.random_u256(workload.SEED_SCALARS, n)  # full 256-bit scalars (unreduced)
    want = oracle.mul_fixed_base(sc)
    for ctx, form in both(gpu_ctx, lane_ctx):
        got = ctx.mul_fixed_base(sc)
        ran(ctx, "fixed", form)
        assert (got == want).all(), form


def test_empty_batches(gpu_ctx):
    e = np.zeros(0, np.uint8)
    assert gpu_ctx.mul_fixed_base(e).shape == (0, 64)
    assert gpu_ctx.mul_var_base(e, e).shape == (0, 64)
    assert gpu_ctx.poseidon5(e).shape == (0, 32)
    assert gpu_ctx.eddsa_verify(e, e, e, e).shape == (0,)


def _points(oracle, golden, n, seed):
    """cfg-3 points: k*B8 + c*T8 (whole group incl. torsion), via the C oracle; the 8 torsion points are a fixture."""
    from babyjubjub_rs_amd import workload
    from conftest import ints
    ks = workload.random_u256(seed, n)
    base = oracle.mul_fixed_base(ks)
    tors = [ints(t) for t in golden["gpu_expected"]["torsion_points"]]
    cs = workload.splitmix64(seed ^ 0x55, n) & np.uint64(7)
    tp = pack([tors[int(c)] for c in cs]).reshape(n, 64)
    return oracle.point_add(base, tp)


def test_var_base_random_full_group(gpu_ctx, lane_ctx, oracle, golden):  # noqa: F811
    from babyjubjub_rs_amd import workload
    n = 1536
    pts = _points(oracle, golden, n, workload.SEED_POINTS)
    sc = workload.random_u256(workload.SEED_SCALARS, n, offset=100)
    # edge rows: identity, order-2 point, off-curve garbage, zero scalar, huge scalars
    pts[0] = pack([(0, 1)]); pts[1] = pack([(0, Q - 1)]); pts[2] = 7; pts[3] = 0
    sc[4] = 0; sc[5] = 255; sc[6] = pack([ORDER]); sc[7] = pack([L])
    want = oracle.mul_var_base(pts, sc)
    for ctx, form in both(gpu_ctx, lane_ctx):
        got = ctx.mul_var_base(pts, sc)
        ran(ctx, "var", form)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (form, bad[:8])


def test_poseidon_random(gpu_ctx, lane_ctx, oracle):  # noqa: F811
    from babyjubjub_rs_amd import workload
    n = 4096
    a = workload.random_u256(workload.SEED_MSGS, 5 * n).reshape(n, 160)  # values >= r are reduced on both sides
    want = oracle.poseidon5(a)
    for ctx, form in both(gpu_ctx, lane_ctx):
        got = ctx.poseidon5(a)
        ran(ctx, "poseidon", form)
        assert (got == want).all(), form


from babyjubjub_rs_amd.workload import make_signatures, corrupt  # noqa: E402  (the cfg-4 generator lives with the other workloads)


def test_verify_random_with_corruption(gpu_ctx, lane_ctx, oracle):  # noqa: F811
    n = 2048
    A, R, S, msg = make_signatures(oracle.mul_fixed_base, oracle.poseidon5, n)
    bad = corrupt(A, R, S, msg, n)
    assert bad.sum() > 8
    want = oracle.verify(A, R, S, msg)
    for ctx, form in both(gpu_ctx, lane_ctx):
        got = ctx.eddsa_verify(A, R, S, msg)
        ran(ctx, "verify", form)
        assert (got == want).all(), form
        assert (got[~bad] == 1).all() and (got[bad] == 0).all()


def test_verify_msg_range_rule(gpu_ctx, lane_ctx, oracle, golden):  # noqa: F811
    """msg > Q -> false; msg == Q accepted and hashed as 0 (src/lib.rs:396-399)."""
    from conftest import ints
    c = golden["gpu_expected"]["msg_range_signature"]           # a valid signature of msg = 0 (tests/golden/make_gpu_expected.py)
    A, R, S = ints(c["A"]), ints(c["R"]), ints(c["S"])
    msgs = [0, Q, Q + 1, (1 << 256) - 1, Q - 1]
    n = len(msgs)
    for ctx, form in both(gpu_ctx, lane_ctx):
        got = ctx.eddsa_verify(pack([A] * n), pack([R] * n), pack([S] * n), pack(msgs))
        ran(ctx, "verify", form)
        assert list(got) == [1, 1, 0, 0, 0], form
    assert list(oracle.verify(pack([A] * n), pack([R] * n), pack([S] * n), pack(msgs))) == [1, 1, 0, 0, 0]


@pytest.mark.parametrize("window_bits", [4, 8, 13, 19])
def test_fixed_base_other_window_widths(oracle, window_bits):
    """the table geometry is a tuning knob; results must not depend on it (13 does not divide 256)."""
    import babyjubjub_rs_amd as bjj
    from babyjubjub_rs_amd import workload
    from dispatch_forms import make_lane_ctx
    for form in (SHORT, LANE):                                  # 777 and 130 items are short calls: both kernels over each table
        ctx = bjj.Context(0, window_bits) if form == SHORT else make_lane_ctx(window_bits)
        try:
            info = ctx.info()
            assert info.window_bits == window_bits and info.n_windows == -(-252 // window_bits)
            assert info.table_bytes == info.n_windows * ((1 << (window_bits - 1)) + 1) * 128
            assert ctx.check_table() == 0   # every entry, by induction from B8, on the device
            sc = workload.random_u256(workload.SEED_SCALARS, 777, offset=5)
            sc[0] = 255
            assert (ctx.mul_fixed_base(sc) == oracle.mul_fixed_base(sc)).all()
            ran(ctx, "fixed", form)
            A, R, S, msg = make_signatures(oracle.mul_fixed_base, oracle.poseidon5, 130)
            S[3, 0] ^= 1
            assert (ctx.eddsa_verify(A, R, S, msg) == oracle.verify(A, R, S, msg)).all()
            ran(ctx, "verify", form)
        finally:
            ctx.close()


def test_fixed_base_table_is_sound_and_signed_digit_edges(gpu_ctx, oracle):
    """default-width table verified entry by entry on the device; scalars that stress the signed recoding
    (digits at +-2^(W-1), carry runs, values around l and 2^256) against the oracle."""
    assert gpu_ctx.check_table() == 0
    W = gpu_ctx.info().window_bits
    l, half = L, 1 << (W - 1)
    nw = 252 // W
    cases = [0, 1, half, half + 1, (1 << W) - 1, 1 << W, l - 1, l, l + 1, 2 * l - 1, 8 * l, (1 << 256) - 1, (1 << 251) - 1,
             (1 << 251), sum(half << (W * j) for j in range(nw)) % l, sum((half + 1) << (W * j) for j in range(nw)),
             sum(((1 << W) - 1) << (W * j) for j in range(0, nw, 2)), l - half, l + half]
    sc = pack([c % (1 << 256) for c in cases])
    got = gpu_ctx.mul_fixed_base(sc)
    ran(gpu_ctx, "fixed", SHORT)                                # 19 items: four lanes per item
    assert (got == oracle.mul_fixed_base(sc)).all()
    assert unpack(got[0].tobytes(), 2)[0] == (0, 1) and unpack(got[7].tobytes(), 2)[0] == (0, 1)
    # the same scalars over the same table on K1, the kernel of the large calls: tiled past the short-call threshold of 2^15 items
    reps = (1 << 15) // len(cases) + 1
    tiled = gpu_ctx.mul_fixed_base(np.tile(sc.reshape(-1, 32), (reps, 1)))
    ran(gpu_ctx, "fixed", LANE)
    assert (tiled == np.tile(got, (reps, 1))).all()


def test_batches_beyond_2_to_the_31_bytes(gpu_ctx, oracle):
    """2^25 + 777 items: output offsets pass 2^31 bytes (64-bit index arithmetic), items are not a multiple of the
    grid, of a 64-item chunk or of the host pipeline's 2^18-item chunks.  Sampled against the oracle, first/last/
    around the 2^25 boundary included, for the host-pointer (pipelined) and the device-pointer API."""
    import torch
    from babyjubjub_rs_amd import workload
    n = (1 << 25) + 777
    sc = workload.random_u256(workload.SEED_SCALARS, n, offset=11)
    rng = np.random.default_rng(5)
    idx = np.unique(np.concatenate([[0, 1, (1 << 18) - 1, 1 << 18, (1 << 25) - 1, 1 << 25, n - 2, n - 1], rng.integers(0, n, 2000)]))
    want = oracle.mul_fixed_base(np.ascontiguousarray(sc[idx]))
    got = gpu_ctx.mul_fixed_base(sc)
    assert got.shape == (n, 64) and (got[idx] == want).all()
    del got
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream()
    d_sc = torch.from_numpy(sc.reshape(-1)).to(dev)
    d_out = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    gpu_ctx.mul_fixed_base_dev(d_sc.data_ptr(), n, d_out.data_ptr(), st.cuda_stream)
    st.synchronize()
    got = d_out.view(n, 64)[torch.from_numpy(idx).to(dev)].cpu().numpy()
    assert (got == want).all()
    # verify at the same size: A = R = s*B8-shaped junk is enough to exercise indexing; expectation from the oracle
    del d_out
    m = (1 << 22) + 333
    A, R, S, msg = make_signatures(oracle.mul_fixed_base, oracle.poseidon5, 4096)
    reps = -(-m // 4096)
    tile = lambda a: np.ascontiguousarray(np.tile(a, (reps, 1))[:m])
    At, Rt, St, Mt = tile(A), tile(R), tile(S), tile(msg)
    bad = rng.integers(0, m, 500)
    St[bad, 0] ^= 1
    ok = gpu_ctx.eddsa_verify(At, Rt, St, Mt)
    expect = np.ones(m, np.uint8); expect[bad] = 0
    assert (ok == expect).all()


def test_independent_contexts_on_concurrent_threads(oracle):
    """bjj_hip.h threading contract: different contexts are independent.  Four host threads, each with its own
    context (own stream, scratch, table), hammer different entry points at the same time (ctypes drops the GIL)."""
    import threading
    import babyjubjub_rs_amd as bjj
    from babyjubjub_rs_amd import workload
    n = 20000
    sc = workload.random_u256(workload.SEED_SCALARS, n, offset=21)
    pts = oracle.mul_fixed_base(workload.random_u256(workload.SEED_POINTS, n, offset=21))
    A, R, S, msg = make_signatures(oracle.mul_fixed_base, oracle.poseidon5, 3000)
    S[::7, 1] ^= 2
    pin = np.concatenate([R, A, msg], axis=1)
    want = {"fixed": oracle.mul_fixed_base(sc), "var": oracle.mul_var_base(pts, sc), "verify": oracle.verify(A, R, S, msg),
            "poseidon": oracle.poseidon5(pin)}
    errors = []

    def worker(kind):
        try:
            ctx = bjj.Context(0, 14)
            try:
                for _ in range(4):
                    got = {"fixed": lambda: ctx.mul_fixed_base(sc), "var": lambda: ctx.mul_var_base(pts, sc),
                           "verify": lambda: ctx.eddsa_verify(A, R, S, msg), "poseidon": lambda: ctx.poseidon5(pin)}[kind]()
                    if not (got == want[kind]).all():
                        errors.append(kind + ": mismatch")
            finally:
                ctx.close()
        except Exception as e:  # noqa: BLE001 - surfaced through the assertion below
            errors.append("%s: %r" % (kind, e))

    ts = [threading.Thread(target=worker, args=(k,)) for k in ("fixed", "var", "verify", "poseidon")]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert errors == []


def test_automatic_window_width_and_second_context(gpu_ctx, oracle):
    """BJJ_WINDOW_AUTO picks the widest table that fits in 60 % of the free device memory: the session's context got
    28 bits (154.6 GB) on an empty MI355X, a second automatic context next to it must settle for a narrower table
    (never fail), verify its own table, and agree bit for bit -- also through the cooperative gathers of the verify and
    sign kernels, with batch sizes that leave partially filled waves."""
    import babyjubjub_rs_amd as bjj
    from babyjubjub_rs_amd import workload
    first = gpu_ctx.info()
    assert first.window_bits in (28, 26, 23, 21, 16) and first.n_windows == -(-252 // first.window_bits)
    ctx = bjj.Context(0, bjj.WINDOW_AUTO)
    try:
        info = ctx.info()
        assert info.window_bits in (26, 23, 21, 16) or first.window_bits < 28
        assert info.table_bytes == info.n_windows * ((1 << (info.window_bits - 1)) + 1) * 128
        assert ctx.check_table() == 0
        for n in (1, 63, 65, 1000):
            sc = workload.random_u256(workload.SEED_SCALARS, n, offset=900 + n)
            want = oracle.mul_fixed_base(sc)
            assert (ctx.mul_fixed_base(sc) == want).all() and (gpu_ctx.mul_fixed_base(sc) == want).all()
        A, R, S, msg = make_signatures(oracle.mul_fixed_base, oracle.poseidon5, 193)
        S[5, 0] ^= 1
        msg[7] = 0xff                                   # msg > Q in the middle of a wave: verdict 0, neighbours unaffected
        want = oracle.verify(A, R, S, msg)
        assert (ctx.eddsa_verify(A, R, S, msg) == want).all() and (gpu_ctx.eddsa_verify(A, R, S, msg) == want).all()
        keys = workload.random_u256(workload.SEED_KEYS, 67, offset=3)
        m = workload.random_u256(workload.SEED_MSGS, 67, offset=3, top_bits_cleared=3)
        m[11] = 0xff                                    # Err item inside a wave of the sign kernel
        r0, s0, ok0 = oracle.sign(keys, m)
        for c in (ctx, gpu_ctx):
            r1, s1, ok1 = c.sign(keys, m)
            assert (ok1 == ok0).all() and (r1 == r0).all() and (s1 == s0).all()
    finally:
        ctx.close()


# ---------------------------------------------------------------- device-pointer API
def test_device_pointer_api_and_streams(gpu_ctx, oracle):
    import torch
    from babyjubjub_rs_amd import workload, BjjError
    dev = torch.device("cuda:0")
    n = 5000
    sc = workload.scalars_254(n)
    d_sc = torch.from_numpy(sc.reshape(-1)).to(dev)
    d_out = torch.empty(n * 64, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream()
    gpu_ctx.reserve(n)
    torch.cuda.synchronize()
    gpu_ctx.mul_fixed_base_dev(d_sc.data_ptr(), n, d_out.data_ptr(), st.cuda_stream)
    st.synchronize()
    want = oracle.mul_fixed_base(sc)
    assert (d_out.cpu().numpy().reshape(n, 64) == want).all()
    # variable base on the results, default (context) stream
    d_out2 = torch.empty(n * 64, dtype=torch.uint8, device=dev)
    gpu_ctx.mul_var_base_dev(d_out.data_ptr(), d_sc.data_ptr(), n, d_out2.data_ptr(), 0)
    gpu_ctx.sync()
    assert (d_out2.cpu().numpy().reshape(n, 64) == oracle.mul_var_base(want, sc)).all()
    # misaligned / NULL device pointers are rejected
    with pytest.raises(BjjError):
        gpu_ctx.mul_fixed_base_dev(d_sc.data_ptr() + 4, n - 1, d_out.data_ptr(), 0)
    with pytest.raises(BjjError):
        gpu_ctx.mul_fixed_base_dev(0, n, d_out.data_ptr(), 0)


# ---------------------------------------------------------------- full-size properties (BASELINE sizes)
def test_full_size_fixed_base_1m(gpu_ctx, oracle):
    """cfg 2 at 2^20: (i) strided sample byte-compared with the oracle, (ii) linearity over the whole
    batch: a*B8 + b*B8 == ((a + b) mod 8l)*B8, (iii) the variable-base kernel on P = B8 agrees."""
    from babyjubjub_rs_amd import workload as w
    n = 1 << 20
    a = w.scalars_254(n)
    ga = gpu_ctx.mul_fixed_base(a)
    idx = np.arange(0, n, 997)
    assert (ga[idx] == oracle.mul_fixed_base(a[idx])).all()
    b = np.roll(a, 1, axis=0)
    gb = np.roll(ga, 1, axis=0)
    a64 = a.view("<u8").reshape(n, 4).astype(object)
    b64 = b.view("<u8").reshape(n, 4).astype(object)
    summed = [(int(x[0]) | int(x[1]) << 64 | int(x[2]) << 128 | int(x[3]) << 192) +
              (int(y[0]) | int(y[1]) << 64 | int(y[2]) << 128 | int(y[3]) << 192) for x, y in zip(a64, b64)]
    gs = gpu_ctx.mul_fixed_base(w.from_ints([s % ORDER for s in summed]))
    assert (gpu_ctx.point_add(ga, gb) == gs).all()
    m = 1 << 17
    b8 = np.tile(pack([(5299619240641551281634865583518297030282874472190772894086521144482721001553,
                        16950150798460657717958625567821834550301663161624707787222815936182638968203)]), (m, 1))
    assert (gpu_ctx.mul_var_base(b8, a[:m]) == ga[:m]).all()


def test_full_size_verify_1m(gpu_ctx, oracle):
    """cfg 4 at 2^20: signatures synthesised with the GPU kernels themselves (a strided sample of
    every intermediate is checked against the oracle), 1/64 corrupted; the verdict vector must equal
    the known corruption mask, and a strided sample must equal the oracle's verdicts."""
    n = 1 << 20
    A, R, S, msg = make_signatures(gpu_ctx.mul_fixed_base, gpu_ctx.poseidon5, n)
    idx = np.arange(0, n, 4099)
    Ao, Ro, So, mo = make_signatures(oracle.mul_fixed_base, oracle.poseidon5, idx.size)  # offset 0 prefix
    assert (A[:idx.size] == Ao).all() and (R[:idx.size] == Ro).all() and (S[:idx.size] == So).all()
    bad = corrupt(A, R, S, msg, n)
    got = gpu_ctx.eddsa_verify(A, R, S, msg)
    assert (got == (~bad).astype(np.uint8)).all()
    assert (got[idx] == oracle.verify(A[idx], R[idx], S[idx], msg[idx])).all()


def test_config0_bench_point_1k_scalars(gpu_ctx, lane_ctx, oracle, golden):  # noqa: F811
    """BASELINE.json configs[0]: benches/bench_babyjubjub.rs:15-38 -- mul_scalar on the bench point with
    1 000 random 254-bit scalars (SURVEY.md 8d cfg 1) plus the two literal criterion scalars."""
    from babyjubjub_rs_amd import workload as w
    b = golden["reference_kats"]["bench_inputs"]
    n = 1000
    sc = w.scalars_254(n)
    sc = np.concatenate([sc, pack(b["scalars"]).reshape(-1, 32)])
    pts = np.tile(pack([tuple(b["p"])]), (sc.shape[0], 1))
    got = gpu_ctx.mul_var_base(pts, sc)
    ran(gpu_ctx, "var", SHORT)
    assert (got == oracle.mul_var_base(pts, sc)).all()
    assert (lane_ctx.mul_var_base(pts, sc) == got).all()        # the same call on K2, the kernel of the large calls
    ran(lane_ctx, "var", LANE)
    import hashlib
    # the digest is printed so a maintainer can compare runs / boxes; the byte comparison above is the test
    print("cfg0 output sha256:", hashlib.sha256(got.tobytes()).hexdigest())


def test_verify_small_order_and_torsion_cases(gpu_ctx, lane_ctx, oracle, golden):  # noqa: F811
    """verdicts that hinge on the cofactor: pk of small order (8*hm*pk vanishes, so s*B8 == R decides),
    R or pk shifted by torsion points, s beyond l.  The GPU path multiplies the check by a short ODD v,
    which must not change any of these verdicts (verify).  96 signatures are a short call: the session's
    context runs the eight-lanes-per-signature kernel (last_verify_dispatch 2), so the same call goes to a context created with
    BJJ_VERIFY_SMALL_MAX=0 as well, which runs K4 (0 or 1), the kernel of the large calls; every verdict is asserted for both."""
    from babyjubjub_rs_amd import workload as w
    from conftest import ints
    tors = [ints(t) for t in golden["gpu_expected"]["torsion_points"]]   # the 8 points of order dividing 8 (j * T8)
    assert tors[0] == (0, 1) and tors[4] == (0, Q - 1)
    n = 96
    s_int = [v % (8 * L) for v in w.to_ints(w.random_u256(0x7075, n))]
    sB = oracle.mul_fixed_base(w.from_ints(s_int))
    msg = w.random_u256(0x7076, n, 0, top_bits_cleared=3)
    pk, R, S, want_true = [], [], [], []
    for i in range(n):
        t1, t2 = tors[i % 8], tors[(i // 8) % 8]
        sb = unpack(sB[i], 2)[0]
        if i % 3 == 0:      # small-order pk, R = s*B8           -> true
            pk.append(t1); R.append(sb); want_true.append(True)
        elif i % 3 == 1:    # small-order pk, R = s*B8 + torsion -> true only if the shift is the identity
            shifted = unpack(oracle.point_add(pack([sb]), pack([t2]))[0], 2)[0]     # s*B8 + torsion, src/lib.rs:88-131, 70-85
            pk.append(t1); R.append(shifted); want_true.append(t2 == (0, 1))
        else:               # random pk: just compare with the oracle
            pk.append(unpack(sB[(i + 1) % n], 2)[0]); R.append(sb); want_true.append(None)
        S.append(s_int[i])
    want = oracle.verify(pack(pk), pack(R), pack(S), msg)
    for ctx, form in both(gpu_ctx, lane_ctx):
        got = ctx.eddsa_verify(pack(pk), pack(R), pack(S), msg)
        assert ctx.info().last_verify_dispatch == 2 if form == SHORT else ctx.info().last_verify_dispatch in (0, 1), form
        assert (got == want).all(), form
        for i, wt in enumerate(want_true):
            if wt is not None:
                assert bool(got[i]) == wt, (form, i)
        assert got.sum() >= n // 3
