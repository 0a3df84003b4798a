"""The newer kernels at sizes where their size-dependent machinery engages more than once (every other file stops below that):

1. bjj_mul_bases, bjj_*_verify_signer, bjj_*_verify_set -- grid-strided loops over a grid capped at the resident lanes: n1 = R + 1
   and n3 = 2 R + 65 items, R = compute_units * 512, so the loop runs a second and a third trip, the last one a full wave plus one
   lane of a ragged wave, and the running product of bjj_k_mul_bases spans up to three items per lane.
2. bjj_mul_common / bjj_in_subgroup / bjj_elgamal_decrypt -- compute_units * 2048 + 65 items: more workgroups than K2's slot queue has
   slots, so the table form works in recycled slots (release, barrier, push; a later workgroup's pop), in both scratch sets.
3. bjj_point_sum -- three and four levels: the launcher's ping-pong of the two entry lists goes past level 1 and back into e0.

Expected values: for EVERY item the library's oracle-tested composition on the same inputs (bjj_mul_var_base + bjj_point_add, the generic
verifiers with the key replicated or gathered, bjj_msm_batch / bjj_msm), and the C oracle on a subset (beyond_cases.oracle_subset:
the whole last trip, the first 64 items of every trip, every 257th item, 2 048 seeded ones).  The whole of n1 does NOT go to the
oracle, the subset does: measured on the CPU, the oracle's mul_var_base (the bases tests need three such products), verify and
verify_schnorr over 131 073 items each stay well above the 5 s on 16 CPUs that would have allowed it.
Every large array is built once per module, on the GPU where the library has a producer; every output buffer starts as a sentinel."""
import os
import re
import time

import numpy as np
import pytest

import beyond_cases as bc
from bases_cases import ORDER8
from conftest import ROOT, ints, pack
from test_gpu_common_scalar import context_with_form
from test_gpu_msm import IDENTITY
from test_gpu_msm_batch import offsets_of
from test_gpu_point_sum import T, _dev_call, by_msm_batch, ok_sum, signs, unit_scalars

pytestmark = pytest.mark.gpu

Q, L = bc.Q, bc.L
B8 = bc.sc.B8
CSRC = os.path.join(ROOT, "babyjubjub-rs_amd", "csrc")
LDS_PER_CU = 160 * 1024            # gfx950
SENTINEL = 0xEE
UMAX = (1 << 64) - 1
FULL = 0x2A6D5E0F1B3C7A9948D1C0E2F3B4A59687766554433221100FFEEDDCCBBAA998


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _define(name, text):
    m = re.search(r"^#define %s (\d+)\b" % name, text, flags=re.M)
    assert m, name
    return int(m.group(1))


def resident_lanes_bound(block):
    """the most lanes per CU of a kernel that stages two table entries per lane in LDS (GatherCoopLds<2>: 2 x FB_STAGE_WORDS words
    per wave), in whole workgroups of `block` lanes"""
    assert "#define FB_STAGE_WORDS (64 * NIELS_WORDS)" in _src("k_common.hpp")
    niels_words = int(re.search(r"^constexpr int NIELS_WORDS = (\d+);", _src("bjj_device.hpp"), flags=re.M).group(1))
    per_workgroup = (block // 64) * 2 * 64 * niels_words * 4
    return (LDS_PER_CU // per_workgroup) * block


def rep(rec, n):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(rec, np.uint8).reshape(1, -1), (n, np.asarray(rec).size)))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))


def sentinel(nbytes, guard=64):
    import torch
    return torch.full((nbytes + guard,), SENTINEL, dtype=torch.uint8, device=torch.device("cuda", 0))


def fetch(d_buf, nbytes, width):
    """the first nbytes of a device buffer as (n, width) records; the guard bytes behind them must still be the sentinel"""
    h = d_buf.cpu().numpy()
    assert (h[nbytes:] == SENTINEL).all()
    return h[:nbytes].reshape(-1, width) if width > 1 else h[:nbytes]


def rows_differ(got, want):
    return np.nonzero((got != want).reshape(len(want), -1).any(axis=1))[0]


def same(got, want, what):
    bad = rows_differ(got, want)
    assert got.shape == want.shape and bad.size == 0, (what, bad.size, bad[:8].tolist())


@pytest.fixture(scope="module")
def grid(gpu_ctx):
    """(compute units, R, n1, n3)"""
    cus = gpu_ctx.info().compute_units
    R = cus * 512
    print("\n[grid] %d compute units: R = %d, n1 = %d, n3 = %d" % (cus, R, R + 1, 2 * R + 65))
    return cus, R, R + 1, 2 * R + 65


def check_trips(grid, block):
    """the precondition of group 1, from info() and the sources: at most R lanes are resident, so n1 items need a second trip and n3 a
    third, whose 65 items are one full wave and one lane of a second"""
    cus, R, n1, n3 = grid
    assert resident_lanes_bound(block) == 512 and cus * resident_lanes_bound(block) == R
    assert n1 > R and [hi - lo for lo, hi in bc.trips(n1, R)] == [R, 1]
    assert n3 > 2 * R and [hi - lo for lo, hi in bc.trips(n3, R)] == [R, R, 65]


@pytest.fixture(scope="module")
def tors(golden):
    t = pack([ints(p) for p in golden["gpu_expected"]["torsion_points"]]).reshape(8, 64)    # j * T8
    t.setflags(write=False)
    return t


# ---- 1a: bjj_mul_bases ----------------------------------------------------------------------------------------------------------------
COMBOS = {"custom": ("c",), "null": (None,), "null_custom": (None, "c")}


@pytest.fixture(scope="module")
def bases_case(gpu_ctx, oracle, grid, tors):
    """a custom point k * B8 + T with a torsion component, two scalar arrays of n3 items with the directed scalars in every trip, the
    products of both points by bjj_mul_var_base, and the C oracle's products on the subset"""
    from babyjubjub_rs_amd import workload as w
    cus, R, n1, n3 = grid
    custom = oracle.point_add(oracle.mul_fixed_base(w.random_u256(w.SEED_POINTS ^ 0xB1D, 1)), tors[3:4])
    S = [bc.placed_scalars(n3, R, (16,), 0xB1D0), np.roll(bc.placed_scalars(n3, R, (16,), 0xB1D1), 5, axis=0)]
    point = {None: pack([B8]).reshape(1, 64), "c": custom}
    sub = bc.oracle_subset(n3, R, 0xB1D2)
    by_gpu, by_oracle = {}, {}
    for j, name in ((0, None), (0, "c"), (1, "c")):
        by_gpu[(name, j)] = gpu_ctx.mul_var_base(rep(point[name], n3), S[j])
        by_oracle[(name, j)] = oracle.mul_var_base(rep(point[name], sub.size), S[j][sub])
        same(by_gpu[(name, j)][sub], by_oracle[(name, j)], ("the yardstick against the oracle", name, j))
    for a in S + list(by_gpu.values()) + list(by_oracle.values()):
        a.setflags(write=False)
    table = gpu_ctx.base(custom, 16)
    yield {"S": S, "d_S": [dev(s) for s in S], "sub": sub, "gpu": by_gpu, "oracle": by_oracle, "table": table}
    table.close()


@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_mul_bases_second_and_third_trip(gpu_ctx, oracle, grid, bases_case, combo):
    cus, R, n1, n3 = grid
    assert _define("BJJ_EPI_BLOCK", _src("bjj_launch.hpp")) == 512 and re.search(r"^#define BJJ_BASES_BLOCK BJJ_EPI_BLOCK\b", _src("k_bases.hip"), flags=re.M)
    check_trips(grid, 512)
    c = bases_case
    spec = COMBOS[combo]
    bases = [None if b is None else c["table"] for b in spec]
    terms = [c["gpu"][(b, j)] for j, b in enumerate(spec)]
    want = terms[0] if len(terms) == 1 else gpu_ctx.point_add(terms[0], terms[1])
    oterms = [c["oracle"][(b, j)] for j, b in enumerate(spec)]
    owant = oterms[0] if len(oterms) == 1 else oracle.point_add(oterms[0], oterms[1])
    sub = c["sub"]
    same(want[sub], owant, (combo, "the yardstick against the oracle"))
    # n3: three trips
    d_out = sentinel(n3 * 64)
    gpu_ctx.mul_bases_dev(bases, [c["d_S"][j].data_ptr() for j in range(len(spec))], n3, d_out.data_ptr())
    gpu_ctx.sync()
    got = fetch(d_out, n3 * 64, 64)
    same(got, want, (combo, "n3"))
    same(got[sub], owant, (combo, "n3, oracle"))
    # n1 from item 7 on: two trips, the second one is the single item R + 7, a directed scalar; lane k now holds item k + 7
    d_out = sentinel(n1 * 64)
    gpu_ctx.mul_bases_dev(bases, [c["d_S"][j].data_ptr() + 7 * 32 for j in range(len(spec))], n1, d_out.data_ptr())
    gpu_ctx.sync()
    got = fetch(d_out, n1 * 64, 64)
    same(got, want[7:7 + n1], (combo, "n1"))
    in1 = sub[(sub >= 7) & (sub < 7 + n1)]
    assert R + 7 in in1
    same(got[in1 - 7], owant[np.searchsorted(sub, in1)], (combo, "n1, oracle"))
    if combo == "null_custom":                             # the host form, once
        got = gpu_ctx.mul_bases(bases, [c["S"][j][7:7 + n1] for j in range(len(spec))])
        same(got, want[7:7 + n1], (combo, "n1, host form"))


# ---- 1b: the signer kernels --------------------------------------------------------------------------------------------------------
def _sign(ctx, keys, msgs, schnorr, seed):
    """valid signatures by the library's signers -> R (n, 64), S (n, 32)"""
    n = len(msgs)
    if not schnorr:
        r, s, ok = ctx.sign(keys, msgs)
        assert ok.all()
        return r.copy(), s.copy()
    nonces = np.random.default_rng(seed).integers(0, 256, size=(n, 128), dtype=np.uint8)
    r, s, ok = ctx.sign_schnorr(keys, msgs, nonces)
    assert ok.all()
    b = s.tobytes()
    red = b"".join((int.from_bytes(b[i:i + 160], "little") % ORDER8).to_bytes(32, "little") for i in range(0, len(b), 160))
    return r.copy(), np.frombuffer(red, np.uint8).reshape(n, 32).copy()


def _signed_and_corrupted(ctx, grid, keys, schnorr, seed, last_kind):
    from babyjubjub_rs_amd import workload as w
    cus, R, n1, n3 = grid
    msgs = w.random_u256(w.SEED_MSGS ^ seed, n3, top_bits_cleared=3)
    plan = bc.corruption_plan(n3, R, last_kind)
    for lo, hi in bc.trips(n3, R):                         # every kind in every trip; the one item of the ragged wave is corrupted
        assert bc.kinds_in(plan, lo, hi) == set(range(len(bc.KINDS))), (lo, hi)
    assert plan[n3 - 1] == last_kind and (n3 - 1) % 64 == 0
    Rp, S = _sign(ctx, keys, bc.messages_to_sign(msgs, plan), schnorr, seed)
    M = msgs.copy()
    bc.corrupt(Rp, S, M, plan)
    return Rp, S, M, plan


def _check_verdicts(want, plan, n):
    """the INPUTS are what they claim: most items valid, 1 in 8 not, and the kinds whose outcome is beyond doubt have it"""
    assert int((want == 1).sum()) > n // 2 and int((want != 1).sum()) > n // 16
    rows = {k: np.asarray([i for i, v in plan.items() if bc.KINDS[v] == k]) for k in bc.KINDS}
    for k in ("msg=Q", "R.x+r"):
        assert (want[rows[k]] == 1).all(), k
    for k in ("flip s", "flip msg", "flip R.x", "flip R.y", "R=(0,0)", "s=2^256-1"):
        assert (want[rows[k]] == 0).all(), k


@pytest.fixture(scope="module")
def signer_case(gpu_ctx, oracle, grid):
    """schnorr -> n3 signatures under ONE key (bjj_sign / bjj_sign_schnorr), 1 in 8 corrupted, the verdicts of the generic verifier
    with the key replicated, and the C oracle's on the subset; the key's table at W = 16"""
    from babyjubjub_rs_amd import workload as w
    cus, R, n1, n3 = grid
    key = w.random_u256(w.SEED_KEYS ^ 0x51B, 1)
    pk = gpu_ctx.public_keys(key).copy()
    table = gpu_ctx.base(pk, 16)
    sub = bc.oracle_subset(n3, R, 0x51B2)
    cache = {}

    def get(schnorr):
        if schnorr not in cache:
            Rp, S, M, plan = _signed_and_corrupted(gpu_ctx, grid, rep(key, n3), schnorr, 0x51B0 + schnorr,
                                                   bc.MSG_ABOVE_Q if schnorr else bc.OFF_CURVE_R)
            want = (gpu_ctx.schnorr_verify if schnorr else gpu_ctx.eddsa_verify)(rep(pk, n3), Rp, S, M)
            owant = (oracle.verify_schnorr if schnorr else oracle.verify)(rep(pk, sub.size), Rp[sub], S[sub], M[sub])
            same(want[sub], owant, ("the yardstick against the oracle", schnorr))
            _check_verdicts(want, plan, n3)
            assert want[n3 - 1] == (2 if schnorr else 0)
            cache[schnorr] = {"in": (Rp, S, M), "d_in": [dev(a) for a in (Rp, S, M)], "want": want, "owant": owant}
        return cache[schnorr]
    yield {"get": get, "table": table, "sub": sub}
    table.close()


@pytest.mark.parametrize("schnorr", [False, True], ids=["eddsa", "schnorr"])
def test_verify_signer_second_and_third_trip(gpu_ctx, grid, signer_case, schnorr):
    cus, R, n1, n3 = grid
    assert _define("BJJ_SIGNER_BLOCK", _src("k_signer.hip")) == 256
    check_trips(grid, 256)
    c = signer_case["get"](schnorr)
    base, sub = signer_case["table"], signer_case["sub"]
    fn = gpu_ctx.schnorr_verify_signer_dev if schnorr else gpu_ctx.eddsa_verify_signer_dev
    d_r, d_s, d_m = c["d_in"]
    d_ok = sentinel(n3, 16)
    fn(base, d_r.data_ptr(), d_s.data_ptr(), d_m.data_ptr(), n3, d_ok.data_ptr())
    gpu_ctx.sync()
    got = fetch(d_ok, n3, 1)
    same(got, c["want"], (schnorr, "n3"))
    same(got[sub], c["owant"], (schnorr, "n3, oracle"))
    # the last n1 items: two trips, the second one is the corrupted last item alone
    lo = n3 - n1
    d_ok = sentinel(n1, 16)
    fn(base, d_r.data_ptr() + lo * 64, d_s.data_ptr() + lo * 32, d_m.data_ptr() + lo * 32, n1, d_ok.data_ptr())
    gpu_ctx.sync()
    got = fetch(d_ok, n1, 1)
    same(got, c["want"][lo:], (schnorr, "n1"))
    same(got[sub[sub >= lo] - lo], c["owant"][sub >= lo], (schnorr, "n1, oracle"))
    Rp, S, M = c["in"]
    got = (base.verify_schnorr if schnorr else base.verify)(Rp[lo:], S[lo:], M[lo:])     # the host form, once
    same(got, c["want"][lo:], (schnorr, "n1, host form"))


# ---- 1c: the signer-set kernels ------------------------------------------------------------------------------------------------------
SET_K, SET_W, BAD_INDEX = 65, 4, 3


@pytest.fixture(scope="module")
def set_case(gpu_ctx, oracle, grid):
    """65 keys (bjj_public_keys; record 3 holds x + r, record 5 repeats record 0), n3 items under uniform indices signed by the
    index's key, corrupted as for one signer, out-of-range indices in every trip and in the ragged wave; the verdicts of the generic
    verifier with the records gathered by index, 3 for an index outside the set"""
    from babyjubjub_rs_amd import workload as w
    cus, R, n1, n3 = grid
    priv = w.random_u256(w.SEED_KEYS ^ 0x5E7, SET_K)
    records = gpu_ctx.public_keys(priv).copy()
    records[3, :32] = np.frombuffer((int.from_bytes(records[3, :32].tobytes(), "little") + Q).to_bytes(32, "little"), np.uint8)
    records[5] = records[0]
    owner = np.arange(SET_K)
    owner[5] = 0
    sset = gpu_ctx.signer_set(records, SET_W)
    sub = bc.oracle_subset(n3, R, 0x5E72)
    outside = {7: SET_K, 63: SET_K + 1, 64: (1 << 32) - 1, R - 1: SET_K, R: SET_K, R + 1: (1 << 32) - 1, R + 70: SET_K + 1,
               2 * R - 1: SET_K, 2 * R: SET_K + 1, 2 * R + 63: (1 << 32) - 1, n3 - 1: SET_K}
    for lo, hi in bc.trips(n3, R):
        assert sum(lo <= i < hi for i in outside) >= 3
    assert n3 - 1 in outside and int(np.isin(sorted(outside), sub).sum()) >= 6         # the oracle's subset meets some in every trip too
    cache = {}

    def get(schnorr):
        if schnorr not in cache:
            idx = np.random.default_rng(0x5E70 + schnorr).integers(0, SET_K, n3).astype(np.uint32)
            assert len(set(idx[:64].tolist())) > 24 and len(set(idx.tolist())) == SET_K     # many signers within one wave
            Rp, S, M, plan = _signed_and_corrupted(gpu_ctx, grid, priv[owner[idx]], schnorr, 0x5E74 + schnorr, bc.OFF_CURVE_R)
            pk = np.ascontiguousarray(records[idx])
            want = (gpu_ctx.schnorr_verify if schnorr else gpu_ctx.eddsa_verify)(pk, Rp, S, M)
            owant = (oracle.verify_schnorr if schnorr else oracle.verify)(pk[sub], Rp[sub], S[sub], M[sub])
            same(want[sub], owant, ("the yardstick against the oracle", schnorr))
            _check_verdicts(want, plan, n3)
            for j in (3, 5):                               # the unreduced record and the repeated one verify like any other
                own = idx == j
                assert own.sum() > 1000 and (want[own] == 1).sum() > own.sum() // 2
            rows = np.asarray(sorted(outside))
            idx[rows] = [outside[i] for i in rows]
            want[rows] = BAD_INDEX
            owant[np.searchsorted(sub, rows[np.isin(rows, sub)])] = BAD_INDEX
            cache[schnorr] = {"in": (idx, Rp, S, M), "d_in": [dev(a) for a in (idx, Rp, S, M)], "want": want, "owant": owant}
        return cache[schnorr]
    yield {"get": get, "set": sset, "sub": sub, "outside": outside}
    sset.close()


@pytest.mark.parametrize("schnorr", [False, True], ids=["eddsa", "schnorr"])
def test_verify_set_second_and_third_trip(gpu_ctx, grid, set_case, schnorr):
    cus, R, n1, n3 = grid
    assert _define("BJJ_SET_BLOCK", _src("k_signer_set.hip")) == 256
    check_trips(grid, 256)
    c = set_case["get"](schnorr)
    sset, sub = set_case["set"], set_case["sub"]
    assert sset.info()[:2] == (SET_K, SET_W)
    fn = gpu_ctx.schnorr_verify_set_dev if schnorr else gpu_ctx.eddsa_verify_set_dev
    d_i, d_r, d_s, d_m = c["d_in"]
    d_ok = sentinel(n3, 16)
    fn(sset, d_i.data_ptr(), d_r.data_ptr(), d_s.data_ptr(), d_m.data_ptr(), n3, d_ok.data_ptr())
    gpu_ctx.sync()
    got = fetch(d_ok, n3, 1)
    same(got, c["want"], (schnorr, "n3"))
    same(got[sub], c["owant"], (schnorr, "n3, oracle"))
    assert int((got == BAD_INDEX).sum()) == len(set_case["outside"])
    lo = n3 - n1                                           # the last n1 items: the second trip is the last item, whose index is outside the set
    d_ok = sentinel(n1, 16)
    fn(sset, d_i.data_ptr() + lo * 4, d_r.data_ptr() + lo * 64, d_s.data_ptr() + lo * 32, d_m.data_ptr() + lo * 32, n1, d_ok.data_ptr())
    gpu_ctx.sync()
    got = fetch(d_ok, n1, 1)
    same(got, c["want"][lo:], (schnorr, "n1"))
    same(got[sub[sub >= lo] - lo], c["owant"][sub >= lo], (schnorr, "n1, oracle"))
    assert got[-1] == BAD_INDEX
    idx, Rp, S, M = c["in"]
    got = (sset.verify_schnorr if schnorr else sset.verify)(idx[lo:], Rp[lo:], S[lo:], M[lo:])     # the host form, once
    same(got, c["want"][lo:], (schnorr, "n1, host form"))


# ---- 2: slot recycling in bjj_mul_common ---------------------------------------------------------------------------------------------
COMMON_FORMS = ("table", "naf")


@pytest.fixture(scope="module")
def common_ctxs():
    made = {f: context_with_form(f) for f in COMMON_FORMS}
    yield made
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def common_n(gpu_ctx):
    """a CU holds at most 2 048 lanes, whatever the occupancy: compute_units * 2048 + 65 items are more 256-lane workgroups than K2's
    queue has slots (one per workgroup K2 can have resident)"""
    cus = gpu_ctx.info().compute_units
    n = cus * 2048 + 65
    block = _define("BJJ_CS_BLOCK", _src("k_common_scalar.hip"))
    assert block == 256 and -(-n // block) > cus * (2048 // block) and -(-n // block) > cus * 8
    print("\n[common scalar] n = %d: %d workgroups, at most %d slots" % (n, -(-n // block), cus * 8))
    return n


@pytest.fixture(scope="module")
def common_case(gpu_ctx, oracle, golden, common_n):
    """points and addends that cycle through the 16 kinds of tests/test_gpu_common_scalar.py (off-curve items land in every workgroup,
    recycled ones included), the products k * P by bjj_mul_var_base for the full-width k and for l, and the oracle's subset"""
    from babyjubjub_rs_amd import workload as w
    n = common_n
    t = [ints(p) for p in golden["gpu_expected"]["torsion_points"]]
    nontrivial = [p for p in sorted(set(t) | {(0, 1)}) if p != (0, 1)]
    assert len(nontrivial) == 7 and (0, Q - 1) in nontrivial
    sub_pts = gpu_ctx.mul_fixed_base(w.random_u256(w.SEED_POINTS ^ 0xC5, n))
    shifted = gpu_ctx.point_add(sub_pts, pack(nontrivial).reshape(7, 64)[np.arange(n) % 7])
    i = np.arange(n)
    P, p_on = bc.mixed_points(sub_pts, shifted, nontrivial, i)
    A, a_on = bc.mixed_points(np.roll(sub_pts, 1, axis=0), np.roll(shifted, 1, axis=0), nontrivial, 5 * i + 7)
    for arr, on in ((P, p_on), (A, a_on)):                 # the flags against the curve equation, four items of every kind
        for r in list(range(64)) + list(range(n - 64, n)):
            assert bc.on_curve(arr[r]) == bool(on[r]), r
    assert (~p_on).sum() == 2 * (n // 16) + (1 if n % 16 == 15 else 0) and (p_on & ~a_on).sum() > n // 16
    prod = {k: gpu_ctx.mul_var_base(P, rep(pack([k]), n)) for k in (FULL, L)}
    sub = np.unique(np.concatenate([np.arange(0, n, 257), np.arange(n - 321, n)]))
    oprod = {k: oracle.mul_var_base(P[sub], rep(pack([k]), sub.size)) for k in (FULL, L)}
    for k in prod:
        same(prod[k][sub][p_on[sub]], oprod[k][p_on[sub]], ("the yardstick against the oracle", hex(k)))
    for a in (P, A, p_on, a_on, *prod.values(), *oprod.values()):
        a.setflags(write=False)
    return {"P": P, "A": A, "p_on": p_on, "a_on": a_on, "prod": prod, "oprod": oprod, "sub": sub, "d_P": dev(P), "d_A": dev(A)}


def _want_point(add, c, prod, on, with_add, subtract):
    """the rule of test_gpu_common_scalar.want_of: the product, negated for a subtraction, added to the addend; (0, 0) / 2 off the curve"""
    from babyjubjub_rs_amd import api
    t = np.array(prod)
    t[~on["p"]] = 0
    if subtract:
        t = api._negate_x(t)
    if with_add:
        t = add(np.ascontiguousarray(c), t)
    good = on["p"] & (on["a"] if with_add else True)
    out = np.array(t).reshape(-1, 64)
    out[~good] = 0
    return out, np.where(good, 1, 2).astype(np.uint8)


def _twice_then_two_streams(ctx, launch, buffers, check):
    """launch(stream, k) writes into buffers()[k]: twice in a row on one stream, then four calls alternating over two streams with
    no synchronisation between them (the second scratch set: its queue and its tables); check(buffers, what) after each round;
    bjj_sync must report no starved slot queue"""
    import torch
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(2)]
    bufs = buffers()
    torch.cuda.synchronize()
    launch(streams[0].cuda_stream, bufs[0])
    launch(streams[0].cuda_stream, bufs[1])
    assert ctx.lib.bjj_sync(ctx.handle) == 0, ctx.lib.bjj_last_error()
    for b in bufs:
        check(b, "twice in a row")
    bufs = buffers()
    torch.cuda.synchronize()
    for k in range(4):
        launch(streams[k % 2].cuda_stream, bufs[k % 2])
    assert ctx.lib.bjj_sync(ctx.handle) == 0, ctx.lib.bjj_last_error()
    for b in bufs:
        check(b, "two streams")


@pytest.mark.parametrize("case", ["plain", "subtract_from_addend"])
def test_mul_common_recycled_slots(gpu_ctx, oracle, common_ctxs, common_case, common_n, case):
    from babyjubjub_rs_amd import api
    n, c = common_n, common_case
    with_add = subtract = case != "plain"
    on = {"p": c["p_on"], "a": c["a_on"]}
    wout, wok = _want_point(gpu_ctx.point_add, c["A"], c["prod"][FULL], on, with_add, subtract)
    sub = c["sub"]
    osub = {"p": c["p_on"][sub], "a": c["a_on"][sub]}
    oout, ook = _want_point(oracle.point_add, c["A"][sub], c["oprod"][FULL], osub, with_add, subtract)
    same(wout[sub], oout, (case, "the yardstick against the oracle"))
    assert (wok[sub] == ook).all() and int((wok == 2).sum()) > n // 16 and int((wok == 1).sum()) > n // 2
    first = {}
    for form in COMMON_FORMS:
        ctx = common_ctxs[form]

        def launch(stream, b):
            ctx.mul_common_dev(FULL, c["d_P"].data_ptr(), c["d_A"].data_ptr() if with_add else None, n, b[0].data_ptr(), b[1].data_ptr() + 3,
                               subtract, stream=stream)

        def check(b, what):
            out, ok = fetch(b[0], n * 64, 64), b[1].cpu().numpy()
            assert (ok[:3] == SENTINEL).all() and (ok[3 + n:] == SENTINEL).all()
            same(ok[3:3 + n], wok, (case, form, what, "ok"))
            same(out, wout, (case, form, what))
            same(out[sub], oout, (case, form, what, "oracle"))
            first.setdefault(form, (out, ok[3:3 + n].copy()))
        _twice_then_two_streams(ctx, launch, lambda: [(sentinel(n * 64), sentinel(n + 3, 4)) for _ in range(2)], check)
    assert first["table"][0].tobytes() == first["naf"][0].tobytes() and first["table"][1].tobytes() == first["naf"][1].tobytes()


def test_in_subgroup_recycled_slots(oracle, common_ctxs, common_case, common_n):
    n, c = common_n, common_case
    identity = IDENTITY.reshape(-1)
    want = np.where(c["p_on"], (c["prod"][L] == identity).all(axis=1).astype(np.uint8), 2).astype(np.uint8)
    sub = c["sub"]
    owant = np.where(c["p_on"][sub], (c["oprod"][L] == identity).all(axis=1).astype(np.uint8), 2).astype(np.uint8)
    assert (want[sub] == owant).all()
    assert all(int((want == v).sum()) > n // 16 for v in (0, 1, 2))
    first = {}
    for form in COMMON_FORMS:
        ctx = common_ctxs[form]

        def launch(stream, b):
            ctx.in_subgroup_dev(c["d_P"].data_ptr(), n, b.data_ptr() + 1, stream=stream)

        def check(b, what):
            ok = b.cpu().numpy()
            assert ok[0] == SENTINEL and (ok[1 + n:] == SENTINEL).all()
            same(ok[1:1 + n], want, (form, what))
            first.setdefault(form, ok[1:1 + n].copy())
        _twice_then_two_streams(ctx, launch, lambda: [sentinel(n + 1, 4) for _ in range(2)], check)
    assert first["table"].tobytes() == first["naf"].tobytes()


@pytest.fixture(scope="module")
def ciphertexts(gpu_ctx, common_n):
    """(C1, C2) = (r B8, m B8 + r PK) with PK = sk B8 by bjj_mul_fixed_base and bjj_mul_bases({NULL, PK}): m is known by construction;
    off-curve components among the first workgroups and among the last"""
    from babyjubjub_rs_amd import workload as w
    n = common_n
    rng = np.random.default_rng(0xE16C)
    sk = int.from_bytes(rng.bytes(31), "little") % L
    ms = rng.integers(0, 1 << 16, n).astype(np.uint64)
    edge = [0, 1, (1 << 16) - 1, 1 << 15, 63, 64]
    ms[:6] = edge
    ms[n - 6:] = edge
    mrec = np.zeros((n, 32), np.uint8)
    mrec[:, :8] = ms.astype("<u8").view(np.uint8).reshape(n, 8)
    rs = w.random_u256(w.SEED_NONCES ^ 0xE16C, n)
    pk = gpu_ctx.mul_fixed_base(pack([sk]))
    base = gpu_ctx.base(pk, 8)
    try:
        c1 = gpu_ctx.mul_fixed_base(rs).copy()
        c2 = gpu_ctx.mul_bases([None, base], [mrec, rs]).copy()
    finally:
        base.close()
    bad = [70, 130, 257, n - 300, n - 66, n - 2]
    c1[70, 0] ^= 1
    c2[130, 32] ^= 1
    c2[257] = 0
    c1[n - 300, 0] ^= 1
    c2[n - 66, 32] ^= 1
    c1[n - 2] = 0
    m = ms.copy()
    m[bad] = UMAX
    ok = np.ones(n, np.uint8)
    ok[bad] = 2
    return {"sk": sk, "m": m, "ok": ok, "c1": c1, "c2": c2, "d_c1": dev(c1), "d_c2": dev(c2)}


def test_elgamal_decrypt_recycled_slots(common_ctxs, ciphertexts, common_n):
    n, c = common_n, ciphertexts
    first = {}
    for form in COMMON_FORMS:
        ctx = common_ctxs[form]
        t = ctx.dlog_table(None, 8)                        # 256 baby steps: 2^8 giant steps per item at range_bits = 16
        try:
            def launch(stream, b):
                ctx.decrypt_dev(t, c["sk"], c["d_c1"].data_ptr(), c["d_c2"].data_ptr(), n, 16, b[0].data_ptr(), b[1].data_ptr() + 1, stream=stream)

            def check(b, what):
                m, ok = fetch(b[0], n * 8, 8).copy().view("<u8").reshape(-1), b[1].cpu().numpy()
                assert ok[0] == SENTINEL and (ok[1 + n:] == SENTINEL).all()
                same(ok[1:1 + n], c["ok"], (form, what, "ok"))
                same(m, c["m"], (form, what, "m"))
                first.setdefault(form, (m, ok[1:1 + n].copy()))
            _twice_then_two_streams(ctx, launch, lambda: [(sentinel(n * 8), sentinel(n + 1, 4)) for _ in range(2)], check)
            if form == "table":                            # the four-call composition on the same inputs, and a wrong key: none found
                wm, wok = ctx.elgamal_decrypt(t, c["sk"], c["c1"], c["c2"], 16)
                assert (wm == c["m"]).all() and (wok == c["ok"]).all()
                m, ok = ctx.decrypt(t, c["sk"] + 1, c["c1"], c["c2"], 16)
                assert (ok[c["ok"] == 1] == 0).all() and (ok[c["ok"] == 2] == 2).all() and (m == UMAX).all()
        finally:
            t.close()
    assert first["table"][0].tobytes() == first["naf"][0].tobytes() and first["table"][1].tobytes() == first["naf"][1].tobytes()


# ---- 3: three and four levels of bjj_point_sum ---------------------------------------------------------------------------------------
def levels(n):
    """psum_level_count of csrc/point_sum.hpp: n items, then two entries per tile, until one tile holds the rest"""
    count, tiles = 1, -(-n // T)
    while tiles > 1:
        count, tiles = count + 1, -(-2 * tiles // T)
    return count


N4 = T ** 3 // 4 + 1
THREE = {"one_segment": [T * T // 2 + 1],
         "long_between_short": [1, T * T // 2 - 7, 3, T + 1, 1, T * T // 2 + T + 5] + [3] * 500}
FOUR = {"one_segment": [N4], "then_300_singletons": [N4] + [1] * 300}


def test_level_counts():
    """the shapes of this file reach the levels they are named for; for T = 256 the counts of tests/test_point_sum_host.py"""
    if T == 256:
        assert [levels(n) for n in (1, 256, 257, 1 << 15, (1 << 15) + 1, 1 << 20, (1 << 32) - 1)] == [1, 1, 2, 2, 3, 3, 5]
    assert levels(T * T // 2) == 2 and levels(T * T // 2 + 1) == 3 and levels(N4 - 1) == 3 and levels(N4) == 4
    assert [levels(sum(v)) for v in THREE.values()] == [3, 3] and [levels(sum(v)) for v in FOUR.values()] == [4, 4]


@pytest.fixture(scope="module")
def pool(gpu_ctx, tors):
    """N4 + 300 points of the whole group, k_i * B8 + c_i * T8 with every third one torsion-shifted, generated on the device"""
    from babyjubjub_rs_amd import workload as w
    n = N4 + 300
    c = (w.splitmix64(w.SEED_POINTS ^ 0x3E, n) & np.uint64(7)).astype(np.int64)
    c[np.arange(n) % 3 != 0] = 0
    pts = gpu_ctx.point_add(gpu_ctx.mul_fixed_base(w.random_u256(w.SEED_POINTS ^ 0x96, n)), tors[c]).copy()
    pts.setflags(write=False)
    return pts


def signed(pts, neg):
    from babyjubjub_rs_amd import api
    out = np.array(pts, np.uint8).reshape(-1, 64)
    if neg is not None:
        out[np.asarray(neg) != 0] = api._negate_x(out[np.asarray(neg) != 0])
    return out


def by_oracle_tree(oracle, pts, neg, off):
    """a balanced tree of the C oracle's additions per segment (an odd element waits for the next level), every segment's pairs of a
    level in one oracle call: any association gives the canonical affine bytes"""
    s = signed(pts, neg)
    segs = [s[a:b] for a, b in zip(off, off[1:])]
    while any(len(x) > 1 for x in segs):
        halves = [len(x) // 2 for x in segs]
        sums = oracle.point_add(np.concatenate([x[0:2 * h:2] for x, h in zip(segs, halves)]),
                                np.concatenate([x[1:2 * h:2] for x, h in zip(segs, halves)]))
        at = np.concatenate([[0], np.cumsum(halves)])
        segs = [np.concatenate([sums[at[j]:at[j + 1]], x[2 * h:]]) for j, (x, h) in enumerate(zip(segs, halves))]
    return np.concatenate([x if len(x) else IDENTITY for x in segs])


@pytest.mark.parametrize("shape", sorted(THREE))
def test_point_sum_three_levels(gpu_ctx, oracle, pool, shape):
    off = offsets_of(THREE[shape])
    n, m = off[-1], len(off) - 1
    assert levels(n) == 3
    pts = pool[:n]
    for k, neg in enumerate(signs(n, 0x33 + len(shape))):
        want, wst = by_msm_batch(gpu_ctx, pts, neg, off)
        assert (wst == -1).all()
        same(want, by_oracle_tree(oracle, pts, neg, off), (shape, k, "the yardstick against the oracle"))
        got, st = _dev_call(gpu_ctx, pts, neg, off)
        assert (st == -1).all(), (shape, k)
        same(got, want, (shape, k))
    if shape == "long_between_short":
        clean, neg = want, neg                             # random signs
        got, st = ok_sum(gpu_ctx, pts, neg, off)           # the host form
        assert (st == -1).all()
        same(got, clean, (shape, "host form"))
        other = pool[N4 + 300 - n:N4 + 300]                # elgamal_sum: both components over the same segments and signs
        s1, s2, st = gpu_ctx.elgamal_sum(pts, other, off, neg)
        assert (st == -1).all()
        same(s1, clean, (shape, "elgamal_sum, C1"))
        same(s2, by_msm_batch(gpu_ctx, other, neg, off)[0], (shape, "elgamal_sum, C2"))
        # one off-curve point in the middle of the long segment that has short ones on both sides
        seg = 5
        hit = (off[seg] + off[seg + 1]) // 2
        assert off[seg + 1] - off[seg] > T * T // 2 and off[seg] % T and off[seg + 1] % T
        p = pts.copy()
        p[hit, 0] ^= 1
        got, st = _dev_call(gpu_ctx, p, neg, off)
        assert st[seg] == hit and (np.delete(st, seg) == -1).all()
        assert (got[seg] == 0).all()
        same(np.delete(got, seg, axis=0), np.delete(clean, seg, axis=0), (shape, "beside the spoiled segment"))
        got, st = _dev_call(gpu_ctx, pts, neg, off)        # the next clean call is unaffected
        assert (st == -1).all()
        same(got, clean, (shape, "afterwards"))


@pytest.fixture(scope="module")
def four_levels(gpu_ctx, oracle, pool):
    """the sum of the first N4 points under random signs: by bjj_msm with the scalars 1 / 8l - 1, AND by the oracle's tree.  The tree
    is used: measured on the CPU, 4 194 304 oracle additions on 16 CPUs stay below the 10 s that allow it; the fixture prints what
    they took"""
    neg = signs(N4 + 300, 0x44)[2]
    by_msm = gpu_ctx.msm(pool[:N4], unit_scalars(N4, neg[:N4]))
    t0 = time.time()
    by_tree = by_oracle_tree(oracle, pool[:N4], neg[:N4], [0, N4])
    print("\n[four levels] oracle tree over %d points: %.1f s" % (N4, time.time() - t0))
    same(by_msm, by_tree, "the yardstick against the oracle")
    return neg, by_msm


@pytest.mark.parametrize("shape", sorted(FOUR))
def test_point_sum_four_levels(gpu_ctx, pool, four_levels, shape):
    """level 2 writes its entries back into the list level 0 wrote, level 3 reads them"""
    off = offsets_of(FOUR[shape])
    n, m = off[-1], len(off) - 1
    assert levels(n) == 4 and levels(N4 - 1) == 3
    neg, first = four_levels
    want = np.concatenate([first, signed(pool[N4:n], neg[N4:n])])
    got, st = _dev_call(gpu_ctx, pool[:n], neg[:n], off)
    assert st.shape == (m,) and (st == -1).all()
    same(got, want, shape)
