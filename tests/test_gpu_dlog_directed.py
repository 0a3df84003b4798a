"""bjj_dlog's promise "never a false answer" on the device, where 32-bit tags otherwise keep confirmation from ever refusing anything.

Through the C ABI of the shipped library: items constructed (tests/dlog_ref.py, plain integers) to share, at one chosen giant step, the
index run and the full 32-bit tag of a table entry while their y is no entry's -- at the first steps, a middle and the last one, on
either side of every cut a call can have, at probe offset 0 and behind foreign entries, and across the end of a table whose probe run
wraps.  The expected result, not found, is the definition's: the C oracle enumerates m * G over the whole range.  The model only
proves that the collision is there and is the item's only one.

Through tests/devfuzz/dlog.hip, the shipped kernel unit compiled with 3-bit tags: the cases of tests/dlog_cases.py, where refused hits
are the rule, against the same unit with 32-bit tags, against bjj_dlog and against the oracle; launches cut at the test's choice with
the in-flight marker read between them; the table check over sound and over corrupted slots."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import dlog_cases as dc
import dlog_ref as dr
from conftest import ROOT, ints, pack, unpack

pytestmark = pytest.mark.gpu

B8 = (5299619240641551281634865583518297030282874472190772894086521144482721001553,
      16950150798460657717958625567821834550301663161624707787222815936182638968203)
ABI_TABLES = [("b8", 4, 15), ("b8", 8, 16), ("order_8l", 8, 16)]       # name, baby bits, range bits
N_ALL = 1100                                                           # two workgroups of the search kernel
TAG_TABLES = [("b8", 4), ("b8", 8), ("b8", 12), ("order_8l", 8)]
N_TAG = 1000


def ranges_of(b):
    return [b - 2, b, b + 1, b + 8]


@pytest.fixture(scope="module")
def env(oracle, golden):
    tors = [ints(t) for t in golden["gpu_expected"]["torsion_points"]]

    def mul(P, ks):
        ks = list(ks)
        return unpack(oracle.mul_var_base(np.tile(pack([P]), len(ks)), pack(ks)), 2)

    def add(p, q):
        return unpack(oracle.point_add(pack([p]), pack([q])), 2)[0]
    bases = {"b8": B8, "order_8l": add(mul(B8, [0x1234567])[0], tors[1])}
    assert dr.on_curve(B8) and mul(bases["order_8l"], [dc.SUBORDER])[0] != (0, 1)
    return {"mul": mul, "add": add, "bases": bases, "torsion": tors}


def _cases(env, G, b, ranges, seed, total):
    n_dir = len(dc.build(env["mul"], env["add"], G, b, ranges, env["torsion"][1], 1, n_random=0))
    cases = dc.interleave(dc.build(env["mul"], env["add"], G, b, ranges, env["torsion"][1], seed, n_random=total - n_dir))
    assert len(cases) == total
    return cases


def _want(cases, n, rb):
    m, ok = dc.expected(cases[:n], rb)
    return np.array(m, dtype=np.uint64), np.array(ok, dtype=np.uint8)


def _same(m, ok, wm, wok, what):
    bad = [(i, int(ok[i]), int(m[i]), int(wok[i]), int(wm[i])) for i in np.nonzero((ok != wok) | (m != wm))[0][:8]]
    assert not bad, (what, bad)


def _not_multiples(env, G, rb, points):
    """the definition: none of `points` is m * G with 0 <= m < 2^rb, enumerated by the C oracle"""
    known = set(env["mul"](G, range(1 << rb)))
    assert len(known) == 1 << rb and env["mul"](G, [77])[0] in known
    assert not [p for p in points if p in known]


@pytest.fixture(scope="module")
def abi_cases(env):
    """per table: the model's table, the constructed items (each one asserted by the model), and N_ALL cases with a constructed item
    at every other position from the start, so that n = 1 and n = 65 hold them beside found neighbours"""
    out = {}
    for name, b, rb in ABI_TABLES:
        G = env["bases"][name]
        T = dr.table(G, b)
        extra = (40, 63, 64) + ((300, 511, 512) if rb - b - 1 >= 10 else ())
        items = dr.false_hit_items(T, rb, extra, random.Random(0xFA15E + 16 * b + len(name)))
        reached = [dr.assert_false_hit(T, it, rb) for it in items]
        assert sum(reached) == len(items) - 2 and {(it["step"], it["kind"]) for it in items} >= {
            (s, k) for s in (0, 1, 63, 64, dr.steps_of(b, rb) - 1) for k in ("first", "behind")}
        _not_multiples(env, G, rb, [it["P"] for it in items])
        cases = _cases(env, G, b, [b - 2, b + 1, rb - 4, rb], 0xD1EC + b, N_ALL - len(items))
        for k, it in enumerate(items):
            cases.insert(2 * k, (it["P"], dc.NOT_IN_RANGE))
        assert len(cases) == N_ALL and isinstance(cases[1][1], int)
        out[(name, b)] = dict(T=T, items=items, cases=cases, recs=pack([rec for rec, _ in cases]).reshape(N_ALL, 64), rb=rb)
    assert sum(len(v["items"]) for v in out.values()) >= 40
    return out


@pytest.fixture(scope="module")
def tables(gpu_ctx, env):
    made = {}

    def get(name, b):
        if (name, b) not in made:
            made[(name, b)] = gpu_ctx.dlog_table(None if name == "b8" else env["bases"][name], b)
        return made[(name, b)]
    yield get
    for t in made.values():
        t.close()


# ---- 1: constructed false hits through the shipped library ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,b,rb", ABI_TABLES)
def test_constructed_false_hits_are_not_found_and_neighbours_keep_their_m(gpu_ctx, tables, abi_cases, name, b, rb):
    """host form at n = 1, 65 and all, then the _dev form.  At (4, 15) the walk is 1 024 steps and the 512-steps-per-item cap cuts
    the call: the items of steps 511 and 512 are refused on the last step of a launch and on the first of the resumed one."""
    import torch
    t, c = tables(name, b), abi_cases[(name, b)]
    for n in (1, 65, N_ALL):
        m, ok = t.dlog(c["recs"][:n], rb)
        wm, wok = _want(c["cases"], n, rb)
        _same(m, ok, wm, wok, (name, b, n))
    assert wok[0] == 0 and wok[1] == 1 and set(wok) == {0, 1, 2}
    dev = torch.device("cuda", 0)
    d_pts = torch.from_numpy(c["recs"].reshape(-1).copy()).to(dev)
    d_m = torch.full((N_ALL * 8,), 0xEE, dtype=torch.uint8, device=dev)
    d_ok = torch.full((N_ALL,), 0xEE, dtype=torch.uint8, device=dev)
    gpu_ctx.dlog_dev(t, d_pts.data_ptr(), N_ALL, rb, d_m.data_ptr(), d_ok.data_ptr())
    gpu_ctx.sync()
    assert d_m.cpu().numpy().tobytes() == wm.tobytes() and d_ok.cpu().numpy().tobytes() == wok.tobytes()


def test_false_hits_beside_the_cut_of_a_context_with_a_launch_bound(abi_cases):
    """BJJ_DLOG_LAUNCH_STEPS = 64 (one item per launch) and 4096 (64 items per launch): launches of 64 steps, so the items of steps
    63 and 64 are refused right before and right after the cut"""
    import babyjubjub_rs_amd as bjj
    c = abi_cases[("b8", 8)]
    assert {it["step"] for it in c["items"]} >= {63, 64}
    for bound, n in (("64", 65), ("4096", N_ALL)):
        old = os.environ.get("BJJ_DLOG_LAUNCH_STEPS")
        os.environ["BJJ_DLOG_LAUNCH_STEPS"] = bound
        try:
            ctx = bjj.Context(0, 16)
        finally:
            if old is None:
                os.environ.pop("BJJ_DLOG_LAUNCH_STEPS", None)
            else:
                os.environ["BJJ_DLOG_LAUNCH_STEPS"] = old
        try:
            m, ok = ctx.dlog_table(None, 8).dlog(c["recs"][:n], c["rb"])
            wm, wok = _want(c["cases"], n, c["rb"])
            _same(m, ok, wm, wok, bound)
        finally:
            ctx.close()


def test_a_constructed_ciphertext_decrypts_to_not_found(gpu_ctx, tables, abi_cases, env):
    """bjj_elgamal_decrypt sits on the same kernel: M = C2 - sk * C1 is a constructed item for two ciphertexts, m * G for the others"""
    c = abi_cases[("b8", 8)]
    rng = np.random.default_rng(0xE16B)
    sk = int.from_bytes(rng.bytes(31), "little") % dc.SUBORDER
    plain = [c["items"][0]["P"], env["mul"](B8, [4242])[0], c["items"][7]["P"], (0, 1)]
    rs = [int.from_bytes(rng.bytes(31), "little") % dc.SUBORDER for _ in plain]
    c1 = [env["mul"](B8, [r])[0] for r in rs]
    c2 = [env["add"](p, env["mul"](a, [sk])[0]) for p, a in zip(plain, c1)]
    m, ok = gpu_ctx.decrypt(tables("b8", 8), sk, pack(c1), pack(c2), c["rb"])
    assert list(ok) == [0, 1, 0, 1] and [int(v) for v in m] == [dc.UINT64_MAX, 4242, dc.UINT64_MAX, 0]


# ---- 2: a probe run across the end of the table -----------------------------------------------------------------------------------------
def test_a_probe_run_that_crosses_the_end_of_the_table(gpu_ctx, env):
    """a base whose 4-bit table has entries homed at the last slot and the run going on over the first ones (the model finds it and
    asserts it: 161 * B8).  Without the `& mask` of the walk or of the insertion this table reads and writes past its allocation."""
    b, rb = 4, 8
    k, T = dr.wrapped_base(B8, b)
    G = env["mul"](B8, [k])[0]
    assert G == T.G and T.wraps(T.mask) and T.run_from(T.mask)[:2] == [T.mask, 0] and len(T._by_home[T.mask]) >= 1
    sites = dr.hit_sites(T)["wrapped"]
    rng = random.Random(0x3A9)
    items = [dict(zip(("P", "Q"), dr.false_hit_item(T, step, idx, e, rng)), step=step, idx=idx, e=e, kind="wrapped")
             for step, (idx, e) in zip((0, 2, 3, 7, 1), sites + sites)]
    assert items and all(dr.assert_false_hit(T, it, rb) == 1 for it in items)
    _not_multiples(env, G, rb, [it["P"] for it in items])
    pts = env["mul"](G, range(1 << rb))
    recs = pack(pts + [it["P"] for it in items]).reshape(-1, 64)
    t = gpu_ctx.dlog_table(G, b)
    try:
        assert t.check() == 0 and t.base() == G
        for range_bits in (rb, b + 2):
            m, ok = t.dlog(recs, range_bits)
            top = 1 << range_bits
            assert [int(v) for v in m[:top]] == list(range(top)) and (ok[:top] == 1).all()      # 7, 9 and their mirrors among them
            assert (ok[top:] == 0).all() and (m[top:] == np.uint64(dc.UINT64_MAX)).all()
    finally:
        t.close()


# ---- 3: the kernel unit with 3-bit tags ---------------------------------------------------------------------------------------------------
class Harness:
    """tests/devfuzz/libbjj_dlog_test_tag<bits>.so on torch tensors, on the null stream"""

    def __init__(self, bits):
        d = os.path.join(ROOT, "tests", "devfuzz")
        name = "libbjj_dlog_test_tag%d.so" % bits
        r = subprocess.run(["make", "-s", name], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.lib = ctypes.CDLL(os.path.join(d, name))
        vp, ci = ctypes.c_void_p, ctypes.c_int
        self.lib.dl_setup.argtypes = [vp, ci, vp, vp]
        self.lib.dl_build.argtypes = [vp, vp, ci, vp, vp]
        self.lib.dl_check.argtypes = [ci, vp, vp, ci, vp, vp]
        self.lib.dl_search.argtypes = [vp, vp, ci, vp, ctypes.c_size_t, ci, ctypes.c_uint32, ctypes.c_uint32, ci, vp, vp, vp]
        assert self.lib.dl_tag_bits() == bits and self.lib.dl_block() == 1024 and self.lib.dl_param_words() == 128
        self.tables = {}

    def table(self, G, b):
        """(params, slots) of G (None = B8), built and synchronised; kept for the module"""
        if (G, b) not in self.tables:
            torch = self.torch
            params = torch.zeros(128, dtype=torch.int32, device=self.dev)
            slots = torch.zeros(1 << (b + 2), dtype=torch.int64, device=self.dev)
            failed = torch.zeros(1, dtype=torch.int64, device=self.dev)
            xy = None if G is None else pack([G])
            assert self.lib.dl_setup(params.data_ptr(), b, None if xy is None else xy.ctypes.data, None) == 0
            assert self.lib.dl_build(slots.data_ptr(), params.data_ptr(), b, failed.data_ptr(), None) == 0
            torch.cuda.synchronize()
            assert int(failed.cpu()[0]) == 0
            self.tables[(G, b)] = (params, slots)
        return self.tables[(G, b)]

    def check(self, tab, b):
        """violated conditions as the library counts them"""
        bad2 = self.torch.zeros(2, dtype=self.torch.int64, device=self.dev)
        assert self.lib.dl_check(64, tab[1].data_ptr(), tab[0].data_ptr(), b, bad2.data_ptr(), None) == 0
        self.torch.cuda.synchronize()
        bad, occ = (int(v) for v in bad2.cpu())
        return bad + (1 if occ != (1 << b) + 1 else 0), occ

    def search(self, tab, b, recs, rb, per_launch=None, between=None):
        """(m, ok) of one call cut into launches of per_launch steps (None: one launch); between(s1, ok bytes) after each launch but
        the last"""
        torch = self.torch
        n = len(recs)
        d_pts = torch.from_numpy(np.ascontiguousarray(recs).reshape(-1).copy()).to(self.dev)
        d_m = torch.full((n,), -0x1111111111111112, dtype=torch.int64, device=self.dev)
        d_ok = torch.full((n,), 0xEE, dtype=torch.uint8, device=self.dev)
        nsteps = dr.steps_of(b, rb)
        step = per_launch or nsteps
        for s0 in range(0, nsteps, step):
            s1 = min(s0 + step, nsteps)
            assert self.lib.dl_search(tab[1].data_ptr(), tab[0].data_ptr(), b, d_pts.data_ptr(), n, rb, s0, s1, 1 if s1 == nsteps else 0,
                                      d_m.data_ptr(), d_ok.data_ptr(), None) == 0
            torch.cuda.synchronize()
            if between is not None and s1 < nsteps:
                between(s1, d_ok.cpu().numpy())
        return d_m.cpu().numpy().view(np.uint64), d_ok.cpu().numpy()


@pytest.fixture(scope="module")
def tag3():
    return Harness(3)


@pytest.fixture(scope="module")
def tag32():
    return Harness(32)


@pytest.fixture(scope="module")
def tag_cases(env):
    out = {}
    for name, b in TAG_TABLES:
        cases = _cases(env, env["bases"][name], b, ranges_of(b), 0xD106 + b, N_TAG)
        out[(name, b)] = (pack([rec for rec, _ in cases]).reshape(N_TAG, 64), cases)
    return out


def _decided_at(truth, b):
    """the giant step that decides an item: window i answers for m in [i 2^(b+1), (i + 1) 2^(b+1)], the earlier window first"""
    return 0 if truth == 0 else (truth - 1) >> (b + 1)


@pytest.mark.parametrize("name,b", TAG_TABLES)
def test_three_bit_tags_give_the_answers_of_32_bit_tags_the_library_and_the_oracle(tables, tag3, tag32, tag_cases, env, name, b):
    recs, cases = tag_cases[(name, b)]
    G = env["bases"][name]
    # the inputs exercise what they are meant to: counted by the model, over what every table of (G, b) refuses -- before any run
    rb = b + 8
    refused = [len(dr.walk(rec, G, b, rb, 3)[0]) for rec, truth in cases[:400]
               if isinstance(truth, int) and truth < (1 << rb) and rec[0] < dc.Q]
    assert sum(1 for r in refused if r >= 1) >= 10 and max(refused) >= 2, (name, b, sorted(refused)[-5:])
    t = tables(name, b)
    arg = None if name == "b8" else G
    for rb in ranges_of(b):
        wm, wok = _want(cases, N_TAG, rb)
        m3, ok3 = tag3.search(tag3.table(arg, b), b, recs, rb)
        _same(m3, ok3, wm, wok, ("tag3", name, b, rb))
        m32, ok32 = tag32.search(tag32.table(arg, b), b, recs, rb)
        ma, oka = t.dlog(recs, rb)
        assert m3.tobytes() == m32.tobytes() == ma.tobytes() == wm.tobytes()
        assert ok3.tobytes() == ok32.tobytes() == oka.tobytes() == wok.tobytes()


@pytest.mark.parametrize("name,b", [("b8", 4), ("b8", 8), ("b8", 12)])
def test_cut_launches_under_three_bit_tags(tag3, tag_cases, name, b):
    """one step and three steps per launch against one launch: a refused hit on the last step of every launch and on the first of
    every resumed one.  Between launches ok[i] is 0xFF exactly for the items whose walk is not over; after the last, for none."""
    recs, cases = tag_cases[(name, b)]
    rb = b + 8
    nsteps = dr.steps_of(b, rb)
    tab = tag3.table(None, b)
    wm, wok = _want(cases, N_TAG, rb)
    seen = []

    def between(s1, ok):
        flying = np.array([t != dc.OFF_CURVE and (not isinstance(t, int) or _decided_at(t, b) >= s1) for _, t in cases])
        assert ((ok == 0xFF) == flying).all(), s1
        assert (ok[~flying] == wok[~flying]).all(), s1
        seen.append(s1)
    whole = tag3.search(tab, b, recs, rb)
    _same(whole[0], whole[1], wm, wok, "uncut")
    for per_launch in (1, 3):
        del seen[:]
        m, ok = tag3.search(tab, b, recs, rb, per_launch, between)
        assert seen == list(range(per_launch, nsteps, per_launch))
        assert not (ok == 0xFF).any()
        assert m.tobytes() == whole[0].tobytes() and ok.tobytes() == whole[1].tobytes(), per_launch


@pytest.mark.parametrize("bits", [3, 32])
@pytest.mark.parametrize("b", [4, 8, 12])
def test_the_table_check_on_the_device_sound_and_corrupted(tag3, tag32, tag_cases, bits, b):
    """(0 violations, 2^b + 1 occupied slots); after one tag bit of one occupied slot is flipped in device memory, and after the low
    bit of a slot's j field is, the check counts violations -- and a search over the corrupted table may miss but never answers
    falsely: every ok = 1 carries the true m, every off-curve item its 2."""
    h = tag3 if bits == 3 else tag32
    params, slots = h.table(None, b)
    assert h.check((params, slots), b) == (0, (1 << b) + 1)
    recs, cases = tag_cases[("b8", b)]
    rb = b + 8
    wm, wok = _want(cases, N_TAG, rb)
    host = slots.cpu().numpy()
    victim = int(np.nonzero(host)[0][(1 << b) // 2])                        # an occupied slot chosen by position alone
    jv = (int(host[victim]) & 0xFFFFFFFF) - 1
    # the baby step an item is found with: the only entry its answer depends on
    needs = np.array([abs(t - ((1 << b) + _decided_at(t, b) * (2 << b))) if isinstance(t, int) else -1 for _, t in cases])
    assert 0 <= jv <= (1 << b) and (needs[wok == 1] != jv).sum() > N_TAG // 2
    for bit in (32, 0):
        slots[victim] ^= (1 << bit)
        try:
            assert h.check((params, slots), b)[0] > 0, bit
            m, ok = h.search((params, slots), b, recs, rb)
        finally:
            slots[victim] ^= (1 << bit)
        found = ok == 1
        assert (m[found] == wm[found]).all() and (wok[found] == 1).all(), bit
        assert ((ok == 2) == (wok == 2)).all() and (m[~found] == np.uint64(dc.UINT64_MAX)).all()
        spared = needs != jv                                                 # one slot: only the items that needed it may be missed
        assert (ok[spared] == wok[spared]).all() and (m[spared] == wm[spared]).all(), bit
    assert h.check((params, slots), b) == (0, (1 << b) + 1)
    m, ok = h.search((params, slots), b, recs, rb)
    _same(m, ok, wm, wok, "restored")
