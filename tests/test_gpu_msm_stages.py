"""The MSM pipeline of bjj_msm / bjj_msm_batch stage by stage on the MI355X.  tests/devfuzz/msm.hip compiles csrc/k_msm.hip and
csrc/k_msm_batch.hip as they ship and runs one stage per call on a scratch block of the test's; after every stage the arrays the
device left behind -- red, niels, counts, status, cursor, total, rec, buckets, window sums, the 64 result bytes -- are read back and
held against the plain-integer model of tests/msm_ref.py (points with known logarithms, expected points by the C oracle).  Every
comparison is exact.  The scratch block is filled with 0xA5 before every run: a bucket or an entry that was never written holds
garbage, not zeros and not the last call's points.

  a. wave_counter_add<u32 / u64> on key / active patterns of the test's choice (a kernel beside the product's)
  b. bjjk::msm_scan over histograms of chosen lengths and counts, against numpy.cumsum in uint64
  c. the stages of real calls, n x c x scalar sets, one off-curve record at the first, a middle and the last index; the batched form
  d. slices and levels over synthetic records, S in {8, 16, 32, 64}
  e. window sums with chosen bucket occupancy

tests/test_msm_stages_host.py judges the model and the checkers on the CPU."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import msm_ref as mr
from conftest import ROOT
from test_msm_host import EDGE_SCALARS

pytestmark = pytest.mark.gpu

FIELDS = ["o_niels", "o_red", "o_counts", "o_cursor", "o_bsum", "o_total", "o_status", "o_out", "o_rec", "o_e0", "o_e1", "o_buckets",
          "o_w0", "o_w1", "o_offsets", "o_flag", "o_seg", "bytes", "W", "G", "keys", "records", "S1", "slices1", "levels", "nb"]
ITEMS = {}          # stage -> items compared (printed by every test: the numbers of the commit message)


def _count(stage, k):
    ITEMS[stage] = ITEMS.get(stage, 0) + int(k)


class Harness:
    """tests/devfuzz/libbjj_msm_test.so on torch tensors, on the null stream"""

    def __init__(self):
        d = os.path.join(ROOT, "tests", "devfuzz")
        r = subprocess.run(["make", "-s", "libbjj_msm_test.so"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)
        lib = self.lib = ctypes.CDLL(os.path.join(d, "libbjj_msm_test.so"))
        vp, ci, cu, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_size_t
        lib.mt_layout.argtypes = [sz, sz, ci, cu, vp]
        lib.mt_level_count.argtypes = [ctypes.c_ulonglong, cu]
        lib.mt_prepare.argtypes = [vp, sz, vp, vp, sz, ci, vp]
        lib.mt_batch_prepare.argtypes = [vp, sz, vp, vp, sz, sz, ci, vp]
        lib.mt_scan.argtypes = [vp, sz, sz, sz, ci, vp]
        lib.mt_scan_only.argtypes = [vp, sz, vp, vp, vp, vp]
        lib.mt_scatter.argtypes = [vp, sz, sz, ci, vp]
        lib.mt_batch_scatter.argtypes = [vp, sz, sz, sz, ci, vp]
        lib.mt_reduce.argtypes = [vp, sz, sz, sz, ci, cu, vp]
        lib.mt_finish.argtypes = [vp, sz, sz, ci, ci, vp]
        lib.mt_batch_finish.argtypes = [vp, sz, sz, sz, ci, ci, vp]
        lib.mt_counter_u32.argtypes = [vp, cu, vp, vp, vp, sz, vp]
        lib.mt_counter_u64.argtypes = [vp, cu, vp, vp, vp, sz, vp]
        assert lib.mt_fields() == len(FIELDS) and lib.mt_block() == mr.BLOCK and lib.mt_scan_tile() == mr.SCAN_TILE
        assert lib.mt_top_block() == mr.TOP_BLOCK and lib.mt_entry_words() == mr.ENTRY_WORDS

    def layout(self, n, m, c, S1=0):
        """the product's MsmLayout as a dict, or None when the harness refuses the arguments"""
        f = (ctypes.c_ulonglong * len(FIELDS))()
        if self.lib.mt_layout(n, m, c, S1, f) != 0:
            return None
        return dict(zip(FIELDS, (int(v) for v in f)))

    def sync(self):
        self.torch.cuda.synchronize()

    def filled(self, nbytes):
        t = self.torch.full((max(int(nbytes), 1),), mr.FILL, dtype=self.torch.uint8, device=self.dev)
        assert t.data_ptr() % 256 == 0
        return t

    def upload(self, arr):
        return self.torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).to(self.dev)

    def read(self, block, off, count, dtype):
        nbytes = int(count) * np.dtype(dtype).itemsize
        assert 0 <= off and off + nbytes <= block.numel()
        return block[off:off + nbytes].cpu().numpy().view(dtype)

    def write(self, block, off, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        assert 0 <= off and off + raw.size <= block.numel()
        block[off:off + raw.size].copy_(self.torch.from_numpy(raw.copy()))


@pytest.fixture(scope="module")
def h():
    return Harness()


@pytest.fixture(scope="module")
def points(oracle):
    return mr.Points(oracle)


def _none(findings, what):
    assert findings == [], (what, findings)


# ---- a. the counters ---------------------------------------------------------------------------------------------------------------------
ARR_LEN = 128


def _wave_patterns():
    """name -> (64 keys, 64 active flags) of one wave"""
    on, every = [1] * 64, list(range(64))
    p = {
        "all_on_one_key": ([5] * 64, on),
        "63_and_1": ([5] * 63 + [9], on),
        "1_and_63": ([9] + [5] * 63, on),
        "groups_3_4_5": ([1] * 3 + [2] * 4 + [3] * 5 + [0] * 52, [1] * 12 + [0] * 52),      # a first group below 4: the break
        "groups_5_4_3": ([3] * 5 + [2] * 4 + [1] * 3 + [0] * 52, [1] * 12 + [0] * 52),      # served, served, then the break
        "group_3_then_40": ([1] * 3 + [2] * 40 + [0] * 21, [1] * 43 + [0] * 21),            # the early break into per-lane atomics
        "16_groups_of_4": ([i // 4 for i in every], on),
        "16_groups_of_4_interleaved": ([i % 16 for i in every], on),
        "64_distinct": (every, on),
        "every_second_inactive": ([7] * 64, [1 - i % 2 for i in every]),
        "lane_0_inactive": ([7] * 64, [0] + [1] * 63),
        "only_lane_63": ([7] * 64, [0] * 63 + [1]),
        "nothing_active": ([7] * 64, [0] * 64),
    }
    assert all(len(k) == 64 and len(a) == 64 for k, a in p.values())
    return p


def _counter_cases():
    """name -> (keys, active) of one launch: every wave pattern alone, a partly filled last wave, four waves of one workgroup and two
    workgroups on the same keys"""
    waves = _wave_patterns()
    cases = dict(waves)
    cases["partly_filled_last_wave"] = ([5] * 101, [1] * 101)
    cases["partly_filled_last_wave_groups"] = ([i // 4 % 16 for i in range(101)], [1] * 101)
    cases["four_waves_one_key"] = ([5] * 256, [1] * 256)
    cases["two_workgroups_one_key"] = ([5] * 512, [1] * 512)
    order = ["16_groups_of_4", "all_on_one_key", "groups_3_4_5", "64_distinct", "63_and_1", "every_second_inactive", "group_3_then_40",
             "16_groups_of_4_interleaved"]
    cases["two_workgroups_mixed_waves"] = (sum((list(waves[w][0]) for w in order), []), sum((list(waves[w][1]) for w in order), []))
    cases["two_workgroups_and_a_part"] = ([i // 4 % 16 for i in range(512 + 37)], [1] * (512 + 37))
    return cases


@pytest.mark.parametrize("bits,init", [(32, 0), (32, (1 << 32) - 2), (64, 0), (64, (1 << 32) - 7)])
def test_wave_counter_add(h, bits, init):
    torch = h.torch
    dt = np.uint32 if bits == 32 else np.uint64
    call = h.lib.mt_counter_u32 if bits == 32 else h.lib.mt_counter_u64
    cases = _counter_cases()
    assert len(cases) >= 12
    above = crossed = 0
    for name, (keys, active) in cases.items():
        n = len(keys)
        mr.validate_counter_input(keys, active, ARR_LEN)
        before = np.full(ARR_LEN, init, dtype=dt)
        d_arr, d_key, d_act = h.upload(before), h.upload(np.array(keys, dtype=np.uint32)), h.upload(np.array(active, dtype=np.uint8))
        d_out = h.filled(n * (bits // 8))
        assert call(d_arr.data_ptr(), ARR_LEN, d_key.data_ptr(), d_act.data_ptr(), d_out.data_ptr(), n, None) == 0
        h.sync()
        after, ret = d_arr.cpu().numpy().view(dt), d_out.cpu().numpy().view(dt)
        _none(mr.check_counter(bits, init, keys, active, ret, before, after), (bits, init, name))
        _count("counter lanes", sum(active))
        if bits == 64 and init:
            got = [int(ret[i]) for i in range(n) if active[i]]
            crossed += int(bool(got) and min(got) < 1 << 32 <= max(got))
            # the base of a wave is the smallest value it returns for the key: whole waves whose base lies at or above 2^32
            above += sum(1 for w in range(0, n, 64) if all(active[w:w + 64]) and len(set(keys[w:w + 64])) == 1
                         and min(int(v) for v in ret[w:w + 64]) >= 1 << 32)
    assert h.lib.mt_counter_u32(None, ARR_LEN, None, None, None, 64, None) == -1
    if bits == 64 and init:
        assert crossed >= 3 and above >= 3, (crossed, above)       # inside one group, and a base handed across the lanes above 2^32
    print("counter patterns: %d (T = u%d, init %#x); u64 bases >= 2^32: %d waves; items %s" % (len(cases), bits, init, above, ITEMS))


# ---- b. the scan ---------------------------------------------------------------------------------------------------------------------------
SCAN_M = [1, 15, 16, 17, 4095, 4096, 4097, 1024 * 4096 - 1, 1024 * 4096, 1024 * 4096 + 1, 2 * 1024 * 4096 + 4097]
BIG = (1 << 32) - 1


def _scan_patterns(M):
    rng = np.random.default_rng(0x5CA0 + M)
    first, mid, last = 0, M // 2, M - 1
    out = {"zero": np.zeros(M, dtype=np.uint32), "one": np.ones(M, dtype=np.uint32),
           "random": rng.integers(0, 1 << 16, size=M, dtype=np.uint32)}
    for name, at in (("big_first", [first]), ("big_middle", [mid]), ("big_last", [last]), ("three_big", [first, mid, last])):
        c = np.zeros(M, dtype=np.uint32)
        c[at] = BIG
        out[name] = c
    r = rng.integers(0, 1 << 16, size=M, dtype=np.uint32)
    r[[first, mid, last]] = BIG
    out["three_big_among_random"] = r
    return out


@pytest.mark.parametrize("M", SCAN_M)
def test_scan_of_a_chosen_histogram(h, M):
    nb = mr.div_up(M, mr.SCAN_TILE)
    for name, counts in _scan_patterns(M).items():
        d_counts = h.upload(counts)
        d_cursor, d_bsum, d_total = h.filled(M * 8), h.filled(nb * 8), h.filled(8)
        assert h.lib.mt_scan_only(d_counts.data_ptr(), M, d_cursor.data_ptr(), d_bsum.data_ptr(), d_total.data_ptr(), None) == 0
        h.sync()
        cursor, total = d_cursor.cpu().numpy().view(np.uint64), int(d_total.cpu().numpy().view(np.uint64)[0])
        _none(mr.check_scan(counts, cursor, total), (M, name))
        if name == "three_big" and M >= 3:
            assert total == 3 * BIG > 1 << 33 and int(cursor[-1]) == 2 * BIG > 1 << 32      # the running sum passes 2^32 and 2^33
        _count("scan keys", M)
    assert h.lib.mt_scan_only(d_counts.data_ptr(), 0, d_cursor.data_ptr(), d_bsum.data_ptr(), d_total.data_ptr(), None) == -1
    assert h.lib.mt_scan_only(None, M, d_cursor.data_ptr(), d_bsum.data_ptr(), d_total.data_ptr(), None) == -1
    print("scan: M = %d, %d tiles, %d chunks of the top kernel; items %s" % (M, nb, mr.div_up(nb, mr.TOP_BLOCK), ITEMS))


# ---- c. the stages of real calls -------------------------------------------------------------------------------------------------------------
def _check_layout(L, n, m, c):
    W, B = mr.windows(c), mr.buckets(c)
    assert (L["W"], L["G"], L["keys"], L["records"]) == (W, B // mr.SEG, m * W * B, n * W)
    assert L["S1"] == mr.slice_records(n * W) and L["slices1"] == mr.div_up(n * W, L["S1"]) and L["levels"] == mr.level_count(n * W, L["S1"])
    assert L["nb"] == mr.div_up(L["keys"], mr.SCAN_TILE)
    offs = [L[k] for k in FIELDS[:17]]
    assert all(o % 256 == 0 for o in offs) and max(offs) < L["bytes"]
    ends = {"o_counts": L["keys"] * 4, "o_cursor": L["keys"] * 8, "o_rec": L["records"] * 8, "o_buckets": L["keys"] * 160,
            "o_w0": m * W * L["G"] * 160, "o_niels": n * 128, "o_red": n * 32, "o_seg": n * 4, "o_offsets": (m + 1) * 8,
            "o_status": m * 8, "o_out": m * 64, "o_bsum": L["nb"] * 8, "o_e0": 2 * L["slices1"] * 160}
    later = sorted(offs + [L["bytes"]])
    for k, size in ends.items():                              # every region ends before the next one begins
        assert L[k] + size <= later[later.index(L[k]) + 1], k


def run_stages(h, points, gpu_ctx, logs, pts, scalars, c, offsets=None, bad=()):
    """one call through the harness, checked after every stage; then the library's own _dev call on the same device inputs"""
    torch = h.torch
    n = len(scalars)
    batch = offsets is not None
    model = mr.Model(logs, scalars, c, offsets=offsets, bad=bad)
    m = model.m
    L = h.layout(n, m, c)
    _check_layout(L, n, m, c)
    block = h.filled(L["bytes"])
    size = block.numel()
    d_pts, d_sc = h.upload(mr.pack_points(pts)), h.upload(mr.pack_scalars(scalars))
    P, S, B = block.data_ptr(), d_pts.data_ptr(), d_sc.data_ptr()
    what = (n, c, m, sorted(bad))
    # 1. prepare
    if batch:
        h.write(block, L["o_offsets"], np.array(model.offsets, dtype=np.uint64))
        assert h.lib.mt_batch_prepare(P, size, S, B, n, m, c, None) == 0
    else:
        assert h.lib.mt_prepare(P, size, S, B, n, c, None) == 0
    h.sync()
    counts = h.read(block, L["o_counts"], model.M, np.uint32)
    _none(mr.check_prepare(model, pts, h.read(block, L["o_red"], n * 8, np.uint32), h.read(block, L["o_niels"], n * 32, np.uint32), counts,
                           h.read(block, L["o_status"], m, np.int64), h.read(block, L["o_seg"], n, np.uint32) if batch else None),
          ("prepare",) + what)
    if batch:
        assert int(h.read(block, L["o_flag"], 1, np.uint32)[0]) == 0
    _count("prepare items", n)
    # 2. scan
    assert h.lib.mt_scan(P, size, n, m, c, None) == 0
    h.sync()
    cursor = h.read(block, L["o_cursor"], model.M, np.uint64)
    total = int(h.read(block, L["o_total"], 1, np.uint64)[0])
    _none(mr.check_scan(counts, cursor, total), ("scan",) + what)
    assert total == model.total <= L["records"]
    _count("scan keys", model.M)
    # 3. scatter
    assert (h.lib.mt_batch_scatter(P, size, n, m, c, None) if batch else h.lib.mt_scatter(P, size, n, c, None)) == 0
    h.sync()
    rec = h.read(block, L["o_rec"], L["records"], np.uint64)
    _none(mr.check_records(model, rec, cursor, counts), ("scatter",) + what)
    assert (rec[total:] == np.uint64(mr.FILL64)).all()                                   # nothing behind the last record
    assert (h.read(block, L["o_cursor"], model.M, np.uint64) == cursor + counts.astype(np.uint64)).all()
    assert (h.read(block, L["o_counts"], model.M, np.uint32) == counts).all()
    _count("records", total)
    # 4. + 5. reduce
    which = h.lib.mt_reduce(P, size, n, m, c, 0, None)
    assert which == len(mr.group_passes(L["G"])) % 2
    h.sync()
    _none(mr.check_buckets(model, points, h.read(block, L["o_buckets"], model.M * mr.ENTRY_WORDS, np.uint32), counts), ("buckets",) + what)
    _none(mr.check_window_sums(model, points, h.read(block, L["o_w1" if which else "o_w0"], m * model.W * mr.ENTRY_WORDS, np.uint32)),
          ("window sums",) + what)
    _count("buckets", len(model.bucket_logs))
    _count("window sums", m * model.W)
    # 6. finish
    assert (h.lib.mt_batch_finish(P, size, n, m, c, which, None) if batch else h.lib.mt_finish(P, size, n, c, which, None)) == 0
    h.sync()
    out = h.read(block, L["o_out"], m * 64, np.uint8).copy()
    _none(mr.check_result(model, points, out), ("finish",) + what)
    assert [int(v) for v in h.read(block, L["o_status"], m, np.int64)] == model.status
    # the library's own call on the same inputs: the harness runs the pipeline the library runs
    d_out = torch.full((m * 64,), 0xEE, dtype=torch.uint8, device=h.dev)
    d_st = torch.full((m + 1,), 0x7777, dtype=torch.int64, device=h.dev)
    if batch:
        d_off = h.upload(np.array(model.offsets, dtype=np.uint64))
        gpu_ctx.msm_batch_dev(S, B, n, d_off.data_ptr(), m, d_out.data_ptr(), d_st.data_ptr(), window_bits=c)
    else:
        gpu_ctx.msm_dev(S, B, n, d_out.data_ptr(), d_st.data_ptr(), window_bits=c)
    gpu_ctx.sync()
    assert d_out.cpu().numpy().tobytes() == out.tobytes(), ("library",) + what
    assert [int(v) for v in d_st.cpu()[:m]] == model.status
    _count("results", m)
    return model


STAGE_N = [1, 63, 64, 65, 255, 256, 257, 1000]
STAGE_C = [4, 5, 7, 8, 10, 13]


def test_the_window_sizes_give_every_number_of_group_passes():
    assert [mr.buckets(c) // mr.SEG for c in STAGE_C] == [1, 2, 8, 16, 64, 512]
    assert [mr.group_passes(mr.buckets(c) // mr.SEG) for c in STAGE_C] == [[], [2], [8], [8, 2], [8, 8], [8, 8, 8]]


@pytest.mark.parametrize("c", STAGE_C)
@pytest.mark.parametrize("n", STAGE_N)
def test_stages_of_real_calls(h, points, gpu_ctx, n, c):
    logs = mr.make_pool(n, 0x9001 + n)
    pts = points.of(logs)
    if n >= 8:
        assert pts[1] == (0, 1) and pts[2] == (0, mr.R_MOD - 1) and pts[5] == (-pts[4][0] % mr.R_MOD, pts[4][1])
    sets = mr.scalar_sets(n, c, 0xC0DE + 64 * n + c, EDGE_SCALARS)
    assert len(sets) == 10
    for name, sc in sets.items():
        model = run_stages(h, points, gpu_ctx, logs, pts, sc, c)
        if name == "one_window":
            assert model.total == n and n * model.W > n                                # one populated window against a bound of n W
        if name == "zero":
            assert model.total == 0
        if name == "digit_at_half":
            assert set(k % model.B for k in model.by_key) == {model.B - 1}             # v == 2^(c-1): the last bucket of every window
    for i in sorted({0, n // 2, n - 1}):                                               # one off-curve record
        spoiled = list(pts)
        spoiled[i] = mr.off_curve(pts[i])
        model = run_stages(h, points, gpu_ctx, logs, spoiled, sets["random"], c, bad=(i,))
        assert model.status == [i] and model.red[i] == 0 and not any(it == i for rs in model.by_key.values() for it, _ in rs)
    print("stages n = %d c = %d: items %s" % (n, c, ITEMS))


def _batch_offsets(n, m):
    if m == 1:
        return [0, n]
    if m == 5:
        return [0, 0, 1, 100, 100, n]                       # empty segments, a one-item segment, boundaries inside a wave
    rnd = random.Random(0x0FF5 + m)
    off = [0, 0, 1, 2, 2, 3] + sorted(rnd.randrange(3, n + 1) for _ in range(m - 6)) + [n]
    assert len(off) == m + 1
    return off


@pytest.mark.parametrize("c", [5, 7])
@pytest.mark.parametrize("m", [1, 5, 64])
def test_stages_of_the_batched_form(h, points, gpu_ctx, m, c):
    n = 257
    logs = mr.make_pool(n, 0xBA7 + m)
    pts = points.of(logs)
    offsets = _batch_offsets(n, m)
    lens = [b - a for a, b in zip(offsets, offsets[1:])]
    if m > 1:
        assert 0 in lens and 1 in lens and any(o % 64 for o in offsets[1:-1])
    sets = mr.scalar_sets(n, c, 0xBA7C + m + c, EDGE_SCALARS)
    for name in ("random", "edge", "digits", "equal", "zero"):
        run_stages(h, points, gpu_ctx, logs, pts, sets[name], c, offsets=offsets)
    for i in sorted({0, 100, n - 1}):
        spoiled = list(pts)
        spoiled[i] = mr.off_curve(pts[i])
        model = run_stages(h, points, gpu_ctx, logs, spoiled, sets["random"], c, offsets=offsets, bad=(i,))
        assert sorted(model.status)[-1] == i and model.status.count(-1) == m - 1
    print("batched stages m = %d c = %d: items %s" % (m, c, ITEMS))


# ---- d. + e. slices, levels and window sums on synthetic records ---------------------------------------------------------------------------
POOL = 64


def run_synthetic(h, points, recs, c, S):
    """mt_prepare on the 64-point pool (repeated up to the layout's item count, scalars zero), then rec, counts, cursor and total
    written by the test, then mt_reduce with slices of S records"""
    W = mr.windows(c)
    n = max(POOL, mr.div_up(len(recs), W))
    logs64 = mr.make_pool(POOL, 0x5E7, torsion_first=True)
    logs = [logs64[i % POOL] for i in range(n)]
    L = h.layout(n, 1, c, 0 if S == 8 else S)
    assert L is not None and L["S1"] == S and h.layout(n, 1, c)["S1"] == 8
    mr.validate_synthetic(recs, L["keys"], POOL, L["records"])
    model = mr.Model.synthetic(logs, recs, c)
    assert model.M == L["keys"] and L["levels"] == h.lib.mt_level_count(L["records"], S) == mr.level_count(L["records"], S)
    block = h.filled(L["bytes"])
    size, P = block.numel(), block.data_ptr()
    d_pts, d_sc = h.upload(mr.pack_points(points.of(logs))), h.upload(np.zeros(n * 32, dtype=np.uint8))
    assert h.lib.mt_prepare(P, size, d_pts.data_ptr(), d_sc.data_ptr(), n, c, None) == 0
    h.sync()
    assert not h.read(block, L["o_counts"], model.M, np.uint32).any() and int(h.read(block, L["o_status"], 1, np.int64)[0]) == -1
    mr.validate_counts(model, model.counts, model.cursor, model.total, L["records"])
    h.write(block, L["o_counts"], model.counts)
    h.write(block, L["o_cursor"], model.cursor)
    h.write(block, L["o_total"], np.array([model.total], dtype=np.uint64))
    h.write(block, L["o_rec"], model.records)
    which = h.lib.mt_reduce(P, size, n, 1, c, 0 if S == 8 else S, None)
    assert which == len(mr.group_passes(L["G"])) % 2
    h.sync()
    what = (c, S, len(recs))
    _none(mr.check_buckets(model, points, h.read(block, L["o_buckets"], model.M * mr.ENTRY_WORDS, np.uint32), model.counts), ("buckets",) + what)
    _none(mr.check_window_sums(model, points, h.read(block, L["o_w1" if which else "o_w0"], model.W * mr.ENTRY_WORDS, np.uint32)),
          ("window sums",) + what)
    _count("synthetic records", len(recs))
    _count("buckets", len(model.bucket_logs))
    _count("window sums", model.W)
    return model, L


def _run(rnd, key, length):
    return [(key, rnd.randrange(POOL), rnd.randrange(2)) for _ in range(length)]


def _aligned_runs(rnd, S):
    """runs of S-1, S, S+1, 2S, 2S+1, 8S and 64S+3 records, each starting at slice offset 0, 1 and S-1 (filler runs in between);
    returns (records, [(start, length)])"""
    recs, runs, key = [], [], 0
    for length in (S - 1, S, S + 1, 2 * S, 2 * S + 1, 8 * S, 64 * S + 3):
        for off in (0, 1, S - 1):
            pad = (off - len(recs)) % S
            if pad:
                recs += _run(rnd, key, pad)
                key += rnd.choice((1, 2, 9))
            runs.append((len(recs), length))
            recs += _run(rnd, key, length)
            key += rnd.choice((1, 2, 9))
    return recs, runs


@pytest.mark.parametrize("S", [8, 16, 32, 64])
def test_slices_and_levels_on_synthetic_records(h, points, S):
    c = 4
    rnd = random.Random(0x511CE + S)
    M = mr.windows(c) * mr.buckets(c)
    lists = {}
    recs, runs = _aligned_runs(rnd, S)
    assert {(s % S, ln) for s, ln in runs} == {(o, ln) for o in (0, 1, S - 1) for ln in (S - 1, S, S + 1, 2 * S, 2 * S + 1, 8 * S, 64 * S + 3)}
    assert len(recs) < 20000 and recs[-1][0] < M
    lists["aligned_runs"] = recs
    for length in (1, S, 8 * 8 * S + 1):                                               # T = 1; one slice; a key partial over the levels
        lists["one_key_%d" % length] = _run(rnd, 77, length)
    lists["every_record_its_own_key"] = [r for key in range(M) for r in _run(rnd, key, 1)]      # T = 512: a multiple of every S
    assert len(lists["every_record_its_own_key"]) % S == 0
    alt = []
    for k in range(M // 2):
        alt += _run(rnd, 2 * k, 1) + _run(rnd, 2 * k + 1, S)
    assert len(alt) < 20000
    lists["alternating_1_and_S"] = alt
    # a doubling inside ext_madd (P, P), a live bucket that is the identity (P, -P), runs of torsion points; items 0 .. 7 are j T8
    special = [(3, 20, 0), (3, 20, 0), (4, 21, 0), (4, 21, 1), (5, 8, 0), (5, 9, 0)]
    special += [(9, t, 0) for t in range(8)] + [(10, 4, 0), (10, 4, 0)] + [(11, t % 8, t & 1) for t in range(3 * S + 1)]
    special += [(12, 22, 1)] * (S + 1) + _run(rnd, 40, S - 3)
    lists["doubling_cancelling_torsion"] = special
    for name, recs in lists.items():
        model, L = run_synthetic(h, points, recs, c, S)
        if name == "one_key_%d" % (8 * 8 * S + 1):
            assert L["levels"] >= 3 and h.lib.mt_level_count(L["records"], S) >= 3       # three levels, from the schedule itself
        if name == "one_key_1":
            assert model.total == 1 and L["slices1"] >= 64                               # a list much shorter than the launch bound
        if name == "doubling_cancelling_torsion":
            assert model.bucket_logs[4] == mr.IDENTITY_LOG and model.bucket_logs[8 - 3] == mr.IDENTITY_LOG
            assert model.bucket_logs[3] == mr.lmul(2, model.logs[20]) and model.bucket_logs[10] == mr.IDENTITY_LOG
    print("slices S = %d (reached from the layout: S1 = %d): %d lists; items %s" % (S, L["S1"], len(lists), ITEMS))


def test_the_slice_override_is_refused_where_it_does_not_fit(h):
    assert h.layout(64, 1, 4, 16)["S1"] == 16 and h.layout(64, 1, 4, 64)["slices1"] == 64
    assert h.layout(64, 1, 4, 12) is None and h.layout(64, 1, 3) is None and h.layout(64, 1, 21) is None and h.layout(0, 1, 4) is None
    n = (1 << 21) // mr.windows(20) + 64                      # the product's own choice is 16 here: nothing to widen
    assert h.layout(n, 1, 20)["S1"] == 16 and h.layout(n, 1, 20, 32) is None
    L = h.layout(64, 1, 4)
    block = h.filled(L["bytes"])
    assert h.lib.mt_scan(block.data_ptr(), L["bytes"] - 1, 64, 1, 4, None) == -1
    assert h.lib.mt_reduce(block.data_ptr(), L["bytes"], 64, 1, 4, 12, None) == -1
    assert h.lib.mt_finish(block.data_ptr(), L["bytes"], 64, 4, 2, None) == -1
    assert h.lib.mt_prepare(block.data_ptr(), L["bytes"], None, None, 64, 4, None) == -1


@pytest.mark.parametrize("c", [7, 10])
def test_window_sums_with_chosen_occupancy(h, points, c):
    W, B = mr.windows(c), mr.buckets(c)
    G = B // mr.SEG
    g = G // 2
    rnd = random.Random(0x0CC + c)
    occupancy = {"only_bucket_1": [1], "only_bucket_B": [B], "around_a_segment_edge": [8 * g, 8 * g + 1], "all": list(range(1, B + 1))}
    for name, bs in occupancy.items():
        recs = []
        for j in range(W):
            for b in bs:
                recs += _run(rnd, j * B + b - 1, 1 + (j + b) % 2)
        model, L = run_synthetic(h, points, recs, c, 8)
        assert set(k % B + 1 for k in model.by_key) == set(bs) and L["G"] == G
        if name == "around_a_segment_edge":
            assert (8 * g - 1) // mr.SEG == g - 1 and (8 * g) // mr.SEG == g and 0 < g < G      # the last bucket of one segment, the first of the next
    print("window sums c = %d (G = %d, passes %s): items %s" % (c, G, mr.group_passes(G), ITEMS))
