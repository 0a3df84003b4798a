"""The model and the checkers of the MSM pipeline stages (tests/msm_ref.py), judged without a GPU.  The device layer --
wave_counter_add, the three scan kernels, the scatter, the launch schedule of slices, levels and group passes -- cannot run on the
CPU, so nothing here runs it: tests/test_gpu_msm_stages.py does, through tests/devfuzz/msm.hip.  What is judged here is what that
test relies on:
  - the model's digits are msm_emul_digits', and its final point is msm_emul_run's (csrc/msm.hpp on the CPU, tests/msm_emul) for
    every scalar set the device test uses;
  - every checker accepts stage outputs that are right by construction (written from the model itself) and reports a finding for
    each seeded mutant of them;
  - the validators of synthetic inputs refuse what would leave a buffer."""
import ctypes
import random

import numpy as np
import pytest

import msm_ref as mr
from test_msm_host import EDGE_SCALARS, emul_msm, msm_emul  # noqa: F401  (the fixture that builds tests/msm_emul)


@pytest.fixture(scope="module")
def points(oracle):
    return mr.Points(oracle)


def _call(points, n, c, name, seed=0x57A6E, bad=()):
    logs = mr.make_pool(n, seed + n)
    pts = points.of(logs)
    sc = mr.scalar_sets(n, c, seed + 31 * n + c, EDGE_SCALARS)[name]
    for i in bad:
        pts[i] = mr.off_curve(pts[i])
    return mr.Model(logs, sc, c, bad=bad), pts, sc


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def test_digits_are_the_emulated_digits(msm_emul):  # noqa: F811
    rnd = random.Random(0xD161)
    for c in range(4, 21):
        for k in EDGE_SCALARS + mr.digit_scalars(c) + [rnd.getrandbits(256) for _ in range(8)]:
            d = (ctypes.c_int * 64)()
            W = msm_emul.msm_emul_digits(int(k).to_bytes(32, "little"), c, d)
            assert W == mr.windows(c) and list(d[:W]) == mr.digits(k, c), (c, k)


def test_digit_scalars_sit_on_the_boundary():
    for c in (4, 5, 7, 8, 10, 13):
        at, above, ripple, top = (mr.digits(k, c) for k in mr.digit_scalars(c))
        half, W = 1 << (c - 1), mr.windows(c)
        assert at.count(half) >= W - 2 and min(at) >= 0                       # v == 2^(c-1): the digit itself, no carry
        assert above[0] == half + 1 - (1 << c) and above.count(-(half - 2)) >= W - 4   # v > 2^(c-1): negative, and a carry into every window
        assert ripple[0] == half + 1 - (1 << c) and all(d == 0 for d in ripple[1:(253 // c)]) and sum(1 for d in ripple[1:] if d) == 1
        assert top[:-1] == [0] * (W - 1) and top[-1] == 1


@pytest.mark.parametrize("c", [4, 7])
@pytest.mark.parametrize("n", [1, 65, 257])
def test_the_models_final_point_is_the_emulated_pipelines(msm_emul, points, n, c):  # noqa: F811
    for name in mr.scalar_sets(1, c, 0, EDGE_SCALARS):
        model, pts, sc = _call(points, n, c, name)
        want, st = emul_msm(msm_emul, pts, sc, c)
        assert st == -1 and mr.unpack_points(model.results(points))[0] == want, (name, n, c)
        assert model.total == int(model.counts.sum()) <= n * model.W
    model, pts, sc = _call(points, 65, c, "random", bad=(40, 7))
    assert emul_msm(msm_emul, pts, sc, c) == ((0, 0), 7) and model.status == [7] and model.red[7] == model.red[40] == 0
    assert mr.unpack_points(model.results(points))[0] == (0, 0) and not any(i in (7, 40) for rs in model.by_key.values() for i, _ in rs)


def test_the_batched_model_is_one_model_per_segment(points):
    n, c = 65, 5
    logs = mr.make_pool(n, 0xBA7C)
    sc = mr.scalar_sets(n, c, 0xBA7C, EDGE_SCALARS)["random"]
    offsets = [0, 0, 1, 1, 40, 65, 65]
    whole = mr.Model(logs, sc, c, offsets=offsets)
    assert whole.seg == [mr.segment_of(offsets, i) for i in range(n)]
    for s in range(len(offsets) - 1):
        lo, hi = offsets[s], offsets[s + 1]
        part = mr.Model(logs[lo:hi], sc[lo:hi], c)
        assert whole.result_logs[s] == part.result_logs[0]
        assert (whole.counts[s * part.M:(s + 1) * part.M] == part.counts).all()


# ---- right by construction: the stage arrays written from the model ----------------------------------------------------------------------
def _right(model, points, pts):
    red = np.array([mr.fr.words(k) for k in model.red], dtype=np.uint32)
    niels = np.zeros((model.n, mr.NIELS_WORDS), dtype=np.uint32)
    for i, p in enumerate(pts):
        if i not in model.bad:
            niels[i, :27] = mr.cr._niels_limbs(mr.cr.to_m1(p), False)
    rec = np.full(max(model.total, 1), mr.FILL64, dtype=np.uint64)
    rec[:model.total] = model.records
    bw = np.full((model.M, mr.ENTRY_WORDS), mr.FILL32, dtype=np.uint32)
    rnd = random.Random(7)
    for key, p in zip(model.bucket_logs, points.of(list(model.bucket_logs.values()))):
        bw[key] = mr.encode_ext(p, z=rnd.randrange(1, mr.R_MOD), key=key)
    ws = np.array([mr.encode_ext(p, z=rnd.randrange(1, mr.R_MOD)) for p in points.of(model.window_logs)], dtype=np.uint32)
    return dict(red=red, niels=niels, counts=model.counts.copy(), status=np.array(model.status, dtype=np.int64), cursor=model.cursor.copy(),
                total=model.total, rec=rec, buckets=bw, wsum=ws, out=model.results(points))


def _all_checks(model, points, pts, a):
    return (mr.check_prepare(model, pts, a["red"], a["niels"], a["counts"], a["status"]) + mr.check_scan(a["counts"], a["cursor"], a["total"])
            + mr.check_records(model, a["rec"], a["cursor"], a["counts"]) + mr.check_buckets(model, points, a["buckets"], a["counts"])
            + mr.check_window_sums(model, points, a["wsum"]) + mr.check_result(model, points, a["out"]))


@pytest.fixture(scope="module")
def call(points):
    model, pts, sc = _call(points, 257, 7, "random")
    return model, pts, _right(model, points, pts)


def test_checkers_accept_what_is_right_by_construction(points, call):
    model, pts, right = call
    assert _all_checks(model, points, pts, right) == []
    for name in ("edge", "digits", "one_window", "zero", "equal"):
        m2, p2, _ = _call(points, 65, 4, name)
        assert _all_checks(m2, points, p2, _right(m2, points, p2)) == [], name
    m2, p2, _ = _call(points, 65, 4, "random", bad=(64,))
    assert _all_checks(m2, points, p2, _right(m2, points, p2)) == []


def _two_neighbours(model):
    """a key with at least two records whose next key is live too"""
    for key in sorted(model.by_key):
        if model.counts[key] >= 2 and key + 1 < model.M and model.counts[key + 1] >= 1 and (key + 1) % model.B:
            return key
    raise AssertionError("no such key")


def test_mutant_a_record_moved_to_the_neighbouring_key(points, call):
    model, pts, right = call
    key = _two_neighbours(model)
    rec = right["rec"].copy()
    a, b = int(model.cursor[key + 1]) - 1, int(model.cursor[key + 1])           # the last slot of key, the first of key + 1
    rec[a], rec[b] = rec[b], rec[a]
    found = mr.check_records(model, rec, right["cursor"], right["counts"])
    assert {f[1] for f in found} == {key, key + 1}
    # ... and with its key field rewritten, so that the slot ranges look right: the sets differ
    rec = right["rec"].copy()
    rec[a] = (int(rec[a]) & ((1 << 33) - 1)) | ((key + 1) << 33)
    assert mr.check_records(model, rec, right["cursor"], right["counts"])


def test_mutant_two_records_in_one_slot(points, call):
    model, pts, right = call
    key = _two_neighbours(model)
    rec = right["rec"].copy()
    s = int(model.cursor[key])
    rec[s] = rec[s + 1]                                                        # both lanes were handed slot s ...
    rec[s + 1] = mr.FILL64                                                     # ... and slot s + 1 was never written
    found = mr.check_records(model, rec, right["cursor"], right["counts"])
    assert found and all(f[0] == "rec" for f in found)


def test_mutant_a_cursor_off_by_one(points, call):
    model, pts, right = call
    key = _two_neighbours(model)
    cursor = right["cursor"].copy()
    cursor[key] += np.uint64(1)
    assert [f[:2] for f in mr.check_scan(right["counts"], cursor, right["total"])] == [("cursor", key)]
    assert mr.check_records(model, right["rec"], cursor, right["counts"])       # the key's range now ends in the neighbour's
    assert [f[0] for f in mr.check_scan(right["counts"], right["cursor"], right["total"] + 1)] == ["total"]


def test_mutant_a_sign_bit_flipped(points, call):
    model, pts, right = call
    key = _two_neighbours(model)
    rec = right["rec"].copy()
    rec[int(model.cursor[key])] ^= np.uint64(1)
    assert {f[1] for f in mr.check_records(model, rec, right["cursor"], right["counts"])} == {key}


def test_mutant_a_bucket_missing_one_point(points, call):
    model, pts, right = call
    key = _two_neighbours(model)
    item, neg = model.by_key[key][-1]
    less = mr.ladd(model.bucket_logs[key], mr.lneg(model.logs[item]) if not neg else model.logs[item])
    bw = right["buckets"].copy()
    bw[key] = mr.encode_ext(points.of([less])[0], key=key)
    assert [f[:2] for f in mr.check_buckets(model, points, bw, right["counts"])] == [("bucket", key)]
    bw = right["buckets"].copy()
    bw[key, 27] ^= 1                                                           # T no longer X Y / Z: the next addition would read it
    assert [f[:2] for f in mr.check_buckets(model, points, bw, right["counts"])] == [("bucket", key)]


def test_mutant_a_bucket_written_for_a_key_with_count_zero(points, call):
    model, pts, right = call
    dead = int(np.nonzero(model.counts == 0)[0][3])
    bw = right["buckets"].copy()
    bw[dead] = mr.encode_ext((0, 1), key=dead)
    assert [f[:2] for f in mr.check_buckets(model, points, bw, right["counts"])] == [("bucket", dead)]
    assert mr.check_buckets(model, points, bw, right["counts"], fill=False) == []
    counts = right["counts"].copy()
    counts[dead] = 1                                                           # ... and a count without a record
    assert mr.check_buckets(model, points, right["buckets"], counts)


def test_mutant_a_window_sum_missing_the_segment_term(points, call):
    model, pts, right = call
    wrong = model.window_logs_without_the_segment_term()
    differ = [j for j in range(model.W) if wrong[j] != model.window_logs[j]]
    assert len(differ) >= model.W - 2                                          # every window with a live bucket above the first segment
    ws = np.array([mr.encode_ext(p) for p in points.of(wrong)], dtype=np.uint32)
    assert [f[1] for f in mr.check_window_sums(model, points, ws)] == differ[:mr.MAX_FINDINGS]
    out = right["out"].copy()
    out[0, 0] ^= 1
    assert mr.check_result(model, points, out)


def test_mutant_a_counter_result_that_repeats_a_position():
    keys = [3] * 40 + [5] * 24
    active = [1] * 64
    active[10] = 0
    for bits, init in ((32, 0), (32, (1 << 32) - 2), (64, (1 << 32) - 7)):
        before = [init] * 8
        after = list(before)
        after[3] = (init + 39) % (1 << bits)
        after[5] = (init + 24) % (1 << bits)
        ret, nxt = [0] * 64, {3: init, 5: init}
        for i in range(64):
            if active[i]:
                ret[i] = nxt[keys[i]] % (1 << bits)
                nxt[keys[i]] += 1
        ret[10] = 0xDEAD                                                       # an inactive lane: anything
        assert mr.check_counter(bits, init, keys, active, ret, before, after) == []
        mut = list(ret)
        mut[20] = mut[19]
        assert [f[1] for f in mr.check_counter(bits, init, keys, active, mut, before, after)] == [3]
        grown = list(after)
        grown[5] = (grown[5] + 1) % (1 << bits)
        assert [f[1] for f in mr.check_counter(bits, init, keys, active, ret, before, grown)] == [5]
        if bits == 64:                                                         # the high word of the base lost on its way across the lanes
            low = [v & 0xffffffff if i >= 32 else v for i, v in enumerate(ret)]
            assert mr.check_counter(bits, init, keys, active, low, before, after)


# ---- the validators ------------------------------------------------------------------------------------------------------------------------
def test_validators_refuse_what_would_leave_a_buffer():
    good = [(0, 1, 0), (0, 2, 1), (3, 63, 0), (511, 0, 1)]
    assert mr.validate_synthetic(good, 512, 64, 4096)
    for bad in ([(3, 1, 0), (2, 1, 0)],            # unsorted keys
                [(0, 64, 0)],                      # an item past the pool
                [(512, 0, 0)],                     # a key past the histogram
                [(0, -1, 0)], [(0, 0, 2)]):
        with pytest.raises(ValueError):
            mr.validate_synthetic(bad, 512, 64, 4096)
    with pytest.raises(ValueError):
        mr.validate_synthetic(good, 512, 64, 3)    # more records than the layout holds
    logs = mr.make_pool(64, 1, torsion_first=True)
    model = mr.Model.synthetic(logs, good, 4)
    assert mr.validate_counts(model, model.counts, model.cursor, model.total, 4096)
    counts = model.counts.copy()
    counts[1] = 1
    with pytest.raises(ValueError):
        mr.validate_counts(model, counts, model.cursor, model.total, 4096)
    with pytest.raises(ValueError):
        mr.validate_counts(model, model.counts, model.cursor + np.uint64(1), model.total, 4096)
    with pytest.raises(ValueError):
        mr.validate_counts(model, model.counts, model.cursor, model.total + 1, 4096)
    with pytest.raises(ValueError):
        mr.validate_counter_input([0, 128], [1, 1], 128)


def test_the_schedule_of_the_model():
    assert [mr.slice_records(r) for r in (1, 1 << 21, (1 << 21) + 8, 1 << 23, 1 << 30)] == [8, 8, 16, 32, 64]
    assert mr.level_count(1, 8) == 0 and mr.level_count(9, 8) == 1 and mr.level_count(8 * 8 * 8 + 1, 8) >= 3
    assert [len(mr.group_passes(mr.buckets(c) // mr.SEG)) for c in (4, 5, 7, 8, 10, 13)] == [0, 1, 1, 2, 2, 3]
    assert [mr.group_passes(mr.buckets(c) // mr.SEG)[-1:] for c in (5, 8)] == [[2], [2]]
