"""The memory contract of bjj_point_sum and bjj_point_sum_dev, under the guarded arenas of tests/memguard.py.  Every array of a
call -- inputs included -- sits inside guards, the device pointers at the contract's minimum alignment (16 bytes and no more, the
sign bytes at an odd address), the host pointers at any offset.  Per call: return code 0 and the bytes bjj_msm_batch gives with
unit scalars; every guard byte and every input byte -- offsets array included -- unchanged; the same bytes for two different
presets of the output regions; with offsets that break their contract only the two output arrays change.  TABLE names every
pointer-taking function of include/bjj_hip_point_sum.h, and a CPU test holds the header to it."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from memguard import DeviceArena, HostArena

TABLE = {
    "bjj_point_sum": ([("pts_xy", 64, "n"), ("neg", 1, "n"), ("offsets", 8, "m+1")], [("out_xy", 64, "m"), ("out_first_off_curve", 8, "m")]),
    "bjj_point_sum_dev": ([("d_pts_xy", 64, "n"), ("d_neg", 1, "n"), ("d_offsets", 8, "m+1")],
                          [("d_out_xy", 64, "m"), ("d_first_off_curve", 8, "m")]),
}
T = int(re.search(r"^#define PSUM_TILE (\d+)\b", open(os.path.join(ROOT, "babyjubjub-rs_amd", "csrc", "point_sum.hpp")).read(),
                  flags=re.M).group(1))
SIZES = (1, T + 1, 2 * T + 3)
DEV_OFFS = {"min_alignment": (16, 33, 16, 16, 16), "mixed": (48, 1, 80, 112, 240)}      # pts, neg, offsets, out, status (mod 256)
HOST_OFFSETS = {"pageable": (0, 1, 8, 33, 100, 16, 250), "pinned": (16, 48, 0, 240, 112, 80, 32), "pinned_misaligned": (8, 1, 33, 100, 20, 250, 4)}


class ByteDeviceArena(DeviceArena):
    """the device arena with byte-granular offsets: d_neg may sit at any address"""
    max_off_step = 1


def test_every_pointer_function_of_the_header_has_a_row():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bjj_hip_point_sum.h")).read(), flags=re.S)
    have = {m.group(1): m.group(2) for m in re.finditer(r"\b(bjj_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt) if "*" in m.group(2)}
    assert sorted(have) == sorted(TABLE) and len(have) == 2
    for f, (ins, outs) in TABLE.items():          # every pointer parameter but the context and the stream is an array of the row
        params = [p.split()[-1].lstrip("*") for p in have[f].split(",") if "*" in p]
        assert params == ["ctx"] + [a[0] for a in ins + outs] + (["stream"] if f.endswith("_dev") else []), f


def _segments(n, m):
    return [0, n] if m == 1 else list(range(n + 1))


def _bad(n, m):
    """offsets that break their contract: a decrease for m >= 2, else a last value that is not n"""
    if m == 1:
        return [0, n + 1]
    off = list(range(n + 1))
    off[m // 2] = n + 5
    return off


@pytest.fixture(scope="module")
def data(gpu_ctx, golden):
    """inputs, and per (n, m) the expected bytes: bjj_msm_batch with the scalars 1 and 8l - 1; computed once, never written"""
    from test_gpu_msm import group_points
    from test_gpu_point_sum import unit_scalars
    nmax = max(SIZES)
    pts = group_points(gpu_ctx, golden, nmax, seed_offset=0x3E4).copy()
    pts[T, 0] ^= 1                                          # one off-curve point, present from n = T + 1 on
    neg = (np.random.RandomState(0x3E4).randint(0, 2, size=nmax) * 0x81).astype(np.uint8)
    want = {}
    for n in SIZES:
        for m in (1, n):
            want[(n, m)] = gpu_ctx.msm_batch(pts[:n], unit_scalars(n, neg[:n]), _segments(n, m))
    assert want[(T + 1, 1)][1].tolist() == [T] and want[(2 * T + 3, 2 * T + 3)][1][T] == T and want[(1, 1)][1].tolist() == [-1]
    for a in (pts, neg):
        a.setflags(write=False)
    return pts, neg, want


def _units(n, m):
    return {"n": n, "m": m, "m+1": m + 1}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(DEV_OFFS))
def test_device_form(gpu_ctx, data, mode):
    pts, neg, want = data
    offs = DEV_OFFS[mode]
    ins_t, outs_t = TABLE["bjj_point_sum_dev"]
    for n in SIZES:
        for m in sorted({1, n}):
            for segs, forced in ((_segments(n, m), None), (_bad(n, m), -2)):
                wout, wst = want[(n, m)] if forced is None else (np.zeros((m, 64), np.uint8), np.full(m, -2, np.int64))
                arrays = [pts[:n], neg[:n], np.asarray(segs, np.uint64).view(np.uint8)]
                results = []
                for fill in (0, 1):
                    a = ByteDeviceArena([(t[0], arr, o) for t, arr, o in zip(ins_t, arrays, offs)],
                                        [(t[0], t[1] * _units(n, m)[t[2]], o) for t, o in zip(outs_t, offs[3:])], fill=fill)
                    assert a.ptr("d_neg") % 2 == 1 and all(a.ptr(k) % 32 == 16 for k in ("d_pts_xy", "d_offsets", "d_out_xy", "d_first_off_curve"))
                    rc = gpu_ctx.lib.bjj_point_sum_dev(gpu_ctx.handle, a.ptr("d_pts_xy"), a.ptr("d_neg"), n, a.ptr("d_offsets"), m,
                                                       a.ptr("d_out_xy"), a.ptr("d_first_off_curve"), None)
                    assert rc == 0, gpu_ctx.lib.bjj_last_error()
                    gpu_ctx.sync()
                    try:
                        out = a.check()
                    except AssertionError as e:
                        raise AssertionError("bjj_point_sum_dev offsets %s %s, n %d, m %d, bad %s, fill %d: %s"
                                             % (mode, offs, n, m, forced is not None, fill, e)) from None
                    assert (out["d_out_xy"].reshape(m, 64) == wout).all(), (mode, n, m, forced, fill)
                    assert (out["d_first_off_curve"].view(np.int64) == wst).all(), (mode, n, m, forced, fill)
                    results.append(out)
                assert all((results[0][k] == results[1][k]).all() for k in results[0])


@pytest.mark.gpu
@pytest.mark.parametrize("mem", sorted(HOST_OFFSETS))
def test_host_form(gpu_ctx, data, mem):
    pts, neg, want = data
    ins_t, outs_t = TABLE["bjj_point_sum"]
    choices = HOST_OFFSETS[mem]
    for k, n in enumerate(SIZES):
        for m in sorted({1, n}):
            wout, wst = want[(n, m)]
            arrays = [pts[:n], neg[:n], np.asarray(_segments(n, m), np.uint64).view(np.uint8)]
            results = []
            for fill in (0, 1):
                offs = [choices[(j + k + fill) % len(choices)] for j in range(5)]
                offs[2] &= ~7                                      # uint64 offsets and int64 status words: naturally aligned, as
                offs[4] &= ~7                                      # the C types ask
                a = HostArena([(t[0], arr, o) for t, arr, o in zip(ins_t, arrays, offs)],
                              [(t[0], t[1] * _units(n, m)[t[2]], o) for t, o in zip(outs_t, offs[3:])], fill=fill,
                              pinned_ctx=None if mem == "pageable" else gpu_ctx)
                try:
                    rc = gpu_ctx.lib.bjj_point_sum(gpu_ctx.handle, a.ptr("pts_xy"), a.ptr("neg"), n, a.ptr("offsets"), m, a.ptr("out_xy"),
                                                   a.ptr("out_first_off_curve"))
                    assert rc == 0, gpu_ctx.lib.bjj_last_error()
                    try:
                        out = a.check()
                    except AssertionError as e:
                        raise AssertionError("bjj_point_sum (%s) offsets %s, n %d, m %d, fill %d: %s" % (mem, offs, n, m, fill, e)) from None
                    # a rejected call (bad offsets) writes nothing at all
                    bad = np.asarray(_bad(n, m), np.uint64)
                    assert gpu_ctx.lib.bjj_point_sum(gpu_ctx.handle, a.ptr("pts_xy"), a.ptr("neg"), n, bad.ctypes.data, m, a.ptr("out_xy"),
                                                     a.ptr("out_first_off_curve")) == -1
                    again = a.check()
                    assert all((again[key] == out[key]).all() for key in out)
                finally:
                    a.close()
                assert (out["out_xy"].reshape(m, 64) == wout).all() and (out["out_first_off_curve"].view(np.int64) == wst).all(), (mem, n, m, fill)
                results.append(out)
            assert all((results[0][key] == results[1][key]).all() for key in results[0])
