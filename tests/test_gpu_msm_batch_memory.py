"""The memory contract of bjj_msm_batch and bjj_msm_batch_dev, under the guarded arenas of tests/memguard.py and with the array
offsets of tests/test_gpu_memory_contract.py (device: all 0, all 16, mixed 16-byte multiples; host: any offset, pageable and
pinned).  Per call: return code 0 and the expected bytes; every guard byte and every input byte -- offsets array included --
unchanged; the same bytes for two different presets of the output regions.  TABLE names every pointer-taking function of
include/bjj_hip_msm_batch.h, and a CPU test holds the header to it."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from memguard import DeviceArena, HostArena

# function -> (input arrays: name, bytes per unit, unit; output arrays likewise); unit "n": per item, "m+1" / "m": per segment
TABLE = {
    "bjj_msm_batch": ([("pts_xy", 64, "n"), ("scalars", 32, "n"), ("offsets", 8, "m+1")], [("out_xy", 64, "m"), ("out_first_off_curve", 8, "m")]),
    "bjj_msm_batch_dev": ([("d_pts_xy", 64, "n"), ("d_scalars", 32, "n"), ("d_offsets", 8, "m+1")],
                          [("d_out_xy", 64, "m"), ("d_first_off_curve", 8, "m")]),
}
DEV_MODES = {"all_0": (0, 0, 0, 0, 0), "all_16": (16, 16, 16, 16, 16), "mixed": (16, 48, 80, 112, 240), "mixed_rot": (240, 16, 48, 80, 112)}
HOST_OFFSETS = {"pageable": (0, 1, 8, 33, 100, 16, 250), "pinned": (16, 48, 0, 240, 112, 80, 32), "pinned_misaligned": (8, 1, 33, 100, 20, 250, 4)}
SEGMENTS = [0, 1, 1, 2, 64, 65, 129, 300]


def test_every_pointer_function_of_the_header_has_a_row():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bjj_hip_msm_batch.h")).read(), flags=re.S)
    have = {m.group(1): m.group(2) for m in re.finditer(r"\b(bjj_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt) if "*" in m.group(2)}
    assert sorted(have) == sorted(TABLE) and len(have) == 2
    for f, (ins, outs) in TABLE.items():          # every pointer parameter but the context and the stream is an array of the row
        params = [p.split()[-1].lstrip("*") for p in have[f].split(",") if "*" in p]
        assert params == ["ctx"] + [a[0] for a in ins + outs] + (["stream"] if f.endswith("_dev") else []), f


@pytest.fixture(scope="module")
def data(gpu_ctx, golden):
    """inputs, and per scenario (offending points) the expected bytes: bjj_msm of every slice; computed once, never written"""
    from test_gpu_msm import group_points, raw_msm, scalars
    pts = group_points(gpu_ctx, golden, 300, seed_offset=0x3E3)
    sc = scalars(300, offset=0x3E3)
    cases = {}
    for name, bad in (("clean", []), ("off_curve", [66, 100, 299])):
        p = pts.copy()
        for i in bad:
            p[i, 0] ^= 1
        out, st = [], []
        for a, b in zip(SEGMENTS, SEGMENTS[1:]):
            o, s = raw_msm(gpu_ctx, p[a:b], sc[a:b])
            out.append(o)
            st.append(s + a if s >= 0 else s)      # bjj_msm counts inside the slice, the batch inside the whole array
        p.setflags(write=False)
        cases[name] = (p, np.concatenate(out), np.array(st, np.int64))
    assert cases["off_curve"][2].tolist() == [-1, -1, -1, -1, -1, 66, 299]
    sc.setflags(write=False)
    return sc, cases


def _units(n, m):
    return {"n": n, "m": m, "m+1": m + 1}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(DEV_MODES))
def test_device_form(gpu_ctx, data, mode):
    sc, cases = data
    offs = DEV_MODES[mode]
    ins_t, outs_t = TABLE["bjj_msm_batch_dev"]
    bad3 = [0, 200, 100, 300]
    runs = [(cases["clean"], SEGMENTS, 0, None), (cases["clean"], SEGMENTS, 4, None), (cases["off_curve"], SEGMENTS, 0, None),
            (cases["clean"], [0, 0, 0], 0, None), (cases["clean"], bad3, 0, -2)]
    for (pts, want, wst), segs, wb, forced in runs:
        m, n = len(segs) - 1, segs[-1] if forced is None else 300
        if forced is not None:
            want, wst = np.zeros((m, 64), np.uint8), np.full(m, -2, np.int64)
        elif n == 0:
            want, wst = np.zeros((m, 64), np.uint8), np.full(m, -1, np.int64)
            want[:, 32] = 1                                        # the identity (0, 1)
        arrays = [pts[:max(n, 1)], sc[:max(n, 1)], np.asarray(segs, np.uint64).view(np.uint8)]
        results = []
        for fill in (0, 1):
            a = DeviceArena([(t[0], arr, o) for t, arr, o in zip(ins_t, arrays, offs)],
                            [(t[0], t[1] * _units(n, m)[t[2]], o) for t, o in zip(outs_t, offs[3:])], fill=fill)
            rc = gpu_ctx.lib.bjj_msm_batch_dev(gpu_ctx.handle, a.ptr("d_pts_xy"), a.ptr("d_scalars"), n, a.ptr("d_offsets"), m, wb,
                                               a.ptr("d_out_xy"), a.ptr("d_first_off_curve"), None)
            assert rc == 0, gpu_ctx.lib.bjj_last_error()
            gpu_ctx.sync()
            try:
                out = a.check()
            except AssertionError as e:
                raise AssertionError("bjj_msm_batch_dev offsets %s %s, segments %s, fill %d: %s" % (mode, offs, segs, fill, e)) from None
            assert (out["d_out_xy"].reshape(m, 64) == want).all(), (mode, segs, wb, fill)
            assert (out["d_first_off_curve"].view(np.int64) == wst).all(), (mode, segs, wb, fill)
            results.append(out)
        assert all((results[0][k] == results[1][k]).all() for k in results[0])


@pytest.mark.gpu
@pytest.mark.parametrize("mem", sorted(HOST_OFFSETS))
def test_host_form(gpu_ctx, data, mem):
    sc, cases = data
    ins_t, outs_t = TABLE["bjj_msm_batch"]
    choices = HOST_OFFSETS[mem]
    m, n = len(SEGMENTS) - 1, 300
    for k, name in enumerate(("clean", "off_curve")):
        pts, want, wst = cases[name]
        arrays = [pts, sc, np.asarray(SEGMENTS, np.uint64).view(np.uint8)]
        results = []
        for fill in (0, 1):
            offs = [choices[(j + k + fill) % len(choices)] for j in range(5)]
            offs[2] &= ~7                                          # uint64 offsets and int64 status words: naturally aligned, as
            offs[4] &= ~7                                          # the C types ask
            a = HostArena([(t[0], arr, o) for t, arr, o in zip(ins_t, arrays, offs)],
                          [(t[0], t[1] * _units(n, m)[t[2]], o) for t, o in zip(outs_t, offs[3:])], fill=fill,
                          pinned_ctx=None if mem == "pageable" else gpu_ctx)
            try:
                rc = gpu_ctx.lib.bjj_msm_batch(gpu_ctx.handle, a.ptr("pts_xy"), a.ptr("scalars"), n, a.ptr("offsets"), m, 0, a.ptr("out_xy"),
                                               a.ptr("out_first_off_curve"))
                assert rc == 0, gpu_ctx.lib.bjj_last_error()
                try:
                    out = a.check()
                except AssertionError as e:
                    raise AssertionError("bjj_msm_batch (%s) offsets %s, fill %d: %s" % (mem, offs, fill, e)) from None
                # a rejected call (bad offsets) writes nothing at all
                bad = np.asarray([0, 200, 100, 300], np.uint64)
                assert gpu_ctx.lib.bjj_msm_batch(gpu_ctx.handle, a.ptr("pts_xy"), a.ptr("scalars"), n, bad.ctypes.data, 3, 0, a.ptr("out_xy"),
                                                 a.ptr("out_first_off_curve")) == -1
                again = a.check()
                assert all((again[key] == out[key]).all() for key in out)
            finally:
                a.close()
            assert (out["out_xy"].reshape(m, 64) == want).all() and (out["out_first_off_curve"].view(np.int64) == wst).all(), (mem, name, fill)
            results.append(out)
        assert all((results[0][key] == results[1][key]).all() for key in results[0])
