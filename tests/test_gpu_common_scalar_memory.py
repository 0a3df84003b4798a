"""The memory contract of the six functions of include/bjj_hip_common_scalar.h, under the guarded arenas of tests/memguard.py.
Every array of a call -- inputs included -- sits inside guards, the device pointers at the contract's minimum alignment (16 bytes
and no more, ok at an odd address), the host pointers at any offset.  Per call: return code 0 and the bytes of the yardstick
(bjj_mul_var_base + bjj_point_add; Context.elgamal_decrypt); every guard byte and every input byte unchanged; the same bytes for two
different presets of the output regions; n == 0 and a rejected call leave the outputs as they were.  The scalar is a host array of
the call like any other: unchanged.  TABLE names every pointer-taking function of the header, and a CPU test holds the header to it."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pack, unpack
from memguard import DeviceArena, HostArena

TABLE = {
    "bjj_mul_common": ([("scalar", 32, "1"), ("pts_xy", 64, "n"), ("add_xy", 64, "n")], [("out_xy", 64, "n"), ("ok", 1, "n")]),
    "bjj_mul_common_dev": ([("scalar", 32, "1"), ("d_pts_xy", 64, "n"), ("d_add_xy", 64, "n")], [("d_out_xy", 64, "n"), ("d_ok", 1, "n")]),
    "bjj_in_subgroup": ([("pts_xy", 64, "n")], [("ok", 1, "n")]),
    "bjj_in_subgroup_dev": ([("d_pts_xy", 64, "n")], [("d_ok", 1, "n")]),
    "bjj_elgamal_decrypt": ([("table", 0, "handle"), ("sk", 32, "1"), ("c1_xy", 64, "n"), ("c2_xy", 64, "n")], [("out_m", 8, "n"), ("ok", 1, "n")]),
    "bjj_elgamal_decrypt_dev": ([("table", 0, "handle"), ("sk", 32, "1"), ("d_c1_xy", 64, "n"), ("d_c2_xy", 64, "n")],
                                [("d_out_m", 8, "n"), ("d_ok", 1, "n")]),
}
SIZES = (1, 65, 257)
L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
KEY = 0x05A1B2C3D4E5F60718293A4B5C6D7E8F9A0B1C2D3E4F5061728394A5B6C7D8E9
DEV_OFFS = {"min_alignment": (16, 16, 16, 33), "mixed": (48, 240, 112, 1)}           # the two inputs, the 16-byte output, ok (mod 256)
HOST_OFFS = {"pageable": (1, 33, 8, 100), "pinned": (16, 0, 240, 251), "pinned_misaligned": (8, 100, 20, 3)}


class ByteDeviceArena(DeviceArena):
    """the device arena with byte-granular offsets: d_ok may sit at any address"""
    max_off_step = 1


def test_every_pointer_function_of_the_header_has_a_row():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bjj_hip_common_scalar.h")).read(), flags=re.S)
    have = {m.group(1): m.group(2) for m in re.finditer(r"\b(bjj_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt) if "*" in m.group(2)}
    assert sorted(have) == sorted(TABLE) and len(have) == 6
    for f, (ins, outs) in TABLE.items():          # every pointer parameter but the context and the stream is an array of the row
        params = [p.split()[-1].lstrip("*") for p in have[f].split(",") if "*" in p]
        assert params == ["ctx"] + [a[0] for a in ins + outs] + (["stream"] if f.endswith("_dev") else []), f


@pytest.fixture(scope="module")
def data(gpu_ctx):
    """ciphertexts (C1, C2) under KEY with an off-curve record in each array, and per n the bytes of the yardsticks; computed once"""
    from babyjubjub_rs_amd import api
    rng = np.random.default_rng(0x3E5)
    nmax = max(SIZES)
    ms = [int(v) for v in rng.integers(0, 1 << 12, nmax)]
    rs = [int.from_bytes(rng.bytes(31), "little") for _ in range(nmax)]
    pk = tuple(unpack(gpu_ctx.mul_fixed_base(pack([KEY % L])), 2)[0])
    base = gpu_ctx.base(pk, 8)
    try:
        c1 = gpu_ctx.mul_fixed_base(pack(rs)).reshape(nmax, 64).copy()
        c2 = gpu_ctx.mul_bases([None, base], [pack(ms), pack(rs)]).reshape(nmax, 64).copy()
    finally:
        base.close()
    c1[64, 0] ^= 1                                           # present from n = 65 on
    c2[200, 32] ^= 1
    table = gpu_ctx.dlog_table(None, 8)
    t = gpu_ctx.mul_var_base(c1, np.tile(pack([KEY]), nmax))
    t[64] = 0
    full = gpu_ctx.point_add(c2, api._negate_x(t)).reshape(nmax, 64).copy()
    bad = np.zeros(nmax, bool)
    bad[[64, 200]] = True
    full[bad] = 0
    lp = gpu_ctx.mul_var_base(c1, np.tile(pack([L]), nmax)).reshape(nmax, 64)
    ident = pack([(0, 1)])
    sub = np.array([2 if i == 64 else 1 if (lp[i] == ident).all() else 0 for i in range(nmax)], np.uint8)
    assert sub[0] == 1 and sub[64] == 2
    want = {}
    for n in SIZES:
        m, ok = gpu_ctx.elgamal_decrypt(table, KEY, c1[:n], c2[:n], 12)
        want[n] = {"out": full[:n].copy(), "ok": np.where(bad[:n], 2, 1).astype(np.uint8), "sub": sub[:n].copy(), "m": m, "dok": ok}
        assert [int(v) for v in m[:5]] == ms[:min(n, 5)] and (n < 65 or ok[64] == 2)
    for a in (c1, c2):
        a.setflags(write=False)
    yield c1, c2, table, want
    table.close()


def _run(gpu_ctx, data, make_arena, dev):
    """the three call families through one arena layout; make_arena(inputs, outputs, fill) -> arena"""
    c1, c2, table, want = data
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    key = pack([KEY])
    tail = (None,) if dev else ()
    for n in SIZES:
        w = want[n]
        calls = {
            "mul_common": ([("a", c1[:n]), ("b", c2[:n])], [("o", n * 64), ("ok", n)],
                           lambda a, cnt, k=key: (lib.bjj_mul_common_dev if dev else lib.bjj_mul_common)(
                               h, k.ctypes.data if k is not None else None, a.ptr("a"), a.ptr("b"), 1, cnt, a.ptr("o"), a.ptr("ok"), *tail),
                           {"o": w["out"].reshape(-1), "ok": w["ok"]}),
            "in_subgroup": ([("a", c1[:n])], [("ok", n)],
                            lambda a, cnt, k=key: (lib.bjj_in_subgroup_dev if dev else lib.bjj_in_subgroup)(
                                h if k is not None else None, a.ptr("a"), cnt, a.ptr("ok"), *tail),
                            {"ok": w["sub"]}),
            "decrypt": ([("a", c1[:n]), ("b", c2[:n])], [("o", n * 8), ("ok", n)],
                        lambda a, cnt, k=key: (lib.bjj_elgamal_decrypt_dev if dev else lib.bjj_elgamal_decrypt)(
                            h, table.handle, k.ctypes.data if k is not None else None, a.ptr("a"), a.ptr("b"), cnt, 12, a.ptr("o"), a.ptr("ok"), *tail),
                        {"o": w["m"].view(np.uint8), "ok": w["dok"]}),
        }
        for name, (ins, outs, call, expect) in calls.items():
            results = []
            for fill in (0, 1):
                a = make_arena(ins, outs, fill)
                try:
                    assert call(a, n) == 0, lib.bjj_last_error()
                    gpu_ctx.sync()
                    try:
                        out = a.check()
                    except AssertionError as e:
                        raise AssertionError("%s%s n %d fill %d: %s" % (name, "_dev" if dev else "", n, fill, e)) from None
                    assert call(a, 0) == 0                                # n == 0 touches nothing
                    assert call(a, n, None) == -1                         # a rejected call (NULL scalar / ctx) writes nothing
                    gpu_ctx.sync()
                    again = a.check()
                    assert all((again[k] == out[k]).all() for k in out)
                finally:
                    a.close()
                for k, v in expect.items():
                    assert (out[k] == v).all(), (name, dev, n, fill, k)
                results.append(out)
            assert all((results[0][k] == results[1][k]).all() for k in results[0])
        assert bytes(key) == KEY.to_bytes(32, "little")                  # the scalar is read, never written


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(DEV_OFFS))
def test_device_forms(gpu_ctx, data, mode):
    offs = DEV_OFFS[mode]

    def make(ins, outs, fill):
        in_offs = offs[:2]
        a = ByteDeviceArena([(nm, arr, o) for (nm, arr), o in zip(ins, in_offs)],
                            [(nm, size, offs[3] if nm == "ok" else offs[2]) for nm, size in outs], fill=fill)
        assert a.ptr("ok") % 2 == 1 and all(a.ptr(nm) % 32 == 16 for nm, _ in ins)
        return a
    _run(gpu_ctx, data, make, True)


@pytest.mark.gpu
@pytest.mark.parametrize("mem", sorted(HOST_OFFS))
def test_host_forms(gpu_ctx, data, mem):
    offs = HOST_OFFS[mem]

    def make(ins, outs, fill):
        return HostArena([(nm, arr, o) for (nm, arr), o in zip(ins, offs[:2])],
                         [(nm, size, offs[3] if nm == "ok" else offs[2] & ~7) for nm, size in outs], fill=fill,
                         pinned_ctx=None if mem == "pageable" else gpu_ctx)
    _run(gpu_ctx, data, make, False)
