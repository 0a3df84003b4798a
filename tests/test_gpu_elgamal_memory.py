"""The memory contract of bjj_elgamal_encrypt / bjj_elgamal_encrypt_dev (include/bjj_hip_elgamal.h) under the guarded arenas of
tests/memguard.py, n = 65: every array of the call -- the four inputs included -- sits inside guards.  Per form: return code 0 and
the bytes of the library's own composition (bjj_mul_bases twice, bjj_point_add twice; zeros and ok = 2 for the one off-curve
addend); nothing outside the three output ranges is written; the inputs are unchanged; the same bytes for two different presets of
the output regions; n == 0 and a rejected call leave the outputs as they were."""
import numpy as np
import pytest

from bases_cases import scalar_array
from conftest import pack
from memguard import DeviceArena, HostArena

pytestmark = pytest.mark.gpu

N = 65
# offsets mod 256 of m, r, add_c1, add_c2, out_c1, out_c2, ok
OFFS = {"dev_all_0": (0, 0, 0, 0, 0, 0, 0), "dev_mixed": (16, 48, 240, 112, 32, 208, 144),
        "host_pageable": (1, 9, 33, 101, 7, 251, 3), "host_pinned": (16, 7, 0, 250, 8, 100, 1)}
BAD = 40


@pytest.fixture(scope="module")
def case(gpu_ctx):
    rng = np.random.default_rng(0xE17A)
    r = scalar_array(N, (8, 12), 0xE17B)
    m = rng.integers(0, 1 << 64, size=N, dtype=np.uint64)
    m[:4] = [0, 1, (1 << 64) - 1, 1 << 63]
    key = gpu_ctx.mul_fixed_base(pack([0x1234567890ABCDEF1122334455667788]))
    g_point = gpu_ctx.mul_fixed_base(pack([0x0FEDCBA987654321]))
    pk, g = gpu_ctx.base(key, 8), gpu_ctx.base(g_point, 12)
    m32 = np.zeros((N, 32), np.uint8)
    m32[:, :8] = m.view(np.uint8).reshape(N, 8)
    p1, p2 = gpu_ctx.mul_bases([g], [r]), gpu_ctx.mul_bases([g, pk], [m32, r])
    a1, a2 = np.roll(p2, 1, axis=0).copy(), np.roll(p1, 3, axis=0).copy()
    w1, w2 = gpu_ctx.point_add(a1, p1).copy(), gpu_ctx.point_add(a2, p2).copy()
    a2[BAD, 33] ^= 2
    w1[BAD] = 0
    w2[BAD] = 0
    ok = np.ones(N, np.uint8)
    ok[BAD] = 2
    yield {"g": g, "pk": pk, "m": m, "r": r, "a1": a1, "a2": a2, "want": {"c1": w1.reshape(-1), "c2": w2.reshape(-1), "ok": ok}}
    pk.close()
    g.close()


@pytest.mark.parametrize("form", sorted(OFFS))
def test_memory_contract(gpu_ctx, case, form):
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    offs = OFFS[form]
    dev = form.startswith("dev")
    g, pk = case["g"].handle.value, case["pk"].handle.value
    tail = (None,) if dev else ()
    fn = lib.bjj_elgamal_encrypt_dev if dev else lib.bjj_elgamal_encrypt
    results = []
    for fill in (0, 1):
        ins = [("m", case["m"].view(np.uint8), offs[0]), ("r", case["r"], offs[1]), ("a1", case["a1"], offs[2]), ("a2", case["a2"], offs[3])]
        outs = [("c1", N * 64, offs[4]), ("c2", N * 64, offs[5]), ("ok", N, offs[6])]
        a = DeviceArena(ins, outs, fill=fill) if dev else HostArena(ins, outs, fill=fill, pinned_ctx=gpu_ctx if form == "host_pinned" else None)
        try:
            args = (a.ptr("m"), a.ptr("r"), a.ptr("a1"), a.ptr("a2"))
            assert fn(h, g, pk, *args, N, a.ptr("c1"), a.ptr("c2"), a.ptr("ok"), *tail) == 0, lib.bjj_last_error()
            gpu_ctx.sync()
            try:
                out = a.check()
            except AssertionError as e:
                raise AssertionError("%s fill %d: %s" % (form, fill, e)) from None
            # n == 0 and rejected calls (one add array alone; no key) leave the outputs as they are
            assert fn(h, g, pk, *args, 0, a.ptr("c1"), a.ptr("c2"), a.ptr("ok"), *tail) == 0
            assert fn(h, g, pk, args[0], args[1], args[2], None, N, a.ptr("c1"), a.ptr("c2"), a.ptr("ok"), *tail) == -1
            assert fn(h, g, None, *args, N, a.ptr("c1"), a.ptr("c2"), a.ptr("ok"), *tail) == -1
            gpu_ctx.sync()
            again = a.check()
            assert all((again[k] == out[k]).all() for k in out)
        finally:
            a.close()
        for k, v in case["want"].items():
            assert (out[k] == v).all(), (form, fill, k, np.nonzero(out[k] != v)[0][:8].tolist())
        results.append(out)
    assert all((results[0][k] == results[1][k]).all() for k in results[0])
