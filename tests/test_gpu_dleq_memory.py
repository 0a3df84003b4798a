"""The memory contract of the six entry points of include/bjj_hip_dleq.h under the guarded arenas of tests/memguard.py, n = 65: every
array of a call -- the inputs included -- sits inside guards.  Per call and form: return code 0 and the bytes of the library's own
composition; nothing outside the output ranges is written; the inputs are unchanged; offsets that are only 16-byte aligned work
(_dev), any offset works for host arrays, and `ok` works at an odd address; the same bytes for two different presets of the output
regions; n == 0 and a rejected call leave the outputs as they were."""
import numpy as np
import pytest

from bases_cases import scalar_array
from conftest import pack
from memguard import FILL_SEEDS, DeviceArena, HostArena, pattern

pytestmark = pytest.mark.gpu

N = 65
L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
SK = 0x1234567890ABCDEF1122334455667788 % L
TAG = 0x0123456789ABCDEF0011223344556677
BAD = 40
ODD_PAD = 16
# offsets mod 256 of up to five inputs and five outputs; the last output is `ok`
# (a device arena places arrays at multiples of 16: there `ok` is given ODD_PAD spare bytes and the call gets its address + 1)
OFFS = {"dev_all_0": ((0, 0, 0, 0, 0), (0, 0, 0, 0, 0)), "dev_mixed": ((16, 48, 240, 112, 32), (208, 144, 80, 176, 16)),
        "host_pageable": ((1, 9, 33, 101, 7), (251, 3, 77, 130, 5)), "host_pinned": ((16, 7, 0, 250, 8), (100, 1, 64, 31, 255))}


def le(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8).copy()


@pytest.fixture(scope="module")
def case(gpu_ctx):
    """the inputs of the three calls and what the older entry points make of them"""
    g_point = gpu_ctx.mul_fixed_base(pack([0x0FEDCBA987654321]))
    g = gpu_ctx.base(g_point, 12)
    pk = gpu_ctx.base(gpu_ctx.mul_common(SK, g_point)[0], 8)
    k = scalar_array(N, (8, 12), 0xD2A0)
    w = scalar_array(2 * N, (8, 12), 0xD2A1)[N:]
    c1 = gpu_ctx.mul_fixed_base(k)
    # bjj_mul_pair: P = C1, Q = the next C1, A = the one after; one off-curve Q
    q, add = np.roll(c1, 1, axis=0).copy(), np.roll(c1, 2, axis=0).copy()
    pair = gpu_ctx.point_add(gpu_ctx.point_add(add, gpu_ctx.mul_var_base(c1, k)), gpu_ctx.mul_var_base(q, w)).copy()
    q[BAD, 33] ^= 2
    pair[BAD] = 0
    ok2 = np.ones(N, np.uint8)
    ok2[BAD] = 2
    # bjj_dleq_prove by its parts (w reduced on the host), with one off-curve C1
    wl = pack([int.from_bytes(bytes(x), "little") % L for x in w]).reshape(N, 32)
    D = gpu_ctx.mul_common(SK, c1)[0].copy()
    A, B = gpu_ctx.mul_bases([g], [wl]).copy(), gpu_ctx.mul_var_base(c1, wl).copy()
    h = gpu_ctx.poseidon5(np.concatenate([np.tile(le(TAG), (N, 1)), c1, D], axis=1))
    c = gpu_ctx.poseidon5(np.concatenate([h, A, B], axis=1))
    z = pack([(int.from_bytes(bytes(a), "little") + int.from_bytes(bytes(b), "little") % L * SK) % L for a, b in zip(wl, c)]).reshape(N, 32).copy()
    c1_bad = c1.copy()
    c1_bad[BAD, 2] ^= 1
    pD, pA, pB, pz = D.copy(), A.copy(), B.copy(), z.copy()
    for x in (pD, pA, pB, pz):
        x[BAD] = 0
    # bjj_dleq_verify: those proofs, one z spoilt, one D off the curve
    vz, vD = z.copy(), D.copy()
    vz[7, 0] ^= 1
    vD[BAD, 40] ^= 4
    okv = np.ones(N, np.uint8)
    okv[7], okv[BAD] = 0, 2
    yield {"g": g, "pk": pk,
           "pair": ([c1, k, q, w, add], {"out": pair.reshape(-1), "ok": ok2}),
           "prove": ([c1_bad, w], {"d": pD.reshape(-1), "a": pA.reshape(-1), "b": pB.reshape(-1), "z": pz.reshape(-1), "ok": ok2}),
           "verify": ([c1, vD, A, B, vz], {"ok": okv})}
    pk.close()
    g.close()


OUT_BYTES = {"pair": [("out", 64), ("ok", 1)], "prove": [("d", 64), ("a", 64), ("b", 64), ("z", 32), ("ok", 1)], "verify": [("ok", 1)]}


@pytest.mark.parametrize("form", sorted(OFFS))
@pytest.mark.parametrize("call", sorted(OUT_BYTES))
def test_memory_contract(gpu_ctx, case, call, form):
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    in_offs, out_offs = OFFS[form]
    dev = form.startswith("dev")
    g, pk = case["g"].handle.value, case["pk"].handle.value
    tag, sk = le(TAG), le(SK)
    tail = (None,) if dev else ()
    arrays, want = case[call]
    names = [nm for nm, _ in OUT_BYTES[call]]
    results = []
    for fill in (0, 1):
        ins = [("in%d" % i, x, in_offs[i]) for i, x in enumerate(arrays)]
        outs = [(nm, N * width, out_offs[-1] if nm == "ok" else out_offs[i]) for i, (nm, width) in enumerate(OUT_BYTES[call])]
        odd = form == "dev_mixed"
        if odd:
            outs = [(nm, sz + ODD_PAD if nm == "ok" else sz, off) for nm, sz, off in outs]
        a = DeviceArena(ins, outs, fill=fill) if dev else HostArena(ins, outs, fill=fill, pinned_ctx=gpu_ctx if form == "host_pinned" else None)
        try:
            ip = [a.ptr(nm) for nm, _, _ in ins]
            op = [a.ptr(nm) + (1 if odd and nm == "ok" else 0) for nm in names]

            def run(n, ip=ip, op=op, pk_=pk, keep=None):
                if call == "pair":
                    fn = lib.bjj_mul_pair_dev if dev else lib.bjj_mul_pair
                    return fn(h, ip[0], ip[1], ip[2], ip[3], ip[4], n, *op, *tail)
                if call == "verify":
                    fn = lib.bjj_dleq_verify_dev if dev else lib.bjj_dleq_verify
                    return fn(h, g, pk_, tag.ctypes.data, *ip, n, *op, *tail)
                fn = lib.bjj_dleq_prove_dev if dev else lib.bjj_dleq_prove
                return fn(h, g, sk.ctypes.data, None if keep == "no tag" else tag.ctypes.data, *ip, n, *op, *tail)
            assert run(N) == 0, lib.bjj_last_error()
            gpu_ctx.sync()
            try:
                out = a.check()
            except AssertionError as e:
                raise AssertionError("%s %s fill %d: %s" % (call, form, fill, e)) from None
            # n == 0 and a rejected call (an input missing; no key; no tag) leave the outputs as they are
            assert run(0) == 0
            assert run(N, ip=[None] + ip[1:]) == -1
            if call == "verify":
                assert run(N, pk_=None) == -1
            if call == "prove":
                assert run(N, keep="no tag") == -1
            gpu_ctx.sync()
            again = a.check()
            assert all((again[k] == out[k]).all() for k in out)
            if odd:                                          # the bytes around the shifted `ok` are still the preset
                lo = a._slot("ok").start
                preset = pattern(FILL_SEEDS[fill], lo, lo + N + ODD_PAD)
                assert out["ok"][0] == preset[0] and (out["ok"][N + 1:] == preset[N + 1:]).all()
                out["ok"] = out["ok"][1:N + 1]
        finally:
            a.close()
        for k, v in want.items():
            assert (out[k] == v).all(), (call, form, fill, k, np.nonzero(out[k] != v)[0][:8].tolist())
        results.append(out)
    assert all((results[0][k] == results[1][k]).all() for k in results[0])

