"""The wave-cooperative gather of the fixed-base table (csrc/k_common.hpp: GatherCoopLds) under its cache policy
(BJJ_GATHER_AUX, whatever the library was built with) and on both memory types of the table (bjj_init: BJJ_TABLE_UNCACHED).
Every user of the gather -- K1 in its 512-lane and its 2 x 256-lane shape, affine and compressed output (NBUF = 2), the
verify and the sign kernels (NBUF = 1) -- is compared item by item, byte for byte, with the C oracle.

W = 16: the 67 MB table builds in milliseconds.  The short-call kernels (four / eight lanes per item, k_small.hip) do not use
the cooperative gather, so the contexts of this file switch them off: every n runs the kernels under test.  Expected values
are computed once per module for the longest batch; every n compares a prefix."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = 16
SHORT = (1, 63, 64, 65, 4097)   # one lane, either side of a wave, more than one workgroup with a ragged last wave
ENV_ALL_MAIN_KERNELS = {"BJJ_FB_QUAD_MAX": "0", "BJJ_SIGN_SMALL_MAX": "0", "BJJ_VERIFY_SMALL_MAX": "0"}


def _context(uncached):
    import babyjubjub_rs_amd as bjj
    with pytest.MonkeyPatch.context() as mp:
        for k, v in ENV_ALL_MAIN_KERNELS.items():
            mp.setenv(k, v)
        mp.setenv("BJJ_TABLE_UNCACHED", "1" if uncached else "0")
        mp.delenv("BJJ_K1_VARIANT", raising=False)
        return bjj.Context(0, W)


@pytest.fixture(scope="module")
def plain_ctx():
    ctx = _context(False)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def uncached_ctx():
    ctx = _context(True)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def sizes(plain_ctx):
    """the n set: SHORT, and one more item than K1 holds resident lanes (512 per CU in either shape), so that lane 0 runs two rounds"""
    return SHORT + (plain_ctx.info().compute_units * 512 + 1,)


@pytest.fixture(scope="module")
def fixed_base_case(oracle, sizes):
    from babyjubjub_rs_amd import workload as w
    L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
    n = max(sizes)
    sc = w.random_u256(w.SEED_SCALARS, n, offset=77)
    for k, v in enumerate([0, 1, 2, L - 1, L, L + 1, 8 * L, (1 << 256) - 1]):   # inside every n >= 63
        sc[40 + k] = np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)
    want = oracle.mul_fixed_base(sc)
    want.setflags(write=False)
    want_c = oracle.compress(want)
    want_c.setflags(write=False)
    return sc, want, want_c


@pytest.fixture(scope="module")
def signature_case(oracle, sizes):
    """keys / messages, the oracle's signatures of them, and the verify inputs made of those with 1 item in 8 corrupted"""
    from babyjubjub_rs_amd import workload as w
    n = max(sizes)
    keys = w.random_u256(w.SEED_KEYS, n, offset=13)
    msgs = w.random_u256(w.SEED_MSGS, n, offset=13, top_bits_cleared=3)
    r, s, ok = oracle.sign(keys, msgs)
    assert ok.all()
    pk = oracle.public_keys(keys)
    v_pk, v_r, v_s, v_m = pk.copy(), r.copy(), s.copy(), msgs.copy()
    bad = np.arange(n) % 8 == 5
    idx = np.nonzero(bad)[0]
    for t, (arr, col) in enumerate(((v_s, 3), (v_m, 9), (v_r, 32 + 17), (v_pk, 6))):   # S, msg, R.y, A.x in turn
        rows = idx[(idx // 8) % 4 == t]
        arr[rows, col] ^= np.uint8(1 << (t + 1))
    want_ok = oracle.verify(v_pk, v_r, v_s, v_m)
    assert (want_ok[~bad] == 1).all() and (want_ok[bad] == 0).all()
    for a in (r, s, want_ok):
        a.setflags(write=False)
    return {"keys": keys, "msgs": msgs, "r": r, "s": s, "verify_in": (v_pk, v_r, v_s, v_m), "verify_ok": want_ok}


def _mismatch(got, want):
    return np.nonzero((got != want).reshape(len(want), -1).any(axis=1))[0][:8]


def _fixed_base_both_shapes(ctx, sc, want, want_c, n):
    """n items through bjj_mul_fixed_base{,_compressed}_dev: launches that run alone (one stream, synchronised) -> 512 lanes per
    workgroup; launches alternating over two streams with no synchronisation -> two workgroups of 256 lanes per CU"""
    import torch
    dev = torch.device("cuda", 0)
    d_sc = torch.from_numpy(np.ascontiguousarray(sc[:n]).reshape(-1)).to(dev)
    st = [torch.cuda.Stream(device=dev) for _ in range(2)]
    for width, exp, call in ((64, want, ctx.mul_fixed_base_dev), (32, want_c, ctx.mul_fixed_base_compressed_dev)):
        d_out = [torch.full((n * width,), 0xCD, dtype=torch.uint8, device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        for _ in range(2):
            call(d_sc.data_ptr(), n, d_out[0].data_ptr(), st[0].cuda_stream)
            ctx.sync()
        assert ctx.info().last_fixed_base_shape == 0
        got = d_out[0].cpu().numpy().reshape(n, width)
        assert (got == exp[:n]).all(), ("512 lanes", width, n, _mismatch(got, exp[:n]))
        d_out[0].fill_(0xCD)
        torch.cuda.synchronize()
        for k in range(4):
            call(d_sc.data_ptr(), n, d_out[k % 2].data_ptr(), st[k % 2].cuda_stream)
        assert ctx.info().last_fixed_base_shape == 1
        ctx.sync()
        for o in d_out:
            got = o.cpu().numpy().reshape(n, width)
            assert (got == exp[:n]).all(), ("2 x 256 lanes", width, n, _mismatch(got, exp[:n]))


@pytest.mark.parametrize("k", range(len(SHORT) + 1), ids=[str(n) for n in SHORT] + ["resident_lanes_plus_1"])
def test_fixed_base_parity_both_shapes(plain_ctx, fixed_base_case, sizes, k):
    _fixed_base_both_shapes(plain_ctx, *fixed_base_case, sizes[k])


@pytest.mark.parametrize("k", range(len(SHORT) + 1), ids=[str(n) for n in SHORT] + ["resident_lanes_plus_1"])
def test_verify_parity(plain_ctx, signature_case, sizes, k):
    n = sizes[k]
    got = plain_ctx.eddsa_verify(*(a[:n] for a in signature_case["verify_in"]))
    assert plain_ctx.info().last_verify_dispatch in (0, 1)   # not the short-call kernel
    want = signature_case["verify_ok"][:n]
    assert (got == want).all(), (n, np.nonzero(got != want)[0][:8])


@pytest.mark.parametrize("k", range(len(SHORT) + 1), ids=[str(n) for n in SHORT] + ["resident_lanes_plus_1"])
def test_sign_parity(plain_ctx, signature_case, sizes, k):
    n = sizes[k]
    r, s, ok = plain_ctx.sign(signature_case["keys"][:n], signature_case["msgs"][:n])
    assert plain_ctx.info().last_sign_form == 0              # one signature per lane: the kernel that gathers
    assert ok.all()
    assert (r == signature_case["r"][:n]).all(), (n, _mismatch(r, signature_case["r"][:n]))
    assert (s == signature_case["s"][:n]).all(), (n, _mismatch(s, signature_case["s"][:n]))


def test_uncached_table_is_sound_and_reported(uncached_ctx, plain_ctx):
    from babyjubjub_rs_amd import _lib
    iu, ip = uncached_ctx.info(), plain_ctx.info()
    assert iu.table_alloc == _lib.BJJ_TABLE_ALLOC_UNCACHED and ip.table_alloc == _lib.BJJ_TABLE_ALLOC_PLAIN
    assert iu.window_bits == ip.window_bits == W and iu.table_bytes == ip.table_bytes == 16 * ((1 << 15) + 1) * 128
    assert uncached_ctx.check_table() == 0 and plain_ctx.check_table() == 0
    print("bjj_init at W = %d: uncached %.1f ms, plain %.1f ms" % (W, iu.init_ms, ip.init_ms))


@pytest.mark.parametrize("k", range(len(SHORT) + 1), ids=[str(n) for n in SHORT] + ["resident_lanes_plus_1"])
def test_fixed_base_parity_on_uncached_table(uncached_ctx, fixed_base_case, sizes, k):
    _fixed_base_both_shapes(uncached_ctx, *fixed_base_case, sizes[k])


def test_uncached_and_plain_contexts_give_identical_bytes(uncached_ctx, plain_ctx, fixed_base_case, sizes):
    """two contexts of one process, one table of each memory type: the same bytes (the host-pointer entry point; short calls
    switched off, so both run K1)"""
    sc, want, want_c = fixed_base_case
    for n in sizes:
        a, b = uncached_ctx.mul_fixed_base(sc[:n]), plain_ctx.mul_fixed_base(sc[:n])
        assert uncached_ctx.info().last_fixed_base_shape in (0, 1) and plain_ctx.info().last_fixed_base_shape in (0, 1)
        assert a.tobytes() == b.tobytes() and (a == want[:n]).all(), n
        a, b = uncached_ctx.mul_fixed_base_compressed(sc[:n]), plain_ctx.mul_fixed_base_compressed(sc[:n])
        assert a.tobytes() == b.tobytes() and (a == want_c[:n]).all(), n
