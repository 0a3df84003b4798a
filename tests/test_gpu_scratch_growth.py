"""Every grow-only block of a context (bjj_hip.hip: Block) grows twice in ONE context and is then used by a smaller call: entry
points are called at n = 1, 65, 4 097 and then 64 items, and every result of every call is compared with the C oracle (the MSM forms
also with each other).  A block that is freed under a launch, sized by the wrong formula or left dangling by a growth shows up as a
wrong result or a fault at these sizes.  The single-launch host forms, which share the bases_io block (and three of them the msm
block), are interleaved in one context at 5, 1, 260, 4 and 3 items.  A last case opens and closes contexts in a row: the blocks release in their destructors,
so a double free or a leak of a per-context block surfaces there.  Needs a real MI355X: run with `pytest -m gpu`."""
import ctypes

import numpy as np
import pytest

from test_gpu_msm import IDENTITY, oracle_msm, raw_msm

pytestmark = pytest.mark.gpu

SIZES = (1, 65, 4097, 64)        # increasing, then smaller: the blocks keep the size of the largest call
PIPE_SIZES = (200, 1000, 300)    # host pipeline with 64 / 128-item chunks: the exact-list split applies from 96 items
N, NP = max(SIZES), max(PIPE_SIZES)


def _undecompressible(oracle, comp):
    """per record: the first single-bit flip after which Point::decompress fails"""
    out = comp.copy()
    for i in range(len(out)):
        for bit in range(64):
            c = comp[i:i + 1].copy()
            c[0, bit >> 3] ^= 1 << (bit & 7)
            if oracle.decompress(c)[1][0] == 0:
                out[i] = c[0]
                break
        else:
            raise AssertionError("no undecompressible neighbour of record %d" % i)
    return out


@pytest.fixture(scope="module")
def data(oracle):
    """inputs and oracle results for the largest size, computed once; a call on n items uses the first n (every entry point here
    works item by item, so a prefix of the results is the result of the prefix)"""
    from babyjubjub_rs_amd import workload as w
    d = {}
    rng = np.random.default_rng(0x67726f77)
    d["sc"] = w.scalars_254(N, offset=0x5c)
    d["keys"] = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    d["pts"] = oracle.mul_fixed_base(w.scalars_254(N, offset=0x9d))
    d["fb32"] = oracle.compress(oracle.mul_fixed_base(d["sc"]))
    d["pk"] = oracle.public_keys(d["keys"])
    d["pk32"] = oracle.compress(d["pk"])
    d["vb"] = oracle.mul_var_base(d["pts"], d["sc"])
    A, R, S, msg = w.make_signatures(oracle.mul_fixed_base, oracle.poseidon5, N)
    # wire format first, then 1 in 64 corrupted (a corrupted point does not compress to anything meaningful): corrupt() flips a bit in
    # the first 32 bytes of A's record and in the second 32 bytes of R's
    z = np.zeros((N, 32), np.uint8)
    A_w, R_w = np.concatenate([oracle.compress(A), z], axis=1), np.concatenate([z, oracle.compress(R)], axis=1)
    bad = w.corrupt(A_w, R_w, S, msg, N)
    d["A32"], d["sig"], d["msg"] = np.ascontiguousarray(A_w[:, :32]), np.concatenate([R_w[:, 32:], S], axis=1), msg
    d["verdict"] = oracle.verify_compressed(d["A32"], d["sig"], d["msg"])
    assert (d["verdict"][~bad] == 1).all() and (d["verdict"][bad] != 1).all() and bad.any()
    # host pipeline: every 50th point off the curve / every 50th public key undecompressible
    d["pts_off"] = d["pts"][:NP].copy()
    d["pts_off"][::50, 7] ^= 4
    d["vb_off"] = d["vb"][:NP].copy()
    d["vb_off"][::50] = oracle.mul_var_base(d["pts_off"][::50], d["sc"][:NP][::50])
    d["A32_bad"] = d["A32"][:NP].copy()
    d["A32_bad"][::50] = _undecompressible(oracle, d["A32"][:NP][::50])
    d["verdict_bad"] = oracle.verify_compressed(d["A32_bad"], d["sig"][:NP], d["msg"][:NP])
    assert (d["verdict_bad"][::50] == 2).all()
    return d


def _flat(a):
    return np.ascontiguousarray(a, np.uint8).reshape(-1)


def test_device_pointer_forms_grow_twice_then_shrink(oracle, data):
    """xy (compressed K1 outputs), codec (scalar keys, decompressed signatures), scratch and slow (K2 + K6)"""
    import torch
    import babyjubjub_rs_amd as bjj
    dev = torch.device("cuda", 0)
    ctx = bjj.Context(0, 16)

    def up(a):
        return torch.from_numpy(_flat(a).copy()).to(dev)

    def run(fn, ins, n, row):
        d_in = [up(a) for a in ins]
        d_out = torch.full((n * row,), 0xAB, dtype=torch.uint8, device=dev)
        fn(*[t.data_ptr() for t in d_in], n, d_out.data_ptr())
        ctx.sync()
        return d_out.cpu().numpy().reshape(n, row) if row > 1 else d_out.cpu().numpy()

    try:
        for n in SIZES:
            assert (run(ctx.mul_fixed_base_compressed_dev, [data["sc"][:n]], n, 32) == data["fb32"][:n]).all(), n
            assert (run(ctx.public_keys_dev, [data["keys"][:n]], n, 64) == data["pk"][:n]).all(), n
            assert (run(ctx.public_keys_compressed_dev, [data["keys"][:n]], n, 32) == data["pk32"][:n]).all(), n
            got = run(ctx.eddsa_verify_compressed_dev, [data["A32"][:n], data["sig"][:n], data["msg"][:n]], n, 1)
            assert (got == data["verdict"][:n]).all(), n
            pts, want, j = data["pts"][:n].copy(), data["vb"][:n].copy(), n // 2      # one off-curve point per call
            pts[j, 7] ^= 4
            want[j] = oracle.mul_var_base(pts[j:j + 1], data["sc"][j:j + 1])[0]
            assert (want[j] != data["vb"][j]).any()
            assert (run(ctx.mul_var_base_dev, [pts, data["sc"][:n]], n, 64) == want).all(), n
    finally:
        ctx.close()


def test_msm_block_grows_with_and_without_the_input_copies(oracle, data):
    """bjj_msm_dev (the scratch alone), bjj_msm and bjj_msm_batch on host pointers (scratch + the inputs behind it)"""
    import torch
    import babyjubjub_rs_amd as bjj
    dev = torch.device("cuda", 0)
    ctx = bjj.Context(0, 16)
    try:
        for n in SIZES:
            pts, sc = data["pts"][:n], data["sc"][:n]
            want = oracle_msm(oracle, pts, sc)
            d_p, d_s = torch.from_numpy(_flat(pts).copy()).to(dev), torch.from_numpy(_flat(sc).copy()).to(dev)
            d_out, d_st = torch.zeros(64, dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
            ctx.msm_dev(d_p.data_ptr(), d_s.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr())
            ctx.sync()
            assert int(d_st[0]) == -1 and (d_out.cpu().numpy().reshape(1, 64) == want).all(), n
            got, st = raw_msm(ctx, pts, sc)
            assert st == -1 and (got == want).all(), n
            cut = n // 3                                                   # two segments (the first one empty for n = 1)
            out, status = ctx.msm_batch(pts, sc, [0, cut, n])
            assert (status == -1).all(), n
            assert (out[0:1] == (oracle_msm(oracle, pts[:cut], sc[:cut]) if cut else IDENTITY)).all(), n
            assert (out[1:2] == oracle_msm(oracle, pts[cut:], sc[cut:])).all(), n
    finally:
        ctx.close()


def test_host_pipeline_blocks_grow_then_shrink(oracle, data, monkeypatch):
    """pipe_wl, dstage, patch_host and the pinned rings: with chunks of 64 / 128 items the calls below take the split form (bulk
    launches per chunk beside ONE exact launch over the batch-wide list), several chunks each"""
    import babyjubjub_rs_amd as bjj
    monkeypatch.setenv("BJJ_PIPE_FIRST_CHUNK", "64")      # read when the context runs its first host-pointer call
    monkeypatch.setenv("BJJ_PIPE_CHUNK", "128")
    ctx = bjj.Context(0, 16)
    lib, hnd = ctx.lib, ctx.handle
    try:
        # pageable inputs and outputs: rings, device staging, the list, and K6's results patched in on the host
        for n in PIPE_SIZES:
            got = ctx.mul_var_base(data["pts_off"][:n], data["sc"][:n])
            i = ctx.info()
            assert (i.last_host_direct_arrays, i.last_host_staged_arrays) == (0, 3) and i.last_host_chunks >= 2, n
            assert (got == data["vb_off"][:n]).all(), n
        # the same calls on pinned arrays
        for n in PIPE_SIZES:
            bufs = [ctx.host_empty(n * 64), ctx.host_empty(n * 32), ctx.host_empty(n * 64)]
            bufs[0][:], bufs[1][:], bufs[2][:] = _flat(data["pts_off"][:n]), _flat(data["sc"][:n]), 0xAB
            ctx._ck(lib.bjj_mul_var_base(hnd, bufs[0].ctypes.data, bufs[1].ctypes.data, ctypes.c_size_t(n), bufs[2].ctypes.data), "bjj_mul_var_base")
            i = ctx.info()
            assert (i.last_host_direct_arrays, i.last_host_staged_arrays) == (3, 0), n
            assert (np.asarray(bufs[2]).reshape(n, 64) == data["vb_off"][:n]).all(), n
            for b in bufs:
                ctx.host_free(b)
        # the wire-format verifier: 162 bytes per item of decompressed records in the device staging, verdicts leave at the end
        for n in PIPE_SIZES:
            got = ctx.eddsa_verify_compressed(data["A32_bad"][:n], data["sig"][:n], data["msg"][:n])
            assert ctx.info().last_host_chunks >= 2, n
            assert (got == data["verdict_bad"][:n]).all(), n
    finally:
        ctx.close()


STAGED_SIZES = (5, 1, 260, 4, 3)   # 5 * 64 and 3 * 32 are no multiples of 256, 4 * 64 is one; 260 grows the block, 4 and 3 reuse it
NS = max(STAGED_SIZES)
SEGMENTS = (0, 4, 1)               # m = 3, n = 5: the CSR forms, one segment empty


@pytest.fixture(scope="module")
def staged(oracle, golden):
    """inputs and expected values of the single-launch host forms for NS items, by the C oracle with the helpers of the per-feature
    tests (bases_cases, signer_cases, signer_set_cases, dlog_cases, test_gpu_msm); every entry works item by item, so a call on n
    items uses the first n.  Computed once, never written."""
    import dlog_cases as dc
    import signer_cases as sc
    import signer_set_cases as ssc
    from babyjubjub_rs_amd import api
    from bases_cases import scalar_array
    from conftest import ints, pack, unpack
    from test_gpu_bases import fold, rep
    rng = np.random.default_rng(0x57A6ED)
    d = {}
    # bjj_mul_bases: two caller-chosen bases and the NULL base (B8)
    d["S"] = [scalar_array(NS, (16,), 0x57A6 + j) for j in range(3)]
    d["P"] = oracle.mul_fixed_base(pack([sc.KEY_SCALAR + 77, sc.KEY_SCALAR + 7919]))
    prod = [oracle.mul_var_base(rep(d["P"][0], NS), d["S"][0]), oracle.mul_fixed_base(d["S"][1]), oracle.mul_var_base(rep(d["P"][1], NS), d["S"][2])]
    d["bases1"], d["bases3"] = prod[0], fold(oracle.point_add, prod)
    # one signer (EdDSA), and a set of three keys (Schnorr): 1 item in 8 corrupted, the directed items of keys 0 and 1 last
    d["A"] = sc.key_point(oracle, sc.KEY_SCALAR)
    d["signer"] = sc.bulk(oracle, d["A"], sc.KEY_SCALAR, NS, 0x51A6, False, False)
    d["signer_want"] = oracle.verify(rep(pack([d["A"]]), NS), *d["signer"])
    assert 0 < int((d["signer_want"] == 1).sum()) < NS
    d["keys"] = ssc.key_list(oracle, golden, 3)
    d["set"] = ssc.dataset(oracle, d["keys"], NS, True, 0x5E7A)
    # logarithms below and beyond 2^8, an off-curve record at [2]
    ms = [0, 255, 1, 256, 7] + [int(v) for v in rng.integers(0, 288, NS - 5)]
    pts = oracle.mul_fixed_base(pack(ms)).copy()
    pts[2, 32] ^= 1
    cases = [(None, dc.OFF_CURVE if i == 2 else m) for i, m in enumerate(ms)]
    d["dlog_pts"], d["dlog_want"] = pts, dc.expected(cases, 8)
    # one scalar times many points (subgroup points, [1] shifted by a point of order 8, [2] off the curve), with and without an addend
    tors = pack([ints(t) for t in golden["gpu_expected"]["torsion_points"]]).reshape(8, 64)
    cp = oracle.mul_fixed_base(pack([int.from_bytes(rng.bytes(31), "little") for _ in range(NS)])).copy()
    cp[1] = oracle.point_add(cp[1:2], tors[1:2])[0]
    cp[2, 0] ^= 1
    ca = oracle.mul_fixed_base(pack([int.from_bytes(rng.bytes(31), "little") for _ in range(NS)]))
    d["k"] = sc.KEY_SCALAR
    kp = oracle.mul_var_base(cp, np.tile(pack([d["k"]]), NS)).copy()
    sub = oracle.point_add(ca, api._negate_x(kp)).copy()
    kp[2], sub[2] = 0, 0
    d["common"] = dict(pts=cp, add=ca, plain=kp, sub=sub, ok=np.where(np.arange(NS) == 2, 2, 1).astype(np.uint8),
                       subgroup=np.where(np.arange(NS) == 2, 2, np.where(np.arange(NS) == 1, 0, 1)).astype(np.uint8))
    # exponential ElGamal under sk: (C1, C2) = (r B8, m B8 + r PK), the plaintexts and the expectations of the logarithms above
    d["sk"] = sc.KEY_SCALAR + 4242
    pk = oracle.mul_fixed_base(pack([d["sk"]]))
    rs = pack([int.from_bytes(rng.bytes(31), "little") for _ in range(NS)])
    d["c1"] = oracle.mul_fixed_base(rs)
    d["c2"] = oracle.point_add(oracle.mul_fixed_base(pack(ms)), oracle.mul_var_base(rep(pk, NS), rs))
    d["dec_want"] = dc.expected([(None, m) for m in ms], 8)
    # the CSR forms on the first five points and scalars
    from test_gpu_msm import ORDER8, oracle_msm
    off = [0] + [int(v) for v in np.cumsum(SEGMENTS)]
    neg = np.array([0, 1, 0, 0, 1], np.uint8)
    unit = pack([ORDER8 - 1 if g else 1 for g in neg]).reshape(5, 32)
    seg = lambda s: np.concatenate([oracle_msm(oracle, ca[a:b], s[a:b]) for a, b in zip(off, off[1:])])
    d["off"], d["neg"] = off, neg
    d["msm_batch"], d["sum_plain"], d["sum_neg"] = seg(d["S"][0][:5]), seg(pack([1] * 5).reshape(5, 32)), seg(unit)
    for v in d.values():
        for a in (v if isinstance(v, (list, tuple)) else v.values() if isinstance(v, dict) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return d


def test_staged_host_forms_share_one_block(staged):
    """bases_io is the staging block of seven host forms and msm, behind a kernel layout, of three: in ONE context the forms are
    interleaved at 5, 1, 260, 4 and 3 items, so that every call finds the block as a different entry left it -- grown by another
    form, larger than it needs, with that form's bytes in it -- and bjj_point_sum / bjj_msm_batch run between them."""
    import babyjubjub_rs_amd as bjj
    d = staged
    c = lambda a, n: np.ascontiguousarray(a[:n])
    ctx = bjj.Context(0, 16)
    try:
        b1, b2 = ctx.base(d["P"][0:1]), ctx.base(d["P"][1:2], 8)
        signer, sset, table = ctx.base(d["A"], 8), ctx.signer_set(d["keys"][3]), ctx.dlog_table(None, 16)
        R, S, M = d["signer"]
        st, cm = d["set"], d["common"]
        for rnd, n in enumerate(STAGED_SIZES):
            assert (ctx.mul_bases([b1], [c(d["S"][0], n)]) == d["bases1"][:n]).all(), n
            ok = signer.verify(c(R, n), c(S, n), c(M, n))
            assert (ok == d["signer_want"][:n]).all(), n
            out, ok = ctx.mul_common(d["k"], c(cm["pts"], n), c(cm["add"], n), True)
            assert (ok == cm["ok"][:n]).all() and (out == cm["sub"][:n]).all(), n
            m, ok = table.dlog(c(d["dlog_pts"], n), 8)
            assert m.tolist() == d["dlog_want"][0][:n] and ok.tolist() == d["dlog_want"][1][:n], n
            out, status = ctx.point_sum(c(cm["add"], 5), d["off"], d["neg"] if rnd & 1 else None)
            assert (status == -1).all() and (out == d["sum_neg" if rnd & 1 else "sum_plain"]).all(), n
            got = ctx.mul_bases([b1, None, b2], [c(s, n) for s in d["S"]])
            assert (got == d["bases3"][:n]).all(), n
            assert (ctx.in_subgroup(c(cm["pts"], n)) == cm["subgroup"][:n]).all(), n
            ok = sset.verify_schnorr(c(st["idx"], n), c(st["R"], n), c(st["S"], n), c(st["msg"], n))
            assert (ok == st["want"][:n]).all(), n
            out, status = ctx.msm_batch(c(cm["add"], 5), c(d["S"][0], 5), d["off"])
            assert (status == -1).all() and (out == d["msm_batch"]).all(), n
            m, ok = ctx.decrypt(table, d["sk"], c(d["c1"], n), c(d["c2"], n), 8)
            assert m.tolist() == d["dec_want"][0][:n] and ok.tolist() == d["dec_want"][1][:n], n
            out, ok = ctx.mul_common(d["k"], c(cm["pts"], n))
            assert (ok == cm["ok"][:n]).all() and (out == cm["plain"][:n]).all(), n
    finally:
        ctx.close()


def test_twenty_contexts_in_a_row(data):
    """every per-context block is released by its destructor, once: 20 contexts, one 65-item call each"""
    import babyjubjub_rs_amd as bjj
    for k in range(20):
        ctx = bjj.Context(0, 16)
        try:
            assert (ctx.public_keys(data["keys"][:65]) == data["pk"][:65]).all(), k
        finally:
            ctx.close()
