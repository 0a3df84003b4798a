"""The memory contract of every entry point of include/bjj_hip.h: WHERE the bytes go.

Every array of a call -- inputs included -- lives inside one guarded arena (tests/memguard.py): 64 KiB of position-dependent
pattern in front of and behind it, at a chosen address modulo 256 (the header promises that 16-byte alignment is enough for
device pointers and sets no rule for host pointers).  Per call: return code 0 and the expected bytes; every guard byte unchanged;
every input byte unchanged; for n = 0 the output regions unchanged as well (bjj_msm: the identity and status -1, nothing else).
Every (row, form, n, offsets) runs twice with the output regions preset to two different patterns: K1, the signer and the key
entries stash phase-1 values in the item's own output slot, so a kernel that read a slot before writing it, or a neighbour's
slot, would give bytes that depend on the preset.

One table (ROWS) drives the device-pointer entries, their host-pointer twins and the bjj_*_multi host forms; a CPU-side gate
(test_every_entry_point_with_a_pointer_has_a_row) fails when the header gains a function with a pointer parameter that has
neither a row nor a line in EXCLUDED.

Expected bytes: once per row, ONE plain call of the same device-pointer entry on fresh torch allocations over the row's whole
input set, held against the C oracle at every item below 4 096, every edge item and a stride through the rest; a batch of n items
is the first n items with its LAST item replaced by an edge item.  bjj_sign_schnorr has no single oracle function: R is the
oracle's mul_scalar(B8, nonce), s the integer nonce + scalar_key * h from the oracle's scalar_key, public key and Poseidon.

Kernel forms are reached with the knobs the suite already uses, read at bjj_init (thresholds lowered to T = 4096 instead of
running 2^15-item batches around the real ones) and asserted from bjj_get_info.  Needs a real MI355X: `pytest -m gpu`."""
import ctypes
import os
import re
import time

import numpy as np
import pytest

from conftest import ROOT, ints, pack
from memguard import DeviceArena, HostArena

Q = 21888242871839275222246405745257275088548364400416034343698204186575808495617
L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
B8 = (5299619240641551281634865583518297030282874472190772894086521144482721001553,
      16950150798460657717958625567821834550301663161624707787222815936182638968203)

T = 4096                       # every short-call threshold of the test contexts (BJJ_*_MAX)
BIG = (1 << 16) + 37           # above 2^16, not a multiple of 64
UNIQUE = 8192                  # distinct items of a generated input set; the rest repeats them
SIZES = [0, 1, 2, 63, 64, 65, 255, 257, 511, 513, 2047, 2048, 2049, T - 1, T, T + 1, BIG]   # 2048: the EdDSA short-call kernels switch
SHORT_SIZES = [1, 65, 513, T + 1, BIG]
MIXED = (16, 48, 80, 112, 240)
HOST_SIZES = [1, 65, 201, 1541]                       # with chunks of 256, then 512 items: one ragged chunk, four chunks
HOST_OFFSETS = {"pageable": (0, 1, 8, 33, 100, 16, 250), "pinned": (16, 48, 0, 240, 112, 80, 32), "pinned_misaligned": (8, 1, 33, 100, 20, 250, 4)}

_SMALL = {"BJJ_FB_QUAD_MAX": T, "BJJ_VB_QUAD_MAX": T, "BJJ_VERIFY_SMALL_MAX": T, "BJJ_P5_COOP_MAX": T, "BJJ_SIGN_SMALL_MAX": T}
PROFILES = {       # environment of bjj_init (kernel knobs) and of the context's first host-pointer call (pipeline knobs)
    "small_behind": dict(_SMALL, BJJ_VB_SPLIT=0),
    "small_beside": dict(_SMALL, BJJ_VB_SPLIT=1),
    "v0_behind": {"BJJ_K1_VARIANT": 0, "BJJ_K2_VARIANT": 0, "BJJ_VERIFY_DISPATCH": 0, "BJJ_VB_SPLIT": 0, "BJJ_P5_COOP_MAX": 0, "BJJ_SIGN_SMALL_MAX": 0},
    "v0_beside": {"BJJ_K2_VARIANT": 0, "BJJ_VB_SPLIT": 1},
    "v1_beside": {"BJJ_K1_VARIANT": 1, "BJJ_K2_VARIANT": 1, "BJJ_VERIFY_DISPATCH": 1, "BJJ_VB_SPLIT": 1},
    "v1_behind": {"BJJ_K2_VARIANT": 1, "BJJ_VB_SPLIT": 0},
}
PIPE_KNOBS = {"BJJ_PIPE_FIRST_CHUNK": 256, "BJJ_PIPE_CHUNK": 512}


# ------------------------------------------------------------------------------------------------ the table
class Form:
    """one kernel form of a row: the context profile it runs under, the signer's constant-time switch, arguments behind n, and what
    bjj_get_info must say after a call of n items"""

    def __init__(self, label, profile, expect, ct=False, post=()):
        self.label, self.profile, self.expect, self.ct, self.post = label, profile, expect, ct, tuple(post)


class Row:
    def __init__(self, name, family, ins, outs, forms, pre=(), multi=None):
        self.name, self.family, self.ins, self.outs, self.forms, self.pre, self.multi = name, family, ins, outs, forms, tuple(pre), multi

    @property
    def dev(self):
        return "bjj_%s_dev" % self.name

    @property
    def host(self):
        return "bjj_%s" % self.name


def _fb(n):
    return {"last_fixed_base_shape": 2 if n <= T else 0}


def _vb(split, wide=False):
    return lambda n: {"last_var_base_form": 2 if n <= T and not wide else 1, "last_var_base_split": split}


FB_FORMS = [Form("quad_then_512", "small_behind", _fb), Form("one_workgroup_512", "v0_behind", lambda n: {"last_fixed_base_shape": 0}),
            Form("two_workgroups_256", "v1_beside", lambda n: {"last_fixed_base_shape": 1})]
PK_FORMS = FB_FORMS + [Form("constant_time", "v0_behind", lambda n: {"signer_constant_time": 1}, ct=True)]


def _vb_forms(wide):
    return [Form("quad_then_tiles_exact_behind", "small_behind", _vb(0, wide)), Form("quad_then_tiles_exact_beside", "small_beside", _vb(1, wide)),
            Form("grid_strided_exact_behind", "v0_behind", lambda n: {"last_var_base_form": 0, "last_var_base_split": 0}),
            Form("grid_strided_exact_beside", "v0_beside", lambda n: {"last_var_base_form": 0, "last_var_base_split": 1}),
            Form("tiles_exact_beside", "v1_beside", lambda n: {"last_var_base_form": 1, "last_var_base_split": 1}),
            Form("tiles_exact_behind", "v1_behind", lambda n: {"last_var_base_form": 1, "last_var_base_split": 0})]


VERIFY_FORMS = [Form("eight_lanes_then_groups", "small_behind", lambda n: {"last_verify_dispatch": 2 if n <= T else 1}),
                Form("persistent_waves", "v0_behind", lambda n: {"last_verify_dispatch": 0}),
                Form("groups", "v1_beside", lambda n: {"last_verify_dispatch": 1})]
P5_FORMS = [Form("six_lanes_then_one", "small_behind", lambda n: {"last_poseidon_form": 1 if n <= T else 0}),
            Form("one_hash_per_lane", "v0_behind", lambda n: {"last_poseidon_form": 0})]
SIGN_FORMS = [Form("eight_lanes_then_one", "small_behind", lambda n: {"last_sign_form": 1 if n <= T else 0}),
              Form("one_signature_per_lane", "v0_behind", lambda n: {"last_sign_form": 0, "signer_constant_time": 0}),
              Form("constant_time", "v0_behind", lambda n: {"last_sign_form": 0, "signer_constant_time": 1}, ct=True)]
SCHNORR_SIGN_FORMS = [Form("table_lookup", "v0_behind", lambda n: {"signer_constant_time": 0}),
                      Form("constant_time", "v0_behind", lambda n: {"signer_constant_time": 1}, ct=True)]
ONE_FORM = [Form("only_form", "small_behind", lambda n: {})]
MSM_FORMS = [Form("window_%d" % wb, "small_behind", lambda n: {}, post=(wb,)) for wb in (0, 4, 20)]

ROWS = [
    Row("mul_fixed_base", "fixed base", [32], [64], FB_FORMS, multi="bjj_mul_fixed_base_multi"),
    Row("mul_fixed_base_compressed", "fixed base", [32], [32], FB_FORMS),
    Row("public_keys", "fixed base", [32], [64], PK_FORMS),
    Row("public_keys_compressed", "fixed base", [32], [32], PK_FORMS),
    Row("mul_var_base", "variable base", [64, 32], [64], _vb_forms(False), multi="bjj_mul_var_base_multi"),
    Row("mul_var_base_wide", "variable base", [64, 64], [64], _vb_forms(True), pre=(64,)),
    Row("eddsa_verify", "verify", [64, 64, 32, 32], [1], VERIFY_FORMS, multi="bjj_eddsa_verify_multi"),
    Row("schnorr_verify", "verify", [64, 64, 32, 32], [1], VERIFY_FORMS),
    Row("eddsa_verify_compressed", "verify", [32, 64, 32], [1], VERIFY_FORMS),
    Row("poseidon5", "poseidon", [160], [32], P5_FORMS),
    Row("sign", "sign", [32, 32], [64, 32, 1], SIGN_FORMS),
    Row("sign_compressed", "sign", [32, 32], [64, 1], SIGN_FORMS),
    Row("sign_schnorr", "sign", [32, 32, 128], [64, 160, 1], SCHNORR_SIGN_FORMS),
    Row("compress_points", "one form", [64], [32], ONE_FORM),
    Row("decompress_points", "one form", [32], [64, 1], ONE_FORM),
    Row("scalar_keys", "one form", [32], [32], ONE_FORM),
    Row("point_add", "one form", [64, 64], [64], ONE_FORM),
    Row("proj_add", "one form", [96, 96], [96], ONE_FORM),
    Row("proj_affine", "one form", [96], [64], ONE_FORM),
    Row("msm", "msm", [64, 32], [64, 8], MSM_FORMS),
]
BY_NAME = {r.name: r for r in ROWS}

EXCLUDED = {   # exported functions with a pointer parameter that have no row, and why
    "bjj_init": "out_ctx is a handle the caller owns on its stack; no batch memory",
    "bjj_free": "takes the opaque context only",
    "bjj_sync": "takes the opaque context only",
    "bjj_stream": "takes the opaque context only",
    "bjj_reserve": "takes the opaque context only",
    "bjj_get_info": "fills a caller struct bounded by struct_size (tests/test_gpu_parity.py)",
    "bjj_check_table": "one uint64 on the caller's stack; reads the library's own table",
    "bjj_set_signer_constant_time": "takes the opaque context only (driven here as a form of the signer rows)",
    "bjj_host_alloc": "returns memory, moves no batch data",
    "bjj_host_free": "releases memory, moves no batch data",
    "bjj_host_register": "pins a caller range in place, moves no batch data",
    "bjj_host_unregister": "unpins a caller range, moves no batch data",
    "bjj_host_is_pinned": "a query, moves no batch data",
    "bjj_multi_init": "handle construction (tests/test_gpu_boundary.py)",
    "bjj_multi_free": "takes the opaque handle only",
    "bjj_multi_size": "takes the opaque handle only",
    "bjj_multi_ctx": "takes the opaque handle only",
    "bjj_multi_device": "takes the opaque handle only",
    "bjj_multi_set_transport": "takes the opaque handle only",
    "bjj_multi_set_chunks": "takes the opaque handle only",
    "bjj_shard_bounds": "host arithmetic into two size_t of the caller (tests/test_abi.py)",
    "bjj_multi_last_timing": "scalars on the caller's stack",
    "bjj_multi_last_overlap": "scalars on the caller's stack",
    "bjj_mul_fixed_base_multi_dev": "needs an RCCL communicator over several GPUs; launches the kernels of bjj_mul_fixed_base_dev",
    "bjj_mul_var_base_multi_dev": "needs an RCCL communicator over several GPUs; launches the kernels of bjj_mul_var_base_dev",
    "bjj_eddsa_verify_multi_dev": "needs an RCCL communicator over several GPUs; launches the kernels of bjj_eddsa_verify_dev",
}


def covered_functions():
    s = set()
    for r in ROWS:
        s |= {r.dev, r.host}
        if r.multi:
            s.add(r.multi)
    return s


# ------------------------------------------------------------------------------------------------ the CPU-side gate
def pointer_functions():
    """every function include/bjj_hip.h declares with a pointer among its parameters (comments stripped, as tests/test_abi.py)"""
    txt = open(os.path.join(ROOT, "include", "bjj_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted({m.group(1) for m in re.finditer(r"\b(bjj_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt) if "*" in m.group(2)})


def test_every_entry_point_with_a_pointer_has_a_row():
    have = pointer_functions()
    assert len(have) > 60 and "bjj_msm_dev" in have and "bjj_version" not in have
    cov = covered_functions()
    assert len(cov) == 2 * len(ROWS) + 3 and len(ROWS) == 20
    assert not cov & set(EXCLUDED), sorted(cov & set(EXCLUDED))
    missing = [f for f in have if f not in cov and f not in EXCLUDED]
    assert missing == [], "no row in ROWS and no reason in EXCLUDED: %s" % missing
    stale = [f for f in list(cov) + list(EXCLUDED) if f not in have]
    assert stale == [], "not (or no longer) a function with a pointer parameter in the header: %s" % stale
    assert all(isinstance(v, str) and v for v in EXCLUDED.values())


def test_the_arena_reports_where_a_stray_store_went():
    """the helper itself, on pageable host memory: layout, addresses modulo 256, and the wording of a failure"""
    data = np.arange(96, dtype=np.uint8)
    a = HostArena([("in", data, 33)], [("ok", 5, 8), ("out", 64, 250)], fill=0)
    b = HostArena([("in", data, 33)], [("ok", 5, 8), ("out", 64, 250)], fill=1)
    for name, off in (("in", 33), ("ok", 8), ("out", 250)):
        assert a.ptr(name) % 256 == off
    s_in, s_ok, s_out = a.slots
    assert s_in.start >= 65536 and s_ok.start - s_in.end >= 65536 and s_out.start - s_ok.end >= 65536 and a.total - s_out.end >= 65536
    g = np.asarray(a.buf[:s_in.start])
    assert len(np.unique(g)) > 200 and (np.asarray(a.buf[s_ok.start:s_ok.end]) != np.asarray(b.buf[s_ok.start:s_ok.end])).any()
    assert (np.asarray(a.buf[s_out.start:s_out.end]) != np.asarray(b.buf[s_out.start:s_out.end])).sum() > 48
    assert set(a.check()) == {"ok", "out"}
    a.buf[s_ok.end:s_ok.end + 3] ^= 0xFF                                   # a 32-bit store of a verdict at the last byte of `ok`
    with pytest.raises(AssertionError, match=r"3 guard bytes changed, 0 \.\. 2 bytes behind `ok`"):
        a.check()
    a.buf[s_ok.end:s_ok.end + 3] ^= 0xFF
    a.buf[s_in.start - 32:s_in.start] = 0
    with pytest.raises(AssertionError, match=r"1 \.\. 32 bytes in front of `in`"):
        a.check()
    a.buf[:] = a.image
    a.buf[s_in.start + 7] ^= 1
    with pytest.raises(AssertionError, match=r"1 bytes changed inside input `in` .*first at byte 7, last at byte 7"):
        a.check()
    a.buf[:] = a.image
    a.buf[s_out.start + 2] ^= 1
    a.check()
    with pytest.raises(AssertionError, match=r"inside untouchable output `out`"):
        a.check(outputs_unchanged=True)


# ------------------------------------------------------------------------------------------------ contexts
_CTX = {}


def _context(profile):
    """bjj.Context(0, 16) made under the profile's knobs; its first host-pointer call (which reads the pipeline knobs) is made here too"""
    import babyjubjub_rs_amd as bjj
    if profile in _CTX:
        return _CTX[profile]
    env = dict(PROFILES[profile], **PIPE_KNOBS)
    keep = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        c = bjj.Context(0, 16)
        c.mul_fixed_base(np.zeros((1, 32), np.uint8))
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    _CTX[profile] = c
    return c


@pytest.fixture(scope="module", autouse=True)
def _contexts_and_environment():
    before = {k: v for k, v in os.environ.items() if k.startswith("BJJ_")}
    t0 = time.time()
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()
    _MULTI.clear()
    _DATA.clear()
    assert {k: v for k, v in os.environ.items() if k.startswith("BJJ_")} == before          # no knob left set
    if COUNTS:
        print("\n[memory contract] %.1f s; calls per family (form x n x offsets x fill): %s"
              % (time.time() - t0, ", ".join("%s %d" % kv for kv in sorted(COUNTS.items()))))


COUNTS = {}
PATHS = set()          # (host entry, "direct" | "staged" | "zero_copy_out" | "zero_copy_in" | "chunks>=3") seen


# ------------------------------------------------------------------------------------------------ inputs and the oracle
def _tile(a, n):
    return np.ascontiguousarray(np.resize(a, (n,) + a.shape[1:]))


def _u256(seed, n, cols=1, clear=0):
    from babyjubjub_rs_amd import workload as w
    return w.random_u256(seed, n * cols, 0, top_bits_cleared=clear).reshape(n, 32 * cols).copy()


def _le(v, nbytes=32):
    return np.frombuffer(int(v).to_bytes(nbytes, "little"), np.uint8)


def _rows(vals, nbytes=32):
    return np.stack([_le(v, nbytes) for v in vals])


def _pt(x, y):
    return np.concatenate([_le(x), _le(y)])


def _off_curve(p):
    p = p.copy()
    p[0] ^= 1
    return p


SCALAR_EDGES = [0, L, 8 * L - 1, (1 << 256) - 1, 1, Q - 1, 8 * L, L - 1]


def _material(ctx, golden):
    """what several rows share: group points, keys, messages, valid EdDSA and Schnorr signatures (UNIQUE of each)"""
    if "material" in _DATA:
        return _DATA["material"]
    from babyjubjub_rs_amd import workload as w
    m = {}
    u = UNIQUE
    m["scalars"] = w.scalars_254(u, offset=31)
    m["scalars"][:, 31] |= (np.arange(u, dtype=np.uint8) & 3) << 6              # bits 254 / 255 on three quarters
    m["points"] = ctx.mul_fixed_base(w.scalars_254(u, offset=777)).copy()
    m["points2"] = ctx.mul_fixed_base(w.scalars_254(u, offset=99777)).copy()
    m["torsion"] = pack([ints(t) for t in golden["gpu_expected"]["torsion_points"]]).reshape(8, 64)
    m["keys"] = _u256(w.SEED_KEYS ^ 0x6D, u)
    m["msgs"] = _u256(w.SEED_MSGS ^ 0x6D, u, clear=3)
    m["nonces"] = _u256(w.SEED_NONCES ^ 0x6D, u, cols=4)
    A, R, S, msg = w.make_signatures(ctx.mul_fixed_base, ctx.poseidon5, u, offset=0x6D)
    A, R, S, msg = A.copy(), R.copy(), S.copy(), msg.copy()
    w.corrupt(A, R, S, msg, u)                                                  # 1 in 64 wrong, a part of them off the curve
    m["eddsa"] = (A, R, S, msg)
    x = w.to_ints(ctx.scalar_keys(m["keys"]))
    pk = ctx.public_keys(m["keys"]).copy()
    k = [v % (8 * L) for v in w.to_ints(_u256(w.SEED_NONCES ^ 0x77, u))]
    rp = ctx.mul_fixed_base(w.from_ints(k)).copy()
    h = w.to_ints(ctx.poseidon5(np.concatenate([pk, rp, m["msgs"]], axis=1)))
    sv = w.from_ints([(k[i] + x[i] * h[i]) % (8 * L) for i in range(u)])
    sv[::9, 1] ^= 4
    pk[11::257, 40] ^= 1
    rp[5::301, 2] ^= 1
    m["schnorr"] = (pk, rp, sv, m["msgs"].copy())
    _DATA["material"] = m
    return m


def _inputs(row, ctx, golden):
    """(base arrays of BIG items, edge arrays) of a row.  Edge items sit at fixed positions of the base and become the last item
    of every batch."""
    from babyjubjub_rs_amd import workload as w
    m = _material(ctx, golden)
    name = row.name
    tors, P, P2 = m["torsion"], m["points"], m["points2"]
    ident, off1, off2 = _pt(0, 1), _off_curve(P[3]), _off_curve(P2[9])
    off2[33] ^= 0x40
    sc_e = _rows(SCALAR_EDGES)
    if name in ("mul_fixed_base", "mul_fixed_base_compressed"):
        base, edge = [m["scalars"]], [sc_e]
    elif name in ("public_keys", "public_keys_compressed", "scalar_keys"):
        base, edge = [m["keys"]], [_rows([0, (1 << 256) - 1, 1, L])]
    elif name in ("mul_var_base", "msm"):
        pe = np.stack([ident, tors[3], off1, P[1], P[2], P[4], P[5], off2, tors[4], _pt(0, Q - 1)])
        se = _rows([5, 8 * L - 1, 12345, 0, L, 8 * L - 1, (1 << 256) - 1, (1 << 256) - 1, L, 3])
        base, edge = [P, m["scalars"]], [pe, se]
    elif name == "mul_var_base_wide":
        pe = np.stack([ident, tors[3], off1, P[1], P[2], P[4], P[5], off2])
        se = _rows([5, 8 * L - 1, (1 << 300) + 7, 0, L, 8 * L - 1, (1 << 512) - 1, (1 << 256) - 1], 64)
        base, edge = [P, np.concatenate([m["scalars"], _u256(0x77696465, UNIQUE)], axis=1)], [pe, se]
    elif name in ("eddsa_verify", "schnorr_verify"):
        A, R, S, msg = m["eddsa"] if name == "eddsa_verify" else m["schnorr"]
        good = [i for i in range(40) if i % 9 and i not in (11, 5)][:8]
        ea, er, es, em = A[good].copy(), R[good].copy(), S[good].copy(), msg[good].copy()
        em[0] = _le(Q)
        em[1] = _le(Q + 1)
        ea[2] = _off_curve(ea[2])
        er[3] = _off_curve(er[3])
        es[4] = _le((int.from_bytes(es[4].tobytes(), "little") % L) + L)       # s + l: the same verdict
        ea[5] = ident
        em[6] = _le((1 << 256) - 1)                                              # [7]: an untouched valid signature
        base, edge = [A, R, S, msg], [ea, er, es, em]
    elif name == "eddsa_verify_compressed":
        A, R, S, msg = m["eddsa"]
        pk32 = ctx.compress_points(A).copy()
        sig = np.concatenate([ctx.compress_points(R), S], axis=1)
        good = [i for i in range(1, 9)]
        ep, eg, em = pk32[good].copy(), sig[good].copy(), msg[good].copy()
        ep[0, 3] ^= 1                                                            # most such y do not decompress; the oracle says which
        eg[1, 5] ^= 1
        ep[2] = 0xFF                                                             # y >= r
        em[3] = _le(Q)
        em[4] = _le(Q + 1)
        eg[5, 40] ^= 1                                                           # s changed
        pk32[7::71, 3] ^= 1
        base, edge = [pk32, sig, msg], [ep, eg, em]
    elif name == "poseidon5":
        e = np.zeros((5, 160), np.uint8)
        e[1] = 0xFF
        e[2] = np.tile(_le(Q), 5)
        e[3] = np.tile(_le(Q - 1), 5)
        e[4] = np.concatenate([_le(v) for v in (1, Q + 1, 0, (1 << 255), L)])
        base, edge = [_u256(0x7035, UNIQUE, cols=5)], [e]
    elif name in ("sign", "sign_compressed", "sign_schnorr"):
        ke = np.stack([m["keys"][1], m["keys"][2], m["keys"][3], np.zeros(32, np.uint8), np.full(32, 0xFF, np.uint8), m["keys"][4]])
        me = _rows([Q, Q + 1, (1 << 256) - 1, 0, Q - 1, 7])
        msgs = m["msgs"].copy()
        msgs[13::97] = _le(Q + 5)                                                # Err items inside the batch
        base, edge = [m["keys"], msgs], [ke, me]
        if name == "sign_schnorr":
            base.append(m["nonces"])
            edge.append(_rows([0, (1 << 1024) - 1, L, 1, 1 << 1023, 8 * L - 1], 128))
    elif name == "compress_points":
        base, edge = [P], [np.stack([ident, off1, tors[3], _pt(Q - 1, Q - 1), _pt(0, 0), np.full(64, 0xFF, np.uint8)])]
    elif name == "decompress_points":
        comp = ctx.compress_points(P).copy()
        comp[7::71, 3] ^= 1
        e = np.stack([comp[1], comp[2], np.full(32, 0xFF, np.uint8), np.zeros(32, np.uint8), _le(1), _le(Q), comp[3]])
        e[0, 3] ^= 1
        e[1, 31] ^= 0x80                                                         # the other sign of x
        base, edge = [comp], [e]
    elif name == "point_add":
        neg = P[6].copy()
        neg[:32] = _le(Q - int.from_bytes(P[6, :32].tobytes(), "little"))
        base, edge = [P, P2], [np.stack([ident, P[5], P[6], tors[3], off1, tors[4]]), np.stack([ident, P[5], neg, tors[5], P2[1], off2])]
    elif name in ("proj_add", "proj_affine"):
        pr = _u256(0x70726F6A, UNIQUE, cols=3)
        pr[::3, :64] = P[::3]                                                     # a third: curve points under a random z ...
        pr[::6, 64:] = _le(1)                                                     # ... half of those with z = 1
        e = np.stack([np.concatenate([ident, _le(1)]), np.concatenate([P[1], _le(0)]), np.zeros(96, np.uint8), np.full(96, 0xFF, np.uint8),
                      np.concatenate([off1, _le(Q - 1)]), np.concatenate([tors[3], _le(2)])])
        base, edge = [pr], [e]
        if name == "proj_add":
            base.append(np.ascontiguousarray(pr[::-1]))
            edge.append(np.ascontiguousarray(e[::-1]))
    else:
        raise KeyError(name)
    base = [_tile(b, BIG) for b in base]
    ne = edge[0].shape[0]
    if name != "msm":
        pos = _edge_positions(ne)
        for b, e in zip(base, edge):
            assert b.shape[1:] == e.shape[1:] and e.shape[0] == ne and b.dtype == e.dtype == np.uint8
            b[pos] = e[np.arange(len(pos)) % ne]
    return base, edge


def _edge_positions(ne):
    return np.array([5 + 37 * k for k in range(ne)] + list(range(4500, BIG, 4099)))


def _loop(fn, out_w, *arrs):
    out = np.empty((arrs[0].shape[0], out_w), np.uint8)
    for i in range(arrs[0].shape[0]):
        fn(i, out[i])
    return out


def _oracle(row, orc, ins):
    """the C oracle's bytes for every item of `ins`: a list like row.outs"""
    name, p = row.name, orc._p
    ins = [np.ascontiguousarray(a) for a in ins]
    n = ins[0].shape[0]
    if name == "mul_fixed_base":
        return [orc.mul_fixed_base(ins[0])]
    if name == "mul_fixed_base_compressed":
        return [orc.compress(orc.mul_fixed_base(ins[0]))]
    if name == "public_keys":
        return [orc.public_keys(ins[0])]
    if name == "public_keys_compressed":
        return [orc.compress(orc.public_keys(ins[0]))]
    if name == "scalar_keys":
        return [_loop(lambda i, o: orc.lib.bjjref_scalar_key(p(ins[0][i]), p(o)), 32, ins[0])]
    if name == "mul_var_base":
        return [orc.mul_var_base(ins[0], ins[1])]
    if name == "mul_var_base_wide":
        return [_loop(lambda i, o: orc.lib.bjjref_mul_scalar(p(ins[0][i]), p(ins[1][i]), ctypes.c_size_t(64), p(o)), 64, ins[0])]
    if name == "eddsa_verify":
        return [orc.verify(*ins).reshape(n, 1)]
    if name == "schnorr_verify":
        return [orc.verify_schnorr(*ins).reshape(n, 1)]
    if name == "eddsa_verify_compressed":
        return [orc.verify_compressed(*ins).reshape(n, 1)]
    if name == "poseidon5":
        return [orc.poseidon5(ins[0])]
    if name in ("sign", "sign_compressed"):
        r, s, ok = orc.sign(ins[0], ins[1])
        r, s = r.copy(), s.copy()
        r[ok == 0] = 0
        s[ok == 0] = 0
        if name == "sign":
            return [r, s, ok.reshape(n, 1)]
        sig = np.concatenate([orc.compress(r), s], axis=1)
        sig[ok == 0] = 0
        return [sig, ok.reshape(n, 1)]
    if name == "sign_schnorr":
        b8 = np.tile(_pt(*B8), (n, 1))
        r = _loop(lambda i, o: orc.lib.bjjref_mul_scalar(p(b8[i]), p(ins[2][i]), ctypes.c_size_t(128), p(o)), 64, ins[0])
        x = _loop(lambda i, o: orc.lib.bjjref_scalar_key(p(ins[0][i]), p(o)), 32, ins[0])
        pk = orc.public_keys(ins[0])
        h = orc.poseidon5(np.concatenate([pk, r, ins[1]], axis=1))              # schnorr_hash: [pk.x, pk.y, r.x, r.y, msg]
        s = np.zeros((n, 160), np.uint8)
        ok = np.ones((n, 1), np.uint8)
        for i in range(n):
            if int.from_bytes(ins[1][i].tobytes(), "little") > Q:
                ok[i], r[i] = 0, 0
                continue
            v = int.from_bytes(ins[2][i].tobytes(), "little") + int.from_bytes(x[i].tobytes(), "little") * int.from_bytes(h[i].tobytes(), "little")
            s[i] = _le(v, 160)
        return [r, s, ok]
    if name == "compress_points":
        return [orc.compress(ins[0])]
    if name == "decompress_points":
        xy, ok = orc.decompress(ins[0])
        xy = xy.copy()
        xy[ok == 0] = 0
        return [xy, ok.reshape(n, 1)]
    if name == "point_add":
        return [orc.point_add(ins[0], ins[1])]
    if name == "proj_add":
        return [_loop(lambda i, o: orc.lib.bjjref_proj_add(p(ins[0][i]), p(ins[1][i]), p(o)), 96, ins[0])]
    if name == "proj_affine":
        return [_loop(lambda i, o: orc.lib.bjjref_proj_affine(p(ins[0][i]), p(o)), 64, ins[0])]
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ calls
def _call(ctx, fname, row, form, in_ptrs, n, out_ptrs, dev):
    args = [ctx.handle] + list(in_ptrs) + [ctypes.c_size_t(v) for v in row.pre] + [ctypes.c_size_t(n)] + list(form.post if form else ())
    outs = list(out_ptrs)
    if row.name == "msm" and not dev:
        outs[1] = ctypes.cast(outs[1], ctypes.POINTER(ctypes.c_int64))
    return getattr(ctx.lib, fname)(*(args + outs + ([None] if dev else [])))


def _plain_dev_call(ctx, row, form, ins, n):
    """the entry on fresh, allocator-aligned torch buffers"""
    import torch
    dev = torch.device("cuda", 0)
    d_in = [torch.from_numpy(np.ascontiguousarray(a[:n]).reshape(-1)).to(dev) if n else torch.zeros(16, dtype=torch.uint8, device=dev) for a in ins]
    d_out = [torch.zeros(max(n, 1) * w if row.name != "msm" else w, dtype=torch.uint8, device=dev) for w in row.outs]
    rc = _call(ctx, row.dev, row, form, [t.data_ptr() for t in d_in], n, [t.data_ptr() for t in d_out], True)
    assert rc == 0, (row.dev, n, ctx.lib.bjj_last_error())
    ctx.sync()
    if row.name == "msm":
        return [t.cpu().numpy() for t in d_out]
    return [t.cpu().numpy()[:n * w].reshape(n, w) for t, w in zip(d_out, row.outs)]


_DATA = {}


def _dataset(row, golden, orc):
    """(base inputs, edge inputs, expected of the base, expected of the edges) -- the expected bytes come from ONE plain device-pointer
    call per set and are held against the oracle here"""
    if row.name in _DATA:
        return _DATA[row.name]
    ctx = _context("small_behind")
    ctx.set_signer_constant_time(False)
    base, edge = _inputs(row, ctx, golden)
    ne = edge[0].shape[0]
    exp_base = _plain_dev_call(ctx, row, None, base, BIG)
    exp_edge = _plain_dev_call(ctx, row, None, edge, ne)
    idx = np.unique(np.concatenate([np.arange(4096), _edge_positions(ne), np.arange(4096, BIG, 997), [BIG - 1]]))
    for got, want in zip(exp_base, _oracle(row, orc, [b[idx] for b in base])):
        assert got[idx].shape == want.shape and (got[idx] == want).all(), (row.name, "base", idx[np.nonzero((got[idx] != want).any(axis=1))[0][:8]])
    for got, want in zip(exp_edge, _oracle(row, orc, edge)):
        assert got.shape == want.shape and (got == want).all(), (row.name, "edge", np.nonzero((got != want).any(axis=1))[0][:8])
    _DATA[row.name] = (base, edge, exp_base, exp_edge)
    return _DATA[row.name]


def _batch(data, n):
    """the first n items, the last one replaced by edge item n mod (number of edges); and what the entry must give for them"""
    base, edge, exp_base, exp_edge = data
    ins = [b[:n].copy() for b in base]
    exp = [e[:n].copy() for e in exp_base]
    if n:
        k = n % edge[0].shape[0]
        for a, e in zip(ins, edge):
            a[n - 1] = e[k]
        for a, e in zip(exp, exp_edge):
            a[n - 1] = e[k]
    return ins, exp


def _offsets(mode, count, n, choices=MIXED):
    if mode == "all_0":
        return [0] * count
    if mode == "all_16":
        return [16] * count
    return [choices[(k + n) % len(choices)] for k in range(count)]          # "mixed": different offsets for the arrays of one call


def _names(row):
    return ["in%d" % k for k in range(len(row.ins))], ["out%d" % k for k in range(len(row.outs))]


def _guarded_dev_call(ctx, row, form, ins, exp, n, mode):
    """both fills; returns nothing, asserts the five rules"""
    in_names, out_names = _names(row)
    cap = max(n, 64)                                               # an n = 0 call still gets regions it must not touch
    results = []
    for fill in (0, 1):
        offs = _offsets(mode, len(in_names) + len(out_names), n)
        a = DeviceArena([(nm, (arr if n else np.zeros((cap, w), np.uint8)), o) for nm, arr, w, o in zip(in_names, ins, row.ins, offs)],
                        [(nm, cap * w, o) for nm, w, o in zip(out_names, row.outs, offs[len(in_names):])], fill=fill)
        rc = _call(ctx, row.dev, row, form, [a.ptr(nm) for nm in in_names], n, [a.ptr(nm) for nm in out_names], True)
        assert rc == 0, (row.dev, form.label, n, mode, ctx.lib.bjj_last_error())
        ctx.sync()
        info = ctx.info()
        try:
            out = a.check(outputs_unchanged=(n == 0))
        except AssertionError as e:
            raise AssertionError("%s [%s] n = %d, offsets %s %s, fill %d: %s" % (row.dev, form.label, n, mode, offs, fill, e)) from None
        if n:
            for key, want in form.expect(n).items():
                assert getattr(info, key) == want, (row.dev, form.label, n, key, getattr(info, key), want)
            for nm, w, e in zip(out_names, row.outs, exp):
                got = out[nm][:n * w].reshape(n, w)
                assert (got == e).all(), (row.dev, form.label, n, mode, fill, nm, "items", np.nonzero((got != e).any(axis=1))[0][:8])
                assert (out[nm][n * w:] == a.image[a._slot(nm).start + n * w:a._slot(nm).end]).all(), (row.dev, n, nm, "beyond item n - 1")
            results.append([out[nm][:n * w] for nm, w in zip(out_names, row.outs)])
        COUNTS[row.family] = COUNTS.get(row.family, 0) + 1
    for x, y in zip(*results) if n else ():
        assert (x == y).all(), (row.dev, form.label, n, mode, "the result depends on what the output held before the call")


DEV_CASES = [pytest.param(r, f, id="%s-%s" % (r.dev, f.label)) for r in ROWS if r.name != "msm" for f in r.forms]


@pytest.mark.gpu
@pytest.mark.parametrize("row,form", DEV_CASES)
def test_device_pointer_entry(row, form, golden, oracle):
    data = _dataset(row, golden, oracle)
    ctx = _context(form.profile)
    ctx.set_signer_constant_time(form.ct)
    for mode, sizes in (("all_0", SIZES), ("all_16", SHORT_SIZES), ("mixed", SHORT_SIZES)):
        for n in sizes:
            ins, exp = _batch(data, n)
            _guarded_dev_call(ctx, row, form, ins, exp, n, mode)
    ctx.set_signer_constant_time(False)


# ---- bjj_msm: ONE result for the batch, so every n has its own expected bytes ----------------------------------------------------
def _tree_sum(add, pts):
    """pairwise tree of affine additions (an odd element waits for the next level), as tests/test_gpu_msm.py"""
    while len(pts) > 1:
        h = len(pts) // 2
        s = add(pts[0:2 * h:2], pts[1:2 * h:2])
        pts = np.concatenate([s, pts[2 * h:]]) if len(pts) % 2 else s
    return np.ascontiguousarray(pts[:1])


def _on_curve(p):
    x, y = int.from_bytes(p[:32].tobytes(), "little") % Q, int.from_bytes(p[32:].tobytes(), "little") % Q
    return (168700 * x * x + y * y - 1 - 168696 * x * x * y * y) % Q == 0


def _msm_data(ctx, golden, orc):
    """inputs of the bjj_msm row and the oracle's k_i * P_i for every item; off-curve points only among the edge items"""
    if "msm" not in _DATA:
        base, edge = _inputs(BY_NAME["msm"], ctx, golden)
        off_edge = [not _on_curve(p) for p in edge[0]]
        assert sum(off_edge) == 2 and all(_on_curve(p) for p in base[0][:64])
        _DATA["msm"] = (base, edge, orc.mul_var_base(base[0], base[1]), orc.mul_var_base(edge[0], edge[1]), off_edge, {})
    return _DATA["msm"]


def _msm_expected(orc, data, n):
    """oracle: the tree of point_add over mul_var_base; (0, 0) and the smallest index for a batch with an off-curve point"""
    base, edge, prod_base, prod_edge, off_edge, cache = data
    if n not in cache:
        k = n % edge[0].shape[0]
        if n == 0:
            cache[n] = (pack([(0, 1)]), -1)
        elif off_edge[k]:
            cache[n] = (np.zeros(64, np.uint8), n - 1)
        else:
            cache[n] = (_tree_sum(orc.point_add, np.concatenate([prod_base[:n - 1], prod_edge[k:k + 1]])).reshape(-1), -1)
    return cache[n]


@pytest.mark.gpu
@pytest.mark.parametrize("form", MSM_FORMS, ids=[f.label for f in MSM_FORMS])
def test_device_pointer_msm(form, golden, oracle):
    row = BY_NAME["msm"]
    ctx = _context(form.profile)
    data = _msm_data(ctx, golden, oracle)
    for mode, sizes in (("all_0", SIZES), ("all_16", SHORT_SIZES), ("mixed", SHORT_SIZES)):
        for n in sizes:
            ins, _ = _batch((data[0], data[1], [], []), n)
            want, status = _msm_expected(oracle, data, n)
            plain = _plain_dev_call(ctx, row, form, ins, n)
            assert (plain[0] == want).all() and int(plain[1].view(np.int64)[0]) == status, (form.label, n)
            exp = [want.reshape(1, 64), np.array([status], np.int64).view(np.uint8).reshape(1, 8)]
            results = []
            for fill in (0, 1):
                offs = _offsets(mode, 4, n)
                cap = max(n, 64)
                a = DeviceArena([("d_pts_xy", ins[0] if n else np.zeros(cap * 64, np.uint8), offs[0]),
                                 ("d_scalars", ins[1] if n else np.zeros(cap * 32, np.uint8), offs[1])],
                                [("d_out_xy", 64, offs[2]), ("d_first_off_curve", 8, offs[3])], fill=fill)
                rc = _call(ctx, row.dev, row, form, [a.ptr("d_pts_xy"), a.ptr("d_scalars")], n, [a.ptr("d_out_xy"), a.ptr("d_first_off_curve")], True)
                assert rc == 0, (form.label, n, ctx.lib.bjj_last_error())
                ctx.sync()
                try:
                    out = a.check()                                # n = 0 writes the identity and -1, and nothing else
                except AssertionError as e:
                    raise AssertionError("bjj_msm_dev [%s] n = %d, offsets %s %s, fill %d: %s" % (form.label, n, mode, offs, fill, e)) from None
                assert (out["d_out_xy"] == exp[0].reshape(-1)).all() and (out["d_first_off_curve"] == exp[1].reshape(-1)).all(), (form.label, n, mode, fill)
                results.append(out)
                COUNTS["msm"] = COUNTS.get("msm", 0) + 1
            assert all((results[0][k] == results[1][k]).all() for k in results[0])


# ------------------------------------------------------------------------------------------------ host pointers
_MULTI = {}


def _host_case(row, mem, golden, orc, multi=False):
    data = _dataset(row, golden, orc) if row.name != "msm" else None
    ctx = _context("small_behind")
    ctx.set_signer_constant_time(False)
    in_names, out_names = _names(row)
    fname = row.multi if multi else row.host
    if multi:
        import babyjubjub_rs_amd as bjj
        if "m" not in _MULTI:
            keep = {k: os.environ.get(k) for k in PIPE_KNOBS}
            os.environ.update({k: str(v) for k, v in PIPE_KNOBS.items()})
            try:
                _MULTI["m"] = bjj.MultiContext([0, 0], 16)         # two ranks on one GPU: the block arithmetic of G > 1
                _MULTI["m"].mul_fixed_base(np.zeros((3, 32), np.uint8))
            finally:
                for k, v in keep.items():
                    os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        handle = _MULTI["m"]
    else:
        handle = ctx
    for n in [0] + HOST_SIZES:
        if row.name == "msm":
            md = _msm_data(ctx, golden, orc)
            ins, _ = _batch((md[0], md[1], [], []), n)
            want, status = _msm_expected(orc, md, n)
            exp = [want.reshape(1, 64), np.array([status], np.int64).view(np.uint8).reshape(1, 8)]
        else:
            ins, exp = _batch(data, n)
        results = []
        for fill in (0, 1):
            choices = HOST_OFFSETS[mem]
            offs = [choices[(k + n + fill) % len(choices)] for k in range(len(in_names) + len(out_names))]
            if row.name == "msm":
                offs[3] = offs[3] & ~7                              # the int64 status word: naturally aligned, as the C type asks
            cap = max(n, 64)
            sizes = [64, 8] if row.name == "msm" else [cap * w for w in row.outs]
            a = HostArena([(nm, (arr if n else np.zeros((cap, w), np.uint8)), o) for nm, arr, w, o in zip(in_names, ins, row.ins, offs)],
                          [(nm, sz, o) for nm, sz, o in zip(out_names, sizes, offs[len(in_names):])], fill=fill,
                          pinned_ctx=None if mem == "pageable" else ctx)
            try:
                rc = _call(handle, fname, row, MSM_FORMS[0] if row.name == "msm" else None,
                           [a.ptr(nm) for nm in in_names], n, [a.ptr(nm) for nm in out_names], False)
                assert rc == 0, (fname, mem, n, handle.lib.bjj_last_error())
                try:
                    out = a.check(outputs_unchanged=(n == 0 and row.name != "msm"))
                except AssertionError as e:
                    raise AssertionError("%s (%s) n = %d, offsets %s, fill %d: %s" % (fname, mem, n, offs, fill, e)) from None
            finally:
                a.close()
            for nm, w, e in zip(out_names, row.outs, exp):
                m_ = 1 if row.name == "msm" else n
                got = out[nm][:m_ * w].reshape(m_, w)
                assert (got == e).all(), (fname, mem, n, fill, nm, "items", np.nonzero((got != e).any(axis=1))[0][:8])
                assert (out[nm][m_ * w:] == a.image[a._slot(nm).start + m_ * w:a._slot(nm).end]).all(), (fname, n, nm, "beyond item n - 1")
            results.append([out[nm][:(1 if row.name == "msm" else n) * w] for nm, w in zip(out_names, row.outs)])
            COUNTS["host"] = COUNTS.get("host", 0) + 1
            if n and not multi and row.name != "msm":              # which path ran (bjj_msm copies its arrays once, outside the pipeline)
                i = ctx.info()
                arrays = len(in_names) + len(out_names)
                if mem == "pageable":
                    assert (i.last_host_direct_arrays, i.last_host_staged_arrays, i.last_host_zero_copy) == (0, arrays, 0), (fname, n)
                    PATHS.add((fname, "staged"))
                else:
                    assert (i.last_host_direct_arrays, i.last_host_staged_arrays) == (arrays, 0), (fname, mem, n)
                    PATHS.add((fname, "direct"))
                    if mem == "pinned_misaligned":
                        assert i.last_host_zero_copy == 0, (fname, n, offs)          # the kernels move 16-byte words: copies realign
                    if i.last_host_zero_copy & 1:
                        PATHS.add((fname, "zero_copy_out"))
                    if i.last_host_zero_copy & 2:
                        PATHS.add((fname, "zero_copy_in"))
                assert i.last_host_chunks == {1: 1, 65: 1, 201: 1, 1541: 4}[n], (fname, mem, n, i.last_host_chunks)
                if i.last_host_chunks >= 3:
                    PATHS.add((fname, "chunks>=3"))
        assert all((x == y).all() for x, y in zip(*results)), (fname, mem, n, "the result depends on what the output held before the call")
    if not multi and row.name != "msm":                            # direct, staged and zero-copy are each KNOWN to have run
        assert (fname, "chunks>=3") in PATHS and (fname, "staged" if mem == "pageable" else "direct") in PATHS
        if mem == "pinned" and row.family == "fixed base":         # short calls on pinned, 16-byte aligned arrays: no copies at all
            assert (fname, "zero_copy_in") in PATHS and (fname, "zero_copy_out") in PATHS, fname


HOST_CASES = [pytest.param(r, mem, id="%s-%s" % (r.host, mem)) for r in ROWS for mem in ("pageable", "pinned", "pinned_misaligned")]


@pytest.mark.gpu
@pytest.mark.parametrize("row,mem", HOST_CASES)
def test_host_pointer_entry(row, mem, golden, oracle):
    _host_case(row, mem, golden, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("row,mem", [pytest.param(r, mem, id="%s-%s" % (r.multi, mem)) for r in ROWS if r.multi for mem in ("pageable", "pinned")])
def test_host_pointer_multi_entry_on_one_device(row, mem, golden, oracle):
    _host_case(row, mem, golden, oracle, multi=True)
