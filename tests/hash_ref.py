"""Plain-integer model and input sets for the Poseidon permutation as the kernels hold it (csrc/poseidon.hpp: poseidon5_t with its
partial rounds one at a time and in pairs, poseidon_full_round; csrc/dleq.hpp: dleq_challenge in both forms; csrc/k_small.hip:
p5c_hash5, six lanes per hash).  Shared by tests/test_hash_ops_host.py (the g++ build of tests/devfuzz/hash_ops.hpp with the bound
assertions live) and tests/test_gpu_hash_ops.py (the same dispatcher and the six-lane kernel on the device, tests/devfuzz/hash.hip).
A plain helper module: no fixtures, no pytest hooks, nothing imported from oracle/; beside the model it holds only cpu_run, the
call into the CPU library that the test modules' fixture builds.

The model is the PLAIN permutation: state [0, in0 .. in4], 68 rounds of { add the round constants; x^5 on every element (the 4
first and 4 last rounds) or on element 0; state <- M . state }, on Python integers mod r.  Its constants are the plain lists
BJJ_K_POSEIDON_C / BJJ_K_POSEIDON_M of csrc/bjj_constants.inc taken out of Montgomery form -- lists no kernel reads: the kernels
run the sparse form (PCF, PKP, PSP, PCAB, PAL) -- and tests/test_constants.py holds them against the oracle's own generator.
tests/test_hash_ops_host.py asserts that they are poseidon_params(6) of oracle/bjj_oracle.py and that poseidon5 below is that
module's poseidon on every edge row, so on a machine without the Python oracle (the GPU tests never run it) the model is still the
oracle's function.  One Python hash costs about 2 ms: the model judges the edge sets, the threaded C oracle every random item.

An item is a tuple of Python integers: the VALUES of its field elements (five for the hashes, nine for the challenges: tag, C1,
D, A, B; six and then the round index for the full round).  The domain of every element is what poseidon5_t states and its
callers deliver: Montgomery form, N-form limbs, value in [0, 2r); records() writes the one N-form limb vector such a value has.
Every generator builds its items inside the domain by construction: nothing is rejected or left out."""
import ctypes
import os
import random

import numpy as np

from field_ref import M29, R1, R_MOD, RINV, TOP_R, dedup, mont, vals_of_limbs, vals_of_words
from test_constants import parse_inc

NL = 9
OPS = dict(p5_plain=0, p5_pairs=1, full_round=2, challenge_plain=3, challenge_pairs=4)
WIDTHS = dict(p5_plain=(45, 17), p5_pairs=(45, 17), full_round=(55, 54), challenge_plain=(81, 8), challenge_pairs=(81, 8))
NELEMS = dict(p5_plain=5, p5_pairs=5, full_round=6, challenge_plain=9, challenge_pairs=9)
TOP_2R = (2 * R_MOD) >> 232           # the largest admissible top limb is TOP_2R - 1 under all-ones limbs, TOP_2R under smaller ones
P5C_GROUP = 8                         # lanes per hash of the six-lane form

_INC = parse_inc()
PCF = _INC["BJJ_K_POSEIDON_CF"]       # csrc/curve.hpp: Consts::PCF, the constants of the 8 full rounds as the kernels add them (Montgomery)
C_PLAIN = [c * RINV % R_MOD for c in _INC["BJJ_K_POSEIDON_C"]]
M_PLAIN = [[m * RINV % R_MOD for m in _INC["BJJ_K_POSEIDON_M"][6 * i:6 * i + 6]] for i in range(6)]
assert len(PCF) == 48 and len(C_PLAIN) == 68 * 6 and all(0 < c < R_MOD for c in PCF)


# ---- the model -------------------------------------------------------------------------------------------------------------
def _mix(st):
    return [sum(m * s for m, s in zip(row, st)) % R_MOD for row in M_PLAIN]


def poseidon5(inputs):
    """the hash of five plain integers: 68 plain rounds, element 0 of the final state"""
    assert len(inputs) == 5
    st = [0] + [v % R_MOD for v in inputs]
    for r in range(68):
        st = [(s + c) % R_MOD for s, c in zip(st, C_PLAIN[6 * r:6 * r + 6])]
        if r < 4 or r >= 64:
            st = [pow(s, 5, R_MOD) for s in st]
        else:
            st[0] = pow(st[0], 5, R_MOD)
        st = _mix(st)
    return st[0]


def full_round(state, rnd):
    """round `rnd` (0 .. 7) of poseidon_full_round on six plain integers, with the constants the kernels add (PCF: those of the
    rounds 0-3 and 64-67, round 64's adjusted for the sparse form before it)"""
    assert len(state) == 6 and 0 <= rnd < 8
    return _mix([pow((s + c * RINV) % R_MOD, 5, R_MOD) for s, c in zip(state, PCF[6 * rnd:6 * rnd + 6])])


def plain(v):
    """the plain integer of a Montgomery value"""
    return v * RINV % R_MOD


def expected(op, items):
    """the model's results: the hash (the p5 ops), the challenge, or the six plain elements of the next state"""
    if op in ("p5_plain", "p5_pairs"):
        return [poseidon5([plain(v) for v in it]) for it in items]
    if op in ("challenge_plain", "challenge_pairs"):
        return [poseidon5([poseidon5([plain(v) for v in it[:5]])] + [plain(v) for v in it[5:]]) for it in items]
    if op == "full_round":
        return [full_round([plain(v) for v in it[:6]], it[6]) for it in items]
    raise ValueError(op)


def _le32(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8)


def expected_c(op, items, oracle):
    """the hashes and the challenges by the threaded C oracle (conftest.Oracle.poseidon5: 160 bytes of plain integers per hash)"""
    hash5 = lambda rows: vals_of_words(np.ascontiguousarray(oracle.poseidon5(_le32([v for row in rows for v in row]))).view("<u4"))  # noqa: E731
    if op in ("p5_plain", "p5_pairs"):
        return hash5([[plain(v) for v in it] for it in items])
    if op in ("challenge_plain", "challenge_pairs"):
        h0 = hash5([[plain(v) for v in it[:5]] for it in items])
        return hash5([[h] + [plain(v) for v in it[5:]] for h, it in zip(h0, items)])
    raise ValueError(op)


# ---- limbs -----------------------------------------------------------------------------------------------------------------
def limbs_of_vals(vals):
    """(n, 9) uint32: the N-form limbs of n values below 2^256, split in numpy"""
    w = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), "<u8").reshape(-1, 4)
    out = np.empty((w.shape[0], NL), np.uint32)
    for i in range(NL):
        lo, sh = divmod(29 * i, 64)
        x = w[:, lo] >> np.uint64(sh)
        if sh + 29 > 64 and lo + 1 < 4:
            x = x | (w[:, lo + 1] << np.uint64(64 - sh))
        out[:, i] = (x & np.uint64(M29) if i < NL - 1 else x).astype(np.uint32)
    return out


def records(op, items):
    """the uint32 input records of `items`"""
    k = NELEMS[op]
    a = limbs_of_vals([v for it in items for v in it[:k]]).reshape(len(items), k * NL)
    if op == "full_round":
        a = np.concatenate([a, np.array([[it[6]] for it in items], np.uint32)], axis=1)
    assert a.shape == (len(items), WIDTHS[op][0])
    return np.ascontiguousarray(a)


def items_of(op, recs):
    """the inverse of records"""
    k = NELEMS[op]
    recs = np.asarray(recs)
    v = vals_of_limbs(recs[:, :k * NL].reshape(-1, NL))
    rows = [tuple(v[i * k:(i + 1) * k]) for i in range(len(recs))]
    return [row + (int(r),) for row, r in zip(rows, recs[:, k * NL])] if op == "full_round" else rows


# ---- edge values of one element ------------------------------------------------------------------------------------------
ONES_TOPS = (0, TOP_R - 1, TOP_R, TOP_2R - 1)
ONES_LOW = (1 << 232) - 1             # limbs 0 .. 7 all ones


def edge_values():
    v = [0, 1, R_MOD - 1, R_MOD, R_MOD + 1, 2 * R_MOD - 2, 2 * R_MOD - 1]
    v += [R1, R1 + R_MOD, mont(R_MOD - 1), mont(R_MOD - 1) + R_MOD]
    v += [1 << (29 * i) for i in range(1, NL)]                               # (the single bit of limb 0 is the value 1 above)
    v += [ONES_LOW + (t << 232) for t in ONES_TOPS]
    assert all(0 <= x < 2 * R_MOD for x in v) and len(set(v)) == len(v)      # every edge the issue names is inside the domain: none dropped
    return v


def sbox_zero_reps(rnd, j):
    """the two representatives of the state element j that makes S-box input j of full round `rnd` zero: st_j + PCF == 0 mod r"""
    c = PCF[6 * rnd + j]
    return [R_MOD - c, 2 * R_MOD - c]


def _rand_elem(rnd, wide=None):
    """a value of the domain: canonical, or in [r, 2r)"""
    wide = rnd.randrange(2) if wide is None else wide
    return rnd.randrange(R_MOD) + (R_MOD if wide else 0)


def _placed(rnd, k, values_at):
    """rows of k elements: every value of values_at(p) at position p with the other k - 1 random (half of them canonical, half in
    [r, 2r), alternating from row to row)"""
    rows = []
    for p in range(k):
        for v in values_at(p):
            row = [_rand_elem(rnd, (len(rows) + q) & 1) for q in range(k)]
            row[p] = v
            rows.append(tuple(row))
    return rows


def p5_edge_rows():
    """each edge value in each of the five positions with the other four random, and in all five at once; for position j the two
    representatives of the value that makes the first S-box input of state element j + 1 zero, alone and in all five at once"""
    rnd = random.Random(0x4A5E0)
    ev = edge_values()
    rows = _placed(rnd, 5, lambda p: ev) + [(v,) * 5 for v in ev]
    rows += _placed(rnd, 5, lambda p: sbox_zero_reps(0, p + 1))
    rows += [tuple(sbox_zero_reps(0, p + 1)[k] for p in range(5)) for k in range(2)]
    return dedup(rows)


def full_round_edge_rows():
    """every round index: the edge values in each of the six positions and in all six, and the states that make S-box input j a
    representative of zero, alone and all six at once"""
    rnd = random.Random(0x4A5E1)
    ev = edge_values()
    rows = []
    for r in range(8):
        part = _placed(rnd, 6, lambda p: ev) + [(v,) * 6 for v in ev]
        part += _placed(rnd, 6, lambda p: sbox_zero_reps(r, p))
        part += [tuple(sbox_zero_reps(r, p)[k] for p in range(6)) for k in range(2)]
        rows += [row + (r,) for row in part]
    return dedup(rows)


def challenge_edge_rows():
    """the tag at the edges with random coordinates (nothing checks the curve equation at this level: the eight coordinates are
    field elements), and every edge value in all nine positions at once"""
    rnd = random.Random(0x4A5E2)
    ev = edge_values()
    rows = [(v,) + tuple(_rand_elem(rnd, (i + q) & 1) for q in range(8)) for i, v in enumerate(ev)]
    return dedup(rows + [(v,) * 9 for v in ev])


def edge_set(op):
    if op in ("p5_plain", "p5_pairs"):
        return p5_edge_rows()
    if op == "full_round":
        return full_round_edge_rows()
    if op in ("challenge_plain", "challenge_pairs"):
        return challenge_edge_rows()
    raise ValueError(op)


def random_set(op, rnd, n):
    """n seeded random items: every element uniform below 2r; one item in eight with one element at an edge value"""
    ev, k = edge_values(), NELEMS[op]
    out = []
    for i in range(n):
        row = [rnd.randrange(2 * R_MOD) for _ in range(k)]
        if i % 8 == 7:
            row[rnd.randrange(k)] = ev[rnd.randrange(len(ev))]
        if op == "full_round":
            row.append(rnd.randrange(8))
        out.append(tuple(row))
    return out


def in_domain(op, item):
    k = NELEMS[op]
    if len(item) != k + (1 if op == "full_round" else 0) or not all(0 <= v < 2 * R_MOD for v in item[:k]):
        return False
    return op != "full_round" or 0 <= item[6] < 8


# ---- checks ----------------------------------------------------------------------------------------------------------------
def _nform_ok(limbs):
    """per row: limbs 0 .. 7 < 2^29 and the top limb < 2^26"""
    limbs = np.asarray(limbs)
    return (limbs[:, :8] <= M29).all(axis=1) & (limbs[:, 8] < (1 << 26))


def check(op, items, out, want=None):
    """indices (with a reason) where the op's output is not what the integers say.  want: the hashes / challenges of
    expected_c; the model's when None"""
    out = np.asarray(out, dtype=np.uint32)
    n = len(items)
    assert out.shape == (n, WIDTHS[op][1]), (op, out.shape)
    want = expected(op, items) if want is None else want
    assert len(want) == n
    bad = []
    if op in ("p5_plain", "p5_pairs"):
        raw, ok, canon = vals_of_limbs(out[:, :NL]), _nform_ok(out[:, :NL]), vals_of_words(out[:, NL:])
        for i in range(n):
            if not ok[i] or raw[i] >= 2 * R_MOD or plain(raw[i]) != want[i] or canon[i] != want[i]:
                bad.append((i, "limbs %s (value %d), words %d, want %d" % (out[i, :NL].tolist(), raw[i], canon[i], want[i])))
    elif op in ("challenge_plain", "challenge_pairs"):
        for i, c in enumerate(vals_of_words(out)):
            if c != want[i]:
                bad.append((i, "challenge %d, want %d" % (c, want[i])))
    elif op == "full_round":
        el = out.reshape(n * 6, NL)
        raw, ok = vals_of_limbs(el), _nform_ok(el)
        for i in range(n):
            last = items[i][6] == 7
            for j in range(6):
                q = 6 * i + j
                if last and j:
                    good = not el[q].any()                          # the record's undefined part: written as zeros
                else:
                    good = ok[q] and raw[q] < 2 * R_MOD and plain(raw[q]) == want[i][j]
                if not good:
                    bad.append((i, "element %d: limbs %s (value %d), want %d" % (j, el[q].tolist(), raw[q], want[i][j])))
                    break
    else:
        raise ValueError(op)
    return bad


def check_six_lane(items, out, want):
    """the six-lane kernel's record: 8 lanes x 9 limbs.  All eight lanes hold identical limbs, in N-form with the top limb below
    2^26, and the value is the hash mod r (the representative is the lane form's or another: lane 0 weak-reduces where the lane
    form takes a dot product)"""
    out = np.asarray(out, dtype=np.uint32)
    n = len(items)
    assert out.shape == (n, P5C_GROUP * NL) and len(want) == n
    lanes = out.reshape(n, P5C_GROUP, NL)
    same = (lanes == lanes[:, :1, :]).all(axis=(1, 2))
    raw, ok = vals_of_limbs(lanes[:, 0, :]), _nform_ok(lanes[:, 0, :])
    bad = []
    for i in range(n):
        if not same[i] or not ok[i] or plain(raw[i]) != want[i]:
            bad.append((i, "lanes %s, want %d" % (lanes[i].tolist() if not same[i] else lanes[i, 0].tolist(), want[i])))
    return bad


def largest_over_r(limbs):
    """the largest value among the limb rows, in units of r"""
    return max(vals_of_limbs(np.asarray(limbs).reshape(-1, NL))) / R_MOD


def cpu_run(lib, op, recs):
    """the op on the CPU harness (tests/emul/emul_hash_ops.cpp: the g++ build of hash_ops.hpp) -> (n, out words) uint32"""
    n = recs.shape[0]
    wi, wo = WIDTHS[op]
    assert recs.shape == (n, wi)
    recs = np.ascontiguousarray(recs, dtype=np.uint32)
    out = np.zeros((n, wo), dtype=np.uint32)
    vp = ctypes.c_void_p

    def part(lo, hi):
        return lib.emul_hash_op(ctypes.c_int(OPS[op]), recs[lo:hi].ctypes.data_as(vp), out[lo:hi].ctypes.data_as(vp), ctypes.c_size_t(hi - lo))
    # the items are independent and the library keeps no state: slices on a few threads (ctypes releases the GIL)
    nthr = max(1, min(8, os.cpu_count() or 1, n // 256))
    cuts = [n * k // nthr for k in range(nthr + 1)]
    if nthr == 1:
        rcs = [part(0, n)]
    else:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(nthr) as ex:
            rcs = list(ex.map(lambda k: part(cuts[k], cuts[k + 1]), range(nthr)))
    assert all(rc == 0 for rc in rcs)
    return out
