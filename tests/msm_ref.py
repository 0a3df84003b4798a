"""Plain-integer model of the bucket pipeline of bjj_msm / bjj_msm_batch (csrc/msm.hpp, k_msm.hip, k_msm_batch.hip), stage by stage:
digits, keys, histogram, cursors, records, buckets, window sums, the final point -- and one checker per stage that holds the arrays
the device left behind against the model and returns a list of findings.  Shared by tests/test_gpu_msm_stages.py (the stages on the
device through tests/devfuzz/msm.hip) and tests/test_msm_stages_host.py (the model against tests/msm_emul, the checkers against
seeded mutants).  A plain helper module in the style of tests/curve_ref.py: no tests, no fixtures, nothing imported from oracle/.

Points have KNOWN LOGARITHMS: a point is the pair (p, t) that stands for p B8 + t T8, p mod l, t mod 8 (the group is Z_l x Z_8).
Every expected bucket, window sum and result is computed on the pairs -- sum of +-p mod l, sum of +-t mod 8 -- and becomes a point by
ONE scalar multiplication of the C oracle (class Points: mul_var_base of B8, point_add of the torsion point), never by an addition
per record.  Device values are compared as POINTS: a stored Ext is 4 x 9 raw Montgomery limbs on the a' = -1 curve, decoded with the
limb helpers of field_ref / curve_ref to affine reference coordinates (representatives are not unique).

A finding is a tuple (stage, key or index, what differs)."""
import random

import numpy as np

import curve_ref as cr
import field_ref as fr

R_MOD = fr.R_MOD
SUBORDER = cr.SUBORDER
ORDER8 = 8 * SUBORDER
ENTRY_WORDS, NIELS_WORDS = 40, 32
SEG, GROUP, LEVEL_SLICE = 8, 8, 8
SCAN_TILE, TOP_BLOCK, BLOCK = 4096, 1024, 256
FILL = 0xA5
FILL32 = 0xA5A5A5A5
FILL64 = 0xA5A5A5A5A5A5A5A5
MAX_FINDINGS = 8
IDENTITY_LOG = (0, 0)


# ---- the schedule (msm.hpp, k_msm.hip: layout) ---------------------------------------------------------------------------------------
def windows(c):
    return (255 + c - 1) // c


def buckets(c):
    return 1 << (c - 1)


def div_up(a, b):
    return (a + b - 1) // b


def slice_records(records):
    """the product's slice size for a record bound"""
    S = 8
    while S < 64 and records // S > 1 << 18:
        S <<= 1
    return S


def level_count(records, S1):
    slices, levels = div_up(records if records else 1, S1), 0
    while slices > 1:
        slices = div_up(2 * slices, LEVEL_SLICE)
        levels += 1
    return levels


def group_passes(G):
    """[F of every bjj_k_msm_group pass]"""
    out = []
    while G > 1:
        F = min(G, GROUP)
        G //= F
        out.append(F)
    return out


# ---- digits and keys -----------------------------------------------------------------------------------------------------------------
def digits(k, c):
    """the signed c-bit digits of k mod 8l, window 0 first: d in [-2^(c-1), 2^(c-1)], a window value ABOVE 2^(c-1) borrows from the next"""
    k %= ORDER8
    half, mask, carry, out = 1 << (c - 1), (1 << c) - 1, 0, []
    for j in range(windows(c)):
        v = ((k >> (c * j)) & mask) + carry
        if v > half:
            carry = 1
            out.append(v - (1 << c))
        else:
            carry = 0
            out.append(v)
    assert carry == 0
    return out


def key_of(s, j, d, c):
    """(s W + j) B + |d| - 1 (s = 0: bjj_msm)"""
    return (s * windows(c) + j) * buckets(c) + abs(d) - 1


def record(key, item, neg):
    return (key << 33) | (item << 1) | (1 if neg else 0)


def segment_of(offsets, i):
    """the last s in [0, m - 1] with offsets[s] <= i"""
    m = len(offsets) - 1
    s = 0
    for t in range(1, m):
        if offsets[t] <= i:
            s = t
    return s


# ---- logarithms ----------------------------------------------------------------------------------------------------------------------
def ladd(a, b):
    return ((a[0] + b[0]) % SUBORDER, (a[1] + b[1]) % 8)


def lneg(a):
    return (-a[0] % SUBORDER, -a[1] % 8)


def lmul(k, a):
    return (k * a[0] % SUBORDER, k * a[1] % 8)


def lsum(terms):
    """sum of k * log over (k, log) pairs"""
    p = t = 0
    for k, a in terms:
        p += k * a[0]
        t += k * a[1]
    return (p % SUBORDER, t % 8)


def _le32(v):
    return int(v).to_bytes(32, "little")


def pack_points(pts):
    return np.frombuffer(b"".join(_le32(x) + _le32(y) for x, y in pts), np.uint8).reshape(-1, 64).copy()


def pack_scalars(ks):
    return np.frombuffer(b"".join(_le32(k) for k in ks), np.uint8).reshape(-1, 32).copy()


def unpack_points(arr):
    b = np.ascontiguousarray(arr, np.uint8).tobytes()
    return [(int.from_bytes(b[i:i + 32], "little"), int.from_bytes(b[i + 32:i + 64], "little")) for i in range(0, len(b), 64)]


class Points:
    """(p, t) -> the affine reference point p B8 + t T8, by the C oracle: one mul_var_base of B8 per new p and one point_add of the
    torsion point j T8 (tests/golden/gpu_expected.json); answers are kept"""

    def __init__(self, oracle):
        self.oracle = oracle
        self.torsion = pack_points(cr.TORSION_REF)
        self.known = {IDENTITY_LOG: (0, 1)}
        self.multiplications = 0

    def of(self, logs):
        logs = [(a[0] % SUBORDER, a[1] % 8) for a in logs]
        new = [a for a in dict.fromkeys(logs) if a not in self.known]
        if new:
            base = np.tile(pack_points([fr.B8]), (len(new), 1))
            pb = self.oracle.mul_var_base(base, pack_scalars([a[0] for a in new]))
            pts = self.oracle.point_add(pb, self.torsion[[a[1] for a in new]])
            self.multiplications += len(new)
            for a, p in zip(new, unpack_points(pts)):
                self.known[a] = p
                self.known[lneg(a)] = (-p[0] % R_MOD, p[1])
        return [self.known[a] for a in logs]


def make_pool(n, seed, torsion_first=False):
    """n logs: seeded points of the whole group, every third one torsion-shifted; from n = 8 on the identity, the point of order 2
    and a pair P, -P are among them (indices 1, 2, 4 and 5).  torsion_first: indices 0 .. 7 are the eight torsion points j T8."""
    rnd = random.Random(seed)
    logs = [(rnd.randrange(1, SUBORDER), rnd.randrange(1, 8) if i % 3 == 0 else 0) for i in range(n)]
    if torsion_first:
        assert n >= 16
        logs[:8] = [(0, t) for t in range(8)]
        logs[9] = lneg(logs[8])
    elif n >= 8:
        logs[1], logs[2], logs[5] = (0, 0), (0, 4), lneg(logs[4])
    return logs


def off_curve(p):
    """a record one bit away from p that is not on the curve"""
    q = (p[0] ^ 1, p[1])
    assert not fr.on_curve(*q)
    return q


# ---- scalar sets -----------------------------------------------------------------------------------------------------------------------
def digit_scalars(c):
    """scalars built from digits, all below 8l so that the reduction leaves them alone: every window at exactly 2^(c-1)
    (digit 2^(c-1), the last bucket, no carry); every window at 2^(c-1) + 1 (a carry out of every window); a carry out of window
    0 that ripples through windows of all ones up to the top; only the top window non-zero"""
    W, half = windows(c), 1 << (c - 1)
    full = [j for j in range(W) if c * (j + 1) <= 253]
    at = sum(half << (c * j) for j in full)
    above = sum((half + 1) << (c * j) for j in full)
    ripple = (1 << 253) - (1 << c) + half + 1
    top = 1 << (c * (W - 1))
    out = [at, above, ripple, top]
    assert all(0 < k < ORDER8 for k in out)
    return out


def scalar_sets(n, c, seed, edge):
    """name -> n scalars (256-bit integers); edge: the EDGE_SCALARS of tests/test_msm_host.py"""
    rnd = random.Random(seed)
    dg = digit_scalars(c)
    k = rnd.getrandbits(256)
    return {
        "random": [rnd.getrandbits(256) for _ in range(n)],
        "edge": [edge[i % len(edge)] for i in range(n)],
        "digits": [dg[i % len(dg)] for i in range(n)],
        "digit_at_half": [dg[0]] * n,
        "digit_above_half": [dg[1]] * n,
        "ripple": [dg[2]] * n,
        "top_window": [dg[3]] * n,
        "one_window": [1 + rnd.randrange(1 << (c - 1)) for _ in range(n)],
        "zero": [0] * n,
        "equal": [k] * n,
    }


# ---- the model of one call ---------------------------------------------------------------------------------------------------------------
class Model:
    """every stage of one call in plain integers.  logs[i]: the item's point (None where `bad` names it: an off-curve record);
    offsets: the CSR offsets of the batched form (None: bjj_msm)"""

    def __init__(self, logs, scalars, c, offsets=None, bad=()):
        n = len(scalars)
        assert len(logs) == n and 4 <= c <= 20
        self.n, self.c, self.W, self.B = n, c, windows(c), buckets(c)
        self.offsets = list(offsets) if offsets is not None else [0, n]
        self.m = len(self.offsets) - 1
        assert self.offsets[0] == 0 and self.offsets[-1] == n and all(a <= b for a, b in zip(self.offsets, self.offsets[1:]))
        self.M = self.m * self.W * self.B
        self.logs = list(logs)
        self.bad = sorted(bad)
        self.seg = [0] * n
        for s in range(self.m):
            for i in range(self.offsets[s], self.offsets[s + 1]):
                self.seg[i] = s
        self.red = [0 if i in bad else k % ORDER8 for i, k in enumerate(scalars)]
        self.status = [-1] * self.m
        for i in reversed(self.bad):
            self.status[self.seg[i]] = i
        self.by_key = {}
        for i, k in enumerate(self.red):
            if k:
                for j, d in enumerate(digits(k, c)):
                    if d:
                        self.by_key.setdefault(key_of(self.seg[i], j, d, c), []).append((i, d < 0))
        self._finish()

    @classmethod
    def synthetic(cls, logs, recs, c):
        """a model whose records are the test's: recs = [(key, item, neg)] in key order (bjj_msm keys)"""
        self = cls.__new__(cls)
        self.n, self.c, self.W, self.B = len(logs), c, windows(c), buckets(c)
        self.m, self.offsets, self.M = 1, [0, len(logs)], windows(c) * buckets(c)
        self.logs, self.bad, self.status = list(logs), [], [-1]
        self.by_key = {}
        for key, item, neg in recs:
            self.by_key.setdefault(key, []).append((item, bool(neg)))
        self._finish(order=[record(*r) for r in recs])
        return self

    def _finish(self, order=None):
        self.counts = np.zeros(self.M, dtype=np.uint32)
        for key, rs in self.by_key.items():
            self.counts[key] = len(rs)
        self.cursor = exclusive_scan(self.counts)
        self.total = int(self.counts.sum(dtype=np.uint64))
        if order is None:
            order = [record(key, i, neg) for key in sorted(self.by_key) for i, neg in self.by_key[key]]
        self.records = np.array(order, dtype=np.uint64)
        self.bucket_logs = {key: lsum((-1 if neg else 1, self.logs[i]) for i, neg in rs) for key, rs in self.by_key.items()}
        nwin = self.m * self.W
        terms = [[] for _ in range(nwin)]
        for key, a in self.bucket_logs.items():
            terms[key // self.B].append((key % self.B + 1, a))
        self.window_logs = [lsum(t) for t in terms]
        self.result_logs = [lsum((1 << (self.c * j), self.window_logs[s * self.W + j]) for j in range(self.W)) for s in range(self.m)]

    def results(self, points):
        """the m expected 64-byte records: (0, 0) for a segment with an off-curve record"""
        pts = points.of(self.result_logs)
        return pack_points([(0, 0) if self.status[s] >= 0 else pts[s] for s in range(self.m)])

    def window_logs_without_the_segment_term(self):
        """what bjj_k_msm_windows would leave if it dropped (g L) R_g: sum over the buckets of (b - g L) B_b"""
        terms = [[] for _ in range(self.m * self.W)]
        for key, a in self.bucket_logs.items():
            b = key % self.B + 1
            terms[key // self.B].append((b - (b - 1) // SEG * SEG, a))
        return [lsum(t) for t in terms]


def exclusive_scan(counts):
    c = np.asarray(counts).astype(np.uint64)
    out = np.zeros(len(c), dtype=np.uint64)
    np.cumsum(c[:-1], out=out[1:])
    return out


# ---- validators of synthetic inputs (a test must never hand the kernels an index that leaves a buffer) ---------------------------------
def validate_synthetic(recs, M, pool_size, records_bound):
    """recs = [(key, item, neg)]: keys below M and non-decreasing, items below the pool size, no more records than the layout holds"""
    if len(recs) > records_bound:
        raise ValueError("%d records, the layout holds %d" % (len(recs), records_bound))
    last = 0
    for t, (key, item, neg) in enumerate(recs):
        if not 0 <= key < M:
            raise ValueError("record %d: key %d is not below %d" % (t, key, M))
        if key < last:
            raise ValueError("record %d: key %d after key %d" % (t, key, last))
        if not 0 <= item < pool_size:
            raise ValueError("record %d: item %d is not below %d" % (t, item, pool_size))
        if neg not in (0, 1, False, True):
            raise ValueError("record %d: sign %r" % (t, neg))
        last = key
    return True


def validate_counts(model, counts, cursor, total, records_bound):
    """the histogram, the cursors and the total a test uploads are the records' own"""
    if int(total) > records_bound or int(total) != len(model.records):
        raise ValueError("total %d against %d records (bound %d)" % (total, len(model.records), records_bound))
    keys = (model.records >> np.uint64(33)).astype(np.int64)
    if not (np.bincount(keys, minlength=model.M) == np.asarray(counts)).all():
        raise ValueError("counts are not the records' histogram")
    if not (exclusive_scan(counts) == np.asarray(cursor)).all():
        raise ValueError("cursor is not the exclusive prefix of counts")
    return True


def validate_counter_input(keys, active, arr_len):
    if len(keys) != len(active) or any(not 0 <= k < arr_len for k in keys):
        raise ValueError("a counter key is not below %d" % arr_len)
    return True


# ---- decoding device values --------------------------------------------------------------------------------------------------------------
def _batch_inverse(vals):
    """1 / v mod r for every v != 0 (None for 0): one inversion"""
    pre, acc = [], 1
    for v in vals:
        pre.append(acc)
        if v:
            acc = acc * v % R_MOD
    inv = pow(acc, -1, R_MOD)
    out = [None] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        if vals[i]:
            out[i] = inv * pre[i] % R_MOD
            inv = inv * vals[i] % R_MOD
    return out


def decode_ext(rows):
    """(k, >= 36) raw words -> per row the affine reference point (x' / F, y), or a string saying why it is no point: Z == 0, or
    T Z != X Y (the next addition reads T).  The Montgomery factor cancels in every quotient."""
    rows = np.asarray(rows, dtype=np.uint32)
    if len(rows) == 0:
        return []
    X, Y, Z, T = (fr.vals_of_limbs(rows[:, 9 * k:9 * k + 9]) for k in range(4))
    zi = _batch_inverse([z % R_MOD for z in Z])
    out = []
    for x, y, z, t, i in zip(X, Y, Z, T, zi):
        if i is None:
            out.append("Z is zero")
        elif (t * z - x * y) % R_MOD:
            out.append("T Z != X Y")
        else:
            out.append((x * i * cr.FINV % R_MOD, y * i % R_MOD))
    return out


def encode_ext(p, z=1, key=0, live=1):
    """an entry (40 words) holding the reference point p: canonical Montgomery limbs of (F x z, y z, z, F x y z)"""
    x, y = cr.to_m1(p)
    c = cr.ext_coords((x, y), z)
    return sum((fr.nform(fr.mont(v)) for v in c), ()) + (key, live, 0, 0)


def decode_niels(rows):
    """(k, 32) words -> per row the plain (y - x, y + x, 2 D' x y) of the entry"""
    rows = np.asarray(rows, dtype=np.uint32)
    c = [fr.vals_of_limbs(rows[:, 9 * k:9 * k + 9]) for k in range(3)]
    return [tuple(v * fr.RINV % R_MOD for v in t) for t in zip(*c)]


def _some(findings):
    return findings[:MAX_FINDINGS]


# ---- the checkers: one per stage ---------------------------------------------------------------------------------------------------------
def check_prepare(model, points, red, niels, counts, status, seg=None):
    """points: the n affine reference records handed to the device (an off-curve one among them where the model says so)"""
    out = []
    red = np.asarray(red, dtype=np.uint32).reshape(model.n, 8)
    for i, (got, want) in enumerate(zip(fr.vals_of_words(red), model.red)):
        if got != want:
            out.append(("red", i, "%#x, want %#x" % (got, want)))
    ent = decode_niels(np.asarray(niels, dtype=np.uint32).reshape(model.n, NIELS_WORDS))
    for i, p in enumerate(points):
        if i not in model.bad and ent[i] != cr.niels_coords(cr.to_m1(p)):
            out.append(("niels", i, "not (y - x, y + x, 2 D' x y) of (F x, y)"))
    counts = np.asarray(counts, dtype=np.uint32)
    for key in np.nonzero(counts != model.counts)[0][:MAX_FINDINGS]:
        out.append(("counts", int(key), "%d, want %d" % (counts[key], model.counts[key])))
    status = [int(v) for v in np.asarray(status).astype(np.int64)]
    if status != model.status:
        out.append(("status", 0, "%s, want %s" % (status[:4], model.status[:4])))
    if seg is not None:
        for i in np.nonzero(np.asarray(seg, dtype=np.int64) != np.array(model.seg))[0][:MAX_FINDINGS]:
            out.append(("seg", int(i), "%d, want %d" % (seg[i], model.seg[i])))
    return _some(out)


def check_scan(counts, cursor, total):
    """cursor and total against numpy.cumsum in uint64"""
    counts = np.asarray(counts, dtype=np.uint32)
    cursor = np.asarray(cursor, dtype=np.uint64)
    want = exclusive_scan(counts)
    out = [("cursor", int(k), "%d, want %d" % (cursor[k], want[k])) for k in np.nonzero(cursor != want)[0][:MAX_FINDINGS]]
    t = int(counts.sum(dtype=np.uint64))
    if int(total) != t:
        out.append(("total", 0, "%d, want %d" % (int(total), t)))
    return out


def check_records(model, rec, cursor, counts):
    """for each key the slots [cursor, cursor + count) hold exactly the model's set of (item, sign) records, in any order.
    cursor, counts: what the device had BEFORE the scatter (checked on their own by check_scan / check_prepare)"""
    rec = np.asarray(rec, dtype=np.uint64)
    counts = np.asarray(counts, dtype=np.uint32)
    cursor = np.asarray(cursor, dtype=np.uint64)
    out = []
    total = int(counts.sum(dtype=np.uint64))
    if total != model.total or len(rec) < total:
        return [("rec", 0, "%d slots for %d records (model %d)" % (len(rec), total, model.total))]
    live = np.nonzero(counts)[0]
    want_keys = np.repeat(live, counts[live]).astype(np.uint64)
    starts = np.repeat(cursor[live], counts[live])
    slots = (starts + (np.arange(total, dtype=np.uint64) - np.repeat(exclusive_scan(counts)[live], counts[live]))).astype(np.int64)
    if total and (slots.max() >= len(rec) or slots.min() < 0):
        return [("rec", 0, "a cursor points outside the record array")]
    got = rec[slots]
    wrong_key = np.nonzero((got >> np.uint64(33)) != want_keys)[0]
    for t in wrong_key[:MAX_FINDINGS]:
        out.append(("rec", int(want_keys[t]), "slot %d holds %#x: not a record of this key" % (slots[t], int(got[t]))))
    a, b = np.sort(got), np.sort(model.records)
    for t in np.nonzero(a != b)[0][:MAX_FINDINGS]:
        out.append(("rec", int(b[t]) >> 33, "record (item %d, sign %d) missing; the device has %#x" % ((int(b[t]) >> 1) & 0xffffffff, int(b[t]) & 1,
                                                                                                        int(a[t]))))
    return _some(out)


def check_buckets(model, points, bucket_words, counts, fill=True):
    """bucket_words: (M, 40) words.  Every key with counts > 0 holds the model's bucket as a point; with `fill`, every other key
    still holds the 0xA5 bytes the test wrote before the run (its 36 value words)"""
    bw = np.asarray(bucket_words, dtype=np.uint32).reshape(model.M, ENTRY_WORDS)
    counts = np.asarray(counts, dtype=np.uint32)
    out = []
    live = [int(k) for k in np.nonzero(counts)[0]]
    if set(live) != set(model.bucket_logs):
        return [("buckets", 0, "the live keys of counts are not the model's")]
    want = points.of([model.bucket_logs[k] for k in live])
    for key, got, w in zip(live, decode_ext(bw[live]), want):
        if got != w:
            out.append(("bucket", key, got if isinstance(got, str) else "another point than the sum of its %d records" % counts[key]))
    if fill:
        dead = np.nonzero((counts == 0) & (bw[:, :36] != FILL32).any(axis=1))[0]
        out += [("bucket", int(k), "written, but no record names this key") for k in dead[:MAX_FINDINGS]]
    return _some(out)


def check_window_sums(model, points, wsum_words):
    """wsum_words: (m W, 40) words against sum_b b * B_b"""
    ww = np.asarray(wsum_words, dtype=np.uint32).reshape(model.m * model.W, ENTRY_WORDS)
    want = points.of(model.window_logs)
    return _some([("wsum", j, got if isinstance(got, str) else "not the sum of b * B_b") for j, (got, w) in enumerate(zip(decode_ext(ww), want))
                  if got != w])


def check_result(model, points, out_bytes):
    got = np.asarray(out_bytes, dtype=np.uint8).reshape(model.m, 64)
    want = model.results(points)
    return _some([("out", s, "%s, want %s" % (unpack_points(got[s]), unpack_points(want[s]))) for s in range(model.m) if (got[s] != want[s]).any()])


def check_counter(bits, init, keys, active, returned, arr_before, arr_after):
    """arr[key] grew by exactly the number of active lanes naming it, and the values returned to those lanes are a permutation of
    init .. init + count - 1 (mod 2^bits).  Nothing is asserted about inactive lanes."""
    mod = 1 << bits
    lanes = {}
    for i, (k, a) in enumerate(zip(keys, active)):
        if a:
            lanes.setdefault(int(k), []).append(i)
    out = []
    for k in range(len(arr_before)):
        cnt = len(lanes.get(k, ()))
        if (int(arr_before[k]) + cnt) % mod != int(arr_after[k]):
            out.append(("counter", k, "grew by %d, want %d" % ((int(arr_after[k]) - int(arr_before[k])) % mod, cnt)))
    for k, ls in lanes.items():
        got = sorted((int(returned[i]) - int(arr_before[k])) % mod for i in ls)
        if got != list(range(len(ls))):
            rep = [v for v, w in zip(got, got[1:]) if v == w]
            out.append(("counter", k, "positions are no permutation" + (": %d repeats" % rep[0] if rep else "")))
    return _some(out)
