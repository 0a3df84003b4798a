"""Plain-integer model and input sets for the part of the field layer that the multiplier fuzz does not reach: the additive
forms of csrc/fr.hpp (fr_add, fr_sub, fr_sub8 and their lazy forms), fr_reduce_weak, fr_canon / fr_is_zero / fr_eq, the word and
Montgomery conversions, and the square-root and codec block of csrc/bjj_device.hpp (fr_sqrt, plain_gt_halfq, words_ge_modulus /
words_gt_modulus, decompress_item, compress_item) with ref_on_curve.  Shared by tests/test_field_ops_host.py (the g++ build of
tests/devfuzz/field_ops.hpp with the bound assertions live) and tests/test_gpu_field_ops.py (the same dispatcher on the
device, tests/devfuzz/field.hip).  A plain helper module: no fixtures, no pytest hooks, nothing imported from oracle/;
beside the model it holds only cpu_run, the call into the CPU library that the test modules' fixture builds.

An item is a tuple of one or two raw vectors (tuples of ints): 9 limbs of 29 bits (value = sum v[i] 2^(29 i); limbs may exceed
29 bits where the op's domain says so) or 8 words of 32 bits.  Every constant below is derived from r here, not read from the
header, so a wrong constant in the header is a failing test.  Equalities are over the integers unless "mod r" is written.
Every random generator builds its inputs inside the op's domain by construction (randrange(bound), then limbs): nothing is
rejected or left out."""
import json
import os
import random

import numpy as np

R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
RADIX = 1 << 261
RINV = pow(RADIX, -1, R_MOD)
R1 = RADIX % R_MOD
M29 = (1 << 29) - 1
ONES30 = (1 << 30) - 1
TOP_R = R_MOD >> 232                # 3171406: top limb of r
TOP_DIV = TOP_R + 1                 # fr_reduce_weak's divisor
HALF = (R_MOD - 1) // 2
A_REF, D_REF = 168700, 168696
B8 = (5299619240641551281634865583518297030282874472190772894086521144482721001553,
      16950150798460657717958625567821834550301663161624707787222815936182638968203)
TS_S = (R_MOD - 1) >> 28            # r - 1 = 2^28 s, s odd
TS_G = pow(5, TS_S, R_MOD)          # generator of the subgroup of order 2^28 (5: the least non-residue)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# op codes and record widths (a, b, out) of tests/devfuzz/field_ops.hpp
OPS = dict(add=0, dbl=1, add_lazy=2, sub=3, neg=4, sub8=5, sub_lazy=6, sub8_of_lazy=7, reduce_weak=8, canon=9, is_zero=10, eq=11,
           from_words=12, to_words=13, to_mont=14, from_mont=15, gt_halfq=16, words_ge_r=17, words_gt_r=18, sqrt=19, on_curve=20,
           decompress=21, compress=22)
WIDTHS = dict(add=(9, 9, 9), dbl=(9, 0, 9), add_lazy=(9, 9, 9), sub=(9, 9, 9), neg=(9, 0, 9), sub8=(9, 9, 9), sub_lazy=(9, 9, 9),
              sub8_of_lazy=(9, 9, 9), reduce_weak=(9, 0, 9), canon=(9, 0, 9), is_zero=(9, 0, 1), eq=(9, 9, 1), from_words=(8, 0, 9),
              to_words=(9, 0, 8), to_mont=(8, 0, 9), from_mont=(9, 0, 8), gt_halfq=(9, 0, 1), words_ge_r=(8, 0, 1),
              words_gt_r=(8, 0, 1), sqrt=(9, 0, 10), on_curve=(9, 9, 1), decompress=(8, 0, 17), compress=(8, 8, 8))


# ---- limbs and words -------------------------------------------------------------------------------------------------------
def nform(v):
    """N-form limbs of v >= 0: limbs 0..7 < 2^29, the rest in limb 8"""
    return tuple((v >> (29 * i)) & M29 for i in range(8)) + (v >> 232,)


def lval(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def words(v):
    return tuple((v >> (32 * j)) & 0xffffffff for j in range(8))


def wval(w):
    return sum(int(x) << (32 * j) for j, x in enumerate(w))


def lazy(v, rnd=None):
    """the same value with carries pushed DOWN: limb i += 2^29, limb i+1 -= 1 (limbs stay < 2^30); every carry that can be
    pushed when rnd is None, each with probability 1/2 otherwise"""
    l = list(nform(v))
    for i in range(8):
        if l[i + 1] > 0 and (rnd is None or rnd.random() < 0.5):
            l[i] += 1 << 29
            l[i + 1] -= 1
    return tuple(l)


def borrowed(k, bits, lend):
    """k r with borrowed limbs: limb 0 += 2^bits, limbs 1..7 += 2^bits - lend, limb 8 -= lend (lend = 2^(bits - 29))"""
    d = nform(k * R_MOD)
    return (d[0] + (1 << bits),) + tuple(x + (1 << bits) - lend for x in d[1:8]) + (d[8] - lend,)


C4 = borrowed(4, 29, 1)             # fr_c4limb
C8 = borrowed(8, 29, 1)             # fr_c8limb
K8 = borrowed(8, 30, 2)             # fr_k8limb
assert lval(C4) == 4 * R_MOD and lval(C8) == 8 * R_MOD and lval(K8) == 8 * R_MOD
assert min(K8[:8]) >= ONES30 and max(C4[1:8]) >= M29


def mont(v):
    return v * RADIX % R_MOD


def vals_of_limbs(rows):
    """the Python integers of many limb rows at once (limbs up to 32 bits): pairs of limbs are joined in numpy first"""
    x = np.asarray(rows).astype(np.uint64)
    c = [(x[:, 2 * j] + (x[:, 2 * j + 1] << np.uint64(29))).tolist() for j in range(4)] + [x[:, 8].tolist()]
    return [a + (b << 58) + (cc << 116) + (d << 174) + (e << 232) for a, b, cc, d, e in zip(*c)]


def vals_of_words(rows):
    x = np.asarray(rows).astype(np.uint64)
    c = [(x[:, 2 * j] | (x[:, 2 * j + 1] << np.uint64(32))).tolist() for j in range(4)]
    return [a | (b << 64) | (cc << 128) | (d << 192) for a, b, cc, d in zip(*c)]


def dedup(items):
    seen, out = set(), []
    for v in items:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


# ---- the shared operand classes, as raw 9-limb vectors ---------------------------------------------------------------------
def nform_values():
    v = [k * R_MOD + d for k in range(16) for d in (-1, 0, 1)] + [16 * R_MOD - 1]
    v += [(1 << (29 * i)) + d for i in range(1, 9) for d in (-1, 0, 1)]
    return dedup(x for x in v if x >= 0)


ONES_TOPS = (0, 1, TOP_R - 1, TOP_R, 4 * TOP_R, 13 * TOP_R - 3)


def nform_class():
    return dedup([nform(v) for v in nform_values()] + [(M29,) * 8 + (t,) for t in ONES_TOPS])


def lazy_class():
    rnd = random.Random(0xF1E1D)
    out = []
    for l in nform_class():
        v = lval(l)
        out += [lazy(v), lazy(v, rnd)]
    return dedup(out + [(ONES30,) * 9, (ONES30 - 1,) * 9])


def any_class():
    """limbs < 2^30: what fr_add and the minuend of fr_sub accept"""
    return dedup(nform_class() + lazy_class())


def subtrahends(C):
    """N-form b with top limb <= C[8], plus the edges of the borrowed constant C: the largest top limb over all-ones limbs, C
    itself limb for limb (every limb of the difference 0), C with one limb one smaller, zero"""
    out = [l for l in nform_class() if l[8] <= C[8]]
    out += [(M29,) * 8 + (C[8],), (0,) * 8 + (C[8],), tuple(C), (0,) * 9, nform(lval(C) - (1 << 232) - 1)]
    out += [tuple(C[j] - (1 if j == i else 0) for j in range(9)) for i in range(9)]
    out += [tuple(min(C[j], M29) for j in range(8)) + (C[8],)]
    return dedup(out)


def lazy_subtrahends():
    """b with b_i <= fr_k8limb(i): lazy limbs under a top limb <= K8[8]"""
    out = [l for l in any_class() if l[8] <= K8[8]]
    out += [(ONES30,) * 8 + (K8[8],), (ONES30 - 1,) * 8 + (K8[8],), tuple(K8), (0,) * 9, (0,) * 8 + (K8[8],)]
    out += [tuple(K8[j] - (1 if j == i else 0) for j in range(9)) for i in range(9)]
    return dedup(out)


def minuends_small():
    return [(0,) * 9, (ONES30,) * 9, nform(R_MOD - 1), lazy(2 * R_MOD), (M29,) * 8 + (13 * TOP_R - 3,), nform(12 * R_MOD - 1)]


def cross_sub(bs, C):
    """(a, b): a few minuends against every subtrahend, and every operand class member against a few subtrahends"""
    few_b = [(0,) * 9, tuple(C), ((ONES30 if C is K8 else M29),) * 8 + (C[8],), nform(2 * R_MOD - 1), nform(R_MOD)]
    return dedup([(a, b) for a in minuends_small() for b in bs] + [(a, b) for a in any_class() for b in few_b])


def word_values():
    v = [0, 1, 2, (1 << 256) - 1, (1 << 256) - 2, 1 << 255, (1 << 255) - 1, R_MOD - 1, R_MOD, R_MOD + 1, HALF, HALF + 1]
    v += [R_MOD + s * (1 << (32 * j)) for j in range(1, 8) for s in (1, -1)]
    v += [k * R_MOD + d for k in range(1, 6) for d in (-1, 0, 1)]
    bits = sorted(set([29 * i + d for i in range(1, 9) for d in (-1, 0)] + [32 * j + d for j in range(1, 8) for d in (-1, 0)] + [0, 255]))
    for b in bits:
        v += [1 << b, (1 << b) - 1, (1 << b) + 1, ((1 << 256) - 1) ^ (1 << b)]
    return dedup(x for x in v if 0 <= x < 1 << 256)


# ---- the curve and the square root in plain integers ----------------------------------------------------------------------
def is_residue(a):
    return pow(a % R_MOD, HALF, R_MOD) == 1


def on_curve(x, y):
    x2, y2 = x * x, y * y
    return (A_REF * x2 + y2 - 1 - D_REF * x2 * y2) % R_MOD == 0


def point_add(p, q):
    (x1, y1), (x2, y2) = p, q
    t = D_REF * x1 * x2 * y1 * y2 % R_MOD
    x3 = (x1 * y2 + y1 * x2) * pow(1 + t, -1, R_MOD) % R_MOD
    y3 = (y1 * y2 - A_REF * x1 * x2) * pow(1 - t, -1, R_MOD) % R_MOD
    return x3, y3


def modsqrt(a):
    """one square root of a residue a mod r (Tonelli-Shanks; used to build edge inputs only, never to judge an output)"""
    a %= R_MOD
    assert is_residue(a)
    x, b, g, m = pow(a, (TS_S + 1) // 2, R_MOD), pow(a, TS_S, R_MOD), TS_G, 28
    while b != 1:
        t, i = b, 0
        while t != 1:
            t, i = t * t % R_MOD, i + 1
        c = pow(g, 1 << (m - i - 1), R_MOD)
        x, g, m = x * c % R_MOD, c * c % R_MOD, i
        b = b * g % R_MOD
    assert x * x % R_MOD == a
    return x


def y_of_x(x):
    """the two y with (x, y) on the curve, or [] : y^2 = (1 - A x^2) / (1 - D x^2)"""
    y2 = (1 - A_REF * x * x) * pow(1 - D_REF * x * x, -1, R_MOD) % R_MOD
    if not is_residue(y2):
        return []
    y = modsqrt(y2)
    return [y, R_MOD - y]


def decompress_x2(v):
    """decompress_point (src/lib.rs:192-224) on the 256-bit integer v, up to the root: (y in range, x^2); Ok needs y in range and
    x^2 a non-zero residue (modsqrt errors on 0 and on non-residues)"""
    y = v & ((1 << 255) - 1)
    if y >= R_MOD:
        return False, 0
    return True, (1 - y * y) * pow(A_REF - D_REF * y * y, -1, R_MOD) % R_MOD      # A / D is a non-residue: never a zero denominator


def decompress_ok(v):
    inr, x2 = decompress_x2(v)
    return inr and x2 != 0 and is_residue(x2)


def compress_model(x, y):
    return (y % R_MOD) | ((1 << 255) if x % R_MOD > HALF else 0)


def golden_points(name):
    with open(os.path.join(GOLDEN, "gpu_expected.json")) as f:
        return [tuple(int(c, 16) for c in p) for p in json.load(f)[name]]


def golden_decompress_inputs():
    with open(os.path.join(GOLDEN, "oracle_vectors.json")) as f:
        return [int.from_bytes(bytes.fromhex(c["in"]), "little") for c in json.load(f)["decompress"]]


# ---- the square-root edge set ------------------------------------------------------------------------------------------------
# e = v 2^(7d): one digit v at position d (v even at d = 0): 448 (digit, position) pairs -- every entry of the four digit tables
# on its own --, 445 distinct logs (e = 0 is the same at every position)
SQRT_SINGLE_DIGIT_LOGS = [v << (7 * d) for d in range(4) for v in range(128) if d or v % 2 == 0]


# one digit v at position d < 3 under NON-ZERO digits at every higher position: a wrong entry of the stripping table (TSN) leaves
# a remainder outside the subgroup of the next digit, whose hash lookup then answers 0 for most values -- with zero digits
# above it the root would still come out right, so the single-digit logs alone cannot see such an entry
SQRT_STRIP_LOGS = [(v << (7 * d)) | sum((1 + (37 * v + k) % 127) << (7 * k) for k in range(d + 1, 4))
                   for d in range(3) for v in range(128) if d or v % 2 == 0]


def sqrt_value_of_log(e, h):
    """a plain residue a with a^s == G^e (e even): a = (G^k h)^2 with k = (e/2) s^-1 mod 2^27, h of odd order"""
    assert e % 2 == 0
    k = (e // 2) * pow(TS_S, -1, 1 << 27) % (1 << 27)
    return pow(pow(TS_G, k, R_MOD) * h, 2, R_MOD)


def sqrt_edge_values():
    """plain values a (the op takes them in Montgomery form, both representatives)"""
    d4 = lambda d0, d1, d2, d3: d0 | (d1 << 7) | (d2 << 14) | (d3 << 21)      # noqa: E731
    logs = SQRT_SINGLE_DIGIT_LOGS + SQRT_STRIP_LOGS + [(1 << 28) - 2, d4(0, 127, 0, 127), d4(126, 0, 127, 0), d4(126, 127, 127, 127), d4(2, 0, 0, 127)]
    logs = dedup(logs)
    out = []
    for i, e in enumerate(logs):
        h = pow(3 + i, 1 << 28, R_MOD)
        a = sqrt_value_of_log(e, h)
        out += [a, a * TS_G % R_MOD]                    # and the same times G: an odd log, a non-residue
    nonres = 5
    return out + [1, R_MOD - 1, 4, nonres, 2, 3, HALF, HALF + 1]


def sqrt_logs_present(items, logs=SQRT_SINGLE_DIGIT_LOGS):
    """which of `logs` (default: the 448 single-digit logs) the sqrt items reach, from the inputs alone: a^s looked up among
    the G^e"""
    table = {pow(TS_G, e, R_MOD): e for e in logs}
    found = set()
    for (a,) in items:
        e = table.get(pow(lval(a) * RINV % R_MOD, TS_S, R_MOD))
        if e is not None:
            found.add(e)
    return found


# ---- edge sets -----------------------------------------------------------------------------------------------------------
def both_reps(v):
    """the canonical and the [r, 2r) representative of v mod r, as N-form limbs"""
    v %= R_MOD
    return [nform(v), nform(v + R_MOD)]


def _edges_add():
    few = [(0,) * 9, (ONES30,) * 9, (ONES30 - 1,) * 9, nform(R_MOD), nform(16 * R_MOD - 1), (M29,) * 8 + (13 * TOP_R - 3,), lazy(13 * R_MOD)]
    pairs = []
    for a in any_class():
        for b in few:
            pairs += [(a, b), (b, a)]
    return dedup(pairs)


def _edges_reduce_weak():
    out = [l for l in nform_class() if l[8] < 1 << 26]
    for k in range(22):
        for d in (-1, 0, 1):
            t = TOP_DIV * k + d
            if 0 <= t < 1 << 26:
                out += [(0,) * 8 + (t,), (M29,) * 8 + (t,)]
    out += [(0,) * 8 + ((1 << 26) - 1,), (M29,) * 8 + ((1 << 26) - 1,)]
    return [(l,) for l in dedup(out)]


def _edges_eq():
    bmax = (M29,) * 8 + (C4[8],)
    bs = [nform(v) for v in (0, 1, R_MOD - 1, R_MOD, R_MOD + 1, 2 * R_MOD - 1, 3 * R_MOD + 7)] + [bmax, (0,) * 8 + (C4[8],)]
    rnd = random.Random(0xE9)
    out = []
    for b in bs:
        vb = lval(b)
        for k in range(-4, 13):
            for d in (-1, 0, 1):
                va = vb + k * R_MOD + d
                if 0 <= va < 12 * R_MOD:
                    out += [(nform(va), b), (lazy(va, rnd), b)]
        out += [(nform(12 * R_MOD - 1), b), (lazy(12 * R_MOD - 1), b), ((0,) * 9, b)]
    return dedup(out)


def _edges_from_mont():
    v = [0, R_MOD, R1, R1 + R_MOD, mont(R_MOD - 1), mont(R_MOD - 1) + R_MOD, 1, R_MOD - 1, R_MOD + 1, 2 * R_MOD - 1, mont(2), mont(HALF)]
    return dedup([(nform(x),) for x in v] + [(l,) for l in nform_class() if lval(l) < 2 * R_MOD])


def _edges_gt_halfq():
    v = [0, 1, HALF - 1, HALF, HALF + 1, HALF + 2, R_MOD - 1, R_MOD - 2]
    v += [(1 << (29 * i)) + d for i in range(1, 9) for d in (-1, 0, 1)]
    v += [HALF ^ (1 << (29 * i)) for i in range(9)] + [HALF + (1 << (29 * i)) for i in range(8)] + [HALF - (1 << (29 * i)) for i in range(8)]
    return [(nform(x),) for x in dedup(v) if 0 <= x < R_MOD]


def _edges_sqrt():
    out = [((0,) * 9,), (nform(R_MOD),)]                       # zero in both representatives, as raw limbs
    for a in sqrt_edge_values():
        out += [(l,) for l in both_reps(mont(a))]
    return dedup(out)


def curve_edge_points():
    pts = [(0, 1), (0, R_MOD - 1)] + golden_points("torsion_points") + [B8]
    out = list(pts)
    for x, y in pts:
        out += [((x + 1) % R_MOD, y), ((x - 1) % R_MOD, y), (x, (y + 1) % R_MOD), (x, (y - 1) % R_MOD)]
    return dedup(out + [(0, 0)])


def _edges_on_curve():
    out = []
    for x, y in curve_edge_points():
        out += [(a, b) for a in both_reps(mont(x)) for b in both_reps(mont(y))]
    return dedup(out)


COMPRESS_X = [0, 1, HALF, HALF + 1, R_MOD - 1, R_MOD, R_MOD + HALF, R_MOD + HALF + 1, 2 * R_MOD, (1 << 256) - 1]
COMPRESS_Y = [0, 1, R_MOD - 1, R_MOD, 1 << 255, (1 << 256) - 1]


def compress_edge_values():
    """(x, y) as 256-bit integers: the sign threshold in both representatives crossed with y at the reduction edges, and the
    curve's own edge points"""
    return dedup([(x, y) for x in COMPRESS_X for y in COMPRESS_Y] + curve_edge_points())


def decompress_edge_values():
    ys = [0, 1, 2, R_MOD - 2, R_MOD - 1, R_MOD, R_MOD + 1, (1 << 255) - 1]
    ys += y_of_x(HALF - 1)                               # the largest x without the sign bit, the smallest with it
    ys += [y for _, y in golden_points("torsion_points")] + [B8[1]]
    v = [y | (s << 255) for y in ys for s in (0, 1)]
    return dedup(v + golden_decompress_inputs())


assert not y_of_x(HALF) and len(y_of_x(HALF - 1)) == 2       # (r-1)/2 is no x of the curve, (r-1)/2 - 1 is


def edge_set(op):
    """the explicit inputs of one op"""
    if op in ("add", "add_lazy"):
        return _edges_add()
    if op == "dbl":
        return [(a,) for a in any_class()]
    if op in ("sub", "sub_lazy"):
        return cross_sub(subtrahends(C4), C4)
    if op == "neg":
        return [(b,) for b in subtrahends(C4)]
    if op == "sub8":
        return cross_sub(subtrahends(C8), C8)
    if op == "sub8_of_lazy":
        return cross_sub(lazy_subtrahends(), K8)
    if op == "reduce_weak":
        return _edges_reduce_weak()
    if op in ("canon", "is_zero"):
        return [(l,) for l in nform_class() if lval(l) < 16 * R_MOD]
    if op == "eq":
        return _edges_eq()
    if op in ("from_words", "to_mont", "words_ge_r", "words_gt_r"):
        return [(words(v),) for v in word_values()]
    if op == "to_words":
        return [(nform(v),) for v in word_values()]
    if op == "from_mont":
        return _edges_from_mont()
    if op == "gt_halfq":
        return _edges_gt_halfq()
    if op == "sqrt":
        return _edges_sqrt()
    if op == "on_curve":
        return _edges_on_curve()
    if op == "decompress":
        return [(words(v),) for v in decompress_edge_values()]
    if op == "compress":
        return [(words(x), words(y)) for x, y in compress_edge_values()]
    raise ValueError(op)


# ---- seeded random inputs, inside the domain by construction ---------------------------------------------------------------
def _rand_any(rnd, bound=13 * R_MOD):
    """limbs < 2^30: raw 30-bit limbs, or the N-form or lazy limbs of a value below `bound`"""
    k = rnd.randrange(3)
    if k == 0:
        return tuple(rnd.randrange(1 << 30) for _ in range(9))
    v = rnd.randrange(bound)
    return nform(v) if k == 1 else lazy(v, rnd)


def _rand_sub_b(rnd, C):
    if C is K8:
        if rnd.randrange(2):
            return tuple(rnd.randrange(c + 1) for c in C)
        return lazy(rnd.randrange((C[8] + 1) << 232), rnd)
    return nform(rnd.randrange((C[8] + 1) << 232))


_CURVE_POOL = []


def curve_pool():
    """512 points of the curve: B8, 2 B8, ... (computed once)"""
    if not _CURVE_POOL:
        p = B8
        for _ in range(512):
            _CURVE_POOL.append(p)
            p = point_add(p, B8)
    return _CURVE_POOL


def _rand_rep(rnd, v):
    return nform(v % R_MOD + (R_MOD if rnd.randrange(2) else 0))


def random_set(op, rnd, n):
    """n seeded random items for the op"""
    if op in ("add", "add_lazy"):
        return [(_rand_any(rnd), _rand_any(rnd)) for _ in range(n)]
    if op == "dbl":
        return [(_rand_any(rnd),) for _ in range(n)]
    if op in ("sub", "sub_lazy"):
        return [(_rand_any(rnd), _rand_sub_b(rnd, C4)) for _ in range(n)]
    if op == "neg":
        return [(_rand_sub_b(rnd, C4),) for _ in range(n)]
    if op == "sub8":
        return [(_rand_any(rnd), _rand_sub_b(rnd, C8)) for _ in range(n)]
    if op == "sub8_of_lazy":
        return [(_rand_any(rnd), _rand_sub_b(rnd, K8)) for _ in range(n)]
    if op == "reduce_weak":
        return [(nform(rnd.randrange(1 << 258)),) for _ in range(n)]
    if op in ("canon", "is_zero"):
        return _random_canon(rnd, n)
    if op == "eq":
        out = []
        for _ in range(n):
            b = rnd.randrange((C4[8] + 1) << 232)
            kmax = (12 * R_MOD - 1 - b) // R_MOD
            kmin = -(b // R_MOD)
            if rnd.randrange(2):
                a = b + rnd.randrange(kmin, kmax + 1) * R_MOD          # congruent
                a += rnd.choice((0, 0, 1)) if a + 1 < 12 * R_MOD else 0
            else:
                a = rnd.randrange(12 * R_MOD)
            out.append((lazy(a, rnd) if rnd.randrange(2) else nform(a), nform(b)))
        return out
    if op in ("from_words", "to_mont", "words_ge_r", "words_gt_r"):
        out = []
        for _ in range(n):
            v = rnd.getrandbits(256) if rnd.randrange(2) else rnd.getrandbits(rnd.randint(1, 256))
            if op.startswith("words_") and rnd.randrange(4) == 0:          # equal to r in the high words, random below
                j = rnd.randrange(8)
                v = (R_MOD >> (32 * j) << (32 * j)) | rnd.getrandbits(32 * j)
            out.append((words(v),))
        return out
    if op == "to_words":
        return [(nform(rnd.getrandbits(256) if rnd.randrange(2) else rnd.getrandbits(rnd.randint(1, 256))),) for _ in range(n)]
    if op == "from_mont":
        return [(nform(rnd.randrange(2 * R_MOD)),) for _ in range(n)]
    if op == "gt_halfq":
        return [(nform(rnd.randrange(R_MOD) if rnd.randrange(2) else HALF - (1 << 20) + rnd.randrange(1 << 21)),) for _ in range(n)]
    if op == "sqrt":
        out = []
        for _ in range(n):
            if rnd.randrange(4) == 0:
                x = rnd.randrange(R_MOD)
                out.append((_rand_rep(rnd, mont(x * x)),))
            else:
                out.append((nform(rnd.randrange(2 * R_MOD)),))
        return out
    if op == "on_curve":
        pool, out = curve_pool(), []
        for _ in range(n):
            k = rnd.randrange(4)
            if k == 0:
                x, y = rnd.randrange(R_MOD), rnd.randrange(R_MOD)
            else:
                x, y = pool[rnd.randrange(len(pool))]
                x = x if rnd.randrange(2) else R_MOD - x
                y = y if rnd.randrange(2) else R_MOD - y
                if k == 3:
                    if rnd.randrange(2):
                        x = (x + rnd.choice((-1, 1))) % R_MOD
                    else:
                        y = (y + rnd.choice((-1, 1))) % R_MOD
            out.append((_rand_rep(rnd, mont(x)), _rand_rep(rnd, mont(y))))
        return out
    if op == "decompress":
        pool, out = curve_pool(), []
        for _ in range(n):
            k = rnd.randrange(4)
            if k == 0:
                v = rnd.getrandbits(256)
            elif k == 1:
                v = rnd.randrange(R_MOD) | (rnd.getrandbits(1) << 255)
            else:
                x, y = pool[rnd.randrange(len(pool))]
                v = (y if rnd.randrange(2) else R_MOD - y) | (rnd.getrandbits(1) << 255)
            out.append((words(v),))
        return out
    if op == "compress":
        out = []
        for _ in range(n):
            x = rnd.getrandbits(256) if rnd.randrange(2) else rnd.randrange(3) * R_MOD + HALF - 2 + rnd.randrange(5)
            y = rnd.getrandbits(256) if rnd.randrange(2) else rnd.randrange(R_MOD)
            out.append((words(x), words(y)))
        return out
    raise ValueError(op)


def _random_canon(rnd, n):
    """N-form values below 16 r, one in eight within 2 of a multiple of r"""
    out = []
    for _ in range(n):
        if rnd.randrange(8) == 0:
            v = min(max(rnd.randrange(17) * R_MOD + rnd.randrange(-2, 3), 0), 16 * R_MOD - 1)
        else:
            v = rnd.randrange(16 * R_MOD)
        out.append((nform(v),))
    return out


# ---- domains (what the op's contract admits; the self-tests hold every edge and random item against them) -------------------
def in_domain(op, item):
    a = item[0]
    b = item[1] if len(item) > 1 else None
    wa, wb, _ = WIDTHS[op]
    if len(a) != wa or (b is None) != (wb == 0) or (b is not None and len(b) != wb):
        return False
    lt30 = lambda l: all(0 <= x < 1 << 30 for x in l)                        # noqa: E731
    isn = lambda l: all(0 <= x <= M29 for x in l[:8]) and 0 <= l[8] < 1 << 32    # noqa: E731
    le = lambda l, C: all(0 <= x <= c for x, c in zip(l, C))                  # noqa: E731
    w32 = lambda w: all(0 <= x < 1 << 32 for x in w)                         # noqa: E731
    if op in ("add", "add_lazy"):
        return lt30(a) and lt30(b)
    if op == "dbl":
        return lt30(a)
    if op in ("sub", "sub_lazy"):
        return lt30(a) and le(b, C4)          # N-form b with top limb <= C4[8], and C4 itself limb for limb
    if op == "neg":
        return le(a, C4)
    if op == "sub8":
        return lt30(a) and le(b, C8)
    if op == "sub8_of_lazy":
        return lt30(a) and le(b, K8)
    if op == "reduce_weak":
        return isn(a) and a[8] < 1 << 26
    if op in ("canon", "is_zero"):
        return isn(a) and lval(a) < 16 * R_MOD
    if op == "eq":
        return lt30(a) and lval(a) < 12 * R_MOD and isn(b) and b[8] <= C4[8]
    if op in ("from_words", "to_mont", "words_ge_r", "words_gt_r", "decompress"):
        return w32(a)
    if op == "compress":
        return w32(a) and w32(b)
    if op == "to_words":
        return isn(a) and lval(a) < 1 << 256
    if op in ("from_mont", "sqrt"):
        return isn(a) and lval(a) < 2 * R_MOD
    if op == "gt_halfq":
        return isn(a) and lval(a) < R_MOD
    if op == "on_curve":
        return isn(a) and isn(b) and lval(a) < 2 * R_MOD and lval(b) < 2 * R_MOD
    raise ValueError(op)


# ---- records and checks --------------------------------------------------------------------------------------------------
def records(op, items):
    """(a, b) uint32 records for `items`; b is None for the ops with one operand"""
    wa, wb, _ = WIDTHS[op]
    a = np.array([it[0] for it in items], dtype=np.uint64).astype(np.uint32).reshape(len(items), wa)
    b = np.array([it[1] for it in items], dtype=np.uint64).astype(np.uint32).reshape(len(items), wb) if wb else None
    return a, b


def items_of(op, a, b):
    """the inverse of records"""
    if b is None:
        return [(tuple(int(x) for x in r),) for r in a]
    return [(tuple(int(x) for x in r), tuple(int(x) for x in s)) for r, s in zip(a, b)]


def _low_ok(out):
    """per row: limbs 0..7 < 2^29"""
    return (np.asarray(out)[:, :8] <= M29).all(axis=1)


def check(op, items, out):
    """indices (with a reason) where the op's output is not what the integers say"""
    a, b = records(op, items)
    out = np.asarray(out, dtype=np.uint32)
    n = len(items)
    assert out.shape == (n, WIDTHS[op][2]), (op, out.shape)
    bad = []
    limbs_in = WIDTHS[op][0] == 9
    A = vals_of_limbs(a) if limbs_in else vals_of_words(a)
    B = None if b is None else (vals_of_limbs(b) if WIDTHS[op][1] == 9 else vals_of_words(b))
    if op in ("add", "dbl", "sub", "neg", "sub8", "sub8_of_lazy"):
        K = dict(add=0, dbl=0, sub=4, neg=4, sub8=8, sub8_of_lazy=8)[op] * R_MOD
        O, low = vals_of_limbs(out), _low_ok(out)
        for i in range(n):
            want = 2 * A[i] if op == "dbl" else K - A[i] if op == "neg" else A[i] + B[i] if op == "add" else A[i] + K - B[i]
            if O[i] != want or not low[i]:
                bad.append((i, "value %d, want %d%s" % (O[i], want, "" if low[i] else "; a limb above 29 bits")))
    elif op in ("add_lazy", "sub_lazy"):
        want = a.astype(np.int64) + b.astype(np.int64) if op == "add_lazy" else a.astype(np.int64) + np.array(C4, np.int64) - b.astype(np.int64)
        for i in np.nonzero((want != out.astype(np.int64)).any(axis=1))[0]:
            bad.append((int(i), "limbs %s, want %s" % (out[i].tolist(), want[i].tolist())))
    elif op == "reduce_weak":
        O, low = vals_of_limbs(out), _low_ok(out)
        for i in range(n):
            q = int(a[i, 8]) // TOP_DIV
            ok = (low[i] and out[i, 8] < 1 << 26 and (O[i] - A[i]) % R_MOD == 0 and O[i] <= A[i]
                  and O[i] < R_MOD + ((q + 1) << 232) and O[i] < 2 * R_MOD)
            if not ok:
                bad.append((i, "value %d from %d (q = %d)" % (O[i], A[i], q)))
    elif op == "canon":
        for i in range(n):
            if tuple(int(x) for x in out[i]) != nform(A[i] % R_MOD):
                bad.append((i, "limbs %s, want %d mod r" % (out[i].tolist(), A[i])))
    elif op in ("is_zero", "eq", "gt_halfq", "words_ge_r", "words_gt_r", "on_curve"):
        for i in range(n):
            if op == "is_zero":
                want = A[i] % R_MOD == 0
            elif op == "eq":
                want = (A[i] - B[i]) % R_MOD == 0
            elif op == "gt_halfq":
                want = A[i] > HALF
            elif op == "words_ge_r":
                want = A[i] >= R_MOD
            elif op == "words_gt_r":
                want = A[i] > R_MOD
            else:
                want = on_curve(A[i] * RINV % R_MOD, B[i] * RINV % R_MOD)
            if int(out[i, 0]) != int(want):
                bad.append((i, "verdict %d, want %d" % (out[i, 0], want)))
    elif op == "from_words":
        for i in range(n):
            if tuple(int(x) for x in out[i]) != nform(A[i]):
                bad.append((i, "limbs %s of %d" % (out[i].tolist(), A[i])))
    elif op == "to_words":
        for i, o in enumerate(vals_of_words(out)):
            if o != A[i]:
                bad.append((i, "words %d of %d" % (o, A[i])))
    elif op == "to_mont":
        O, low = vals_of_limbs(out), _low_ok(out)
        for i in range(n):
            if not low[i] or O[i] >= 2 * R_MOD or (O[i] - A[i] * RADIX) % R_MOD:
                bad.append((i, "value %d of %d" % (O[i], A[i])))
    elif op == "from_mont":
        for i, o in enumerate(vals_of_words(out)):
            if o != A[i] * RINV % R_MOD:
                bad.append((i, "words %d of %d" % (o, A[i])))
    elif op == "sqrt":
        O, low = vals_of_limbs(out[:, 1:]), _low_ok(out[:, 1:])
        for i in range(n):
            plain = A[i] * RINV % R_MOD
            flag = int(out[i, 0])
            if flag == 1:          # a root proves the residue: root^2 == a, in plain values
                x = O[i] * RINV % R_MOD
                ok = plain != 0 and low[i] and O[i] < 2 * R_MOD and x * x % R_MOD == plain
            else:
                ok = flag == 0 and (plain == 0 or not is_residue(plain))
            if not ok:
                bad.append((i, "flag %d root %d of %d" % (flag, O[i], A[i])))
    elif op == "decompress":
        X, Y = vals_of_words(out[:, 1:9]), vals_of_words(out[:, 9:17])
        for i in range(n):
            inr, x2 = decompress_x2(A[i])
            flag = int(out[i, 0])
            if flag == 1:          # the root proves the residue: x^2 == x2 with the sign the bit asks for pins x
                ok = (inr and x2 != 0 and Y[i] == A[i] & ((1 << 255) - 1) and X[i] < R_MOD and X[i] * X[i] % R_MOD == x2
                      and (X[i] > HALF) == bool(A[i] >> 255))
            else:
                ok = flag == 0 and X[i] == 0 and Y[i] == 0 and (not inr or x2 == 0 or not is_residue(x2))
            if not ok:
                bad.append((i, "flag %d x %d y %d of %d" % (flag, X[i], Y[i], A[i])))
    elif op == "compress":
        for i, o in enumerate(vals_of_words(out)):
            if o != compress_model(A[i], B[i]):
                bad.append((i, "%d of (%d, %d)" % (o, A[i], B[i])))
    else:
        raise ValueError(op)
    return bad


def cpu_run(lib, op, a, b):
    """the op on the CPU harness (tests/emul/emul_field_ops.cpp: the g++ build of field_ops.hpp) -> (n, out words) uint32"""
    import ctypes
    n = a.shape[0]
    wa, wb, wo = WIDTHS[op]
    assert a.shape == (n, wa) and ((b is None and wb == 0) or b.shape == (n, wb))
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = None if b is None else np.ascontiguousarray(b, dtype=np.uint32)
    out = np.zeros((n, wo), dtype=np.uint32)
    vp = ctypes.c_void_p

    def part(lo, hi):
        return lib.emul_field_op(ctypes.c_int(OPS[op]), a[lo:hi].ctypes.data_as(vp), None if b is None else b[lo:hi].ctypes.data_as(vp),
                                 out[lo:hi].ctypes.data_as(vp), ctypes.c_size_t(hi - lo))
    # the items are independent and the library keeps no state: slices on a few threads (ctypes releases the GIL)
    nthr = max(1, min(8, os.cpu_count() or 1, n // 1024))
    cuts = [n * k // nthr for k in range(nthr + 1)]
    if nthr == 1:
        rcs = [part(0, n)]
    else:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(nthr) as ex:
            rcs = list(ex.map(lambda k: part(cuts[k], cuts[k + 1]), range(nthr)))
    assert all(rc == 0 for rc in rcs)
    return out
