"""Plain-integer model and directed input sets for the group-law layer: the extended-coordinate formulas and conversions of
csrc/curve.hpp (ext_madd, ext_add_pn, ext_dbl, ext_to_pniels, pniels_cneg, ext_from_ref_affine, ref_add) and the per-lane table,
ladder and fixed-table code of csrc/bjj_device.hpp (niels_cneg_lazy, vb_build_table, vb_table_load, pniels_to_ext,
vb_mul_windowed, ref_mul_scalar, var_base_item, niels_from_affine, niels_lift, ext_equals_niels, fixed_table_entry,
fixed_table_chain, fixed_table_check_slot).  Shared by tests/test_curve_ops_host.py (the g++ build of
tests/devfuzz/curve_ops.hpp with the bound assertions live) and tests/test_gpu_curve_ops.py (the same dispatcher on the device,
tests/devfuzz/curve.hip).  A plain helper module in the style of tests/field_ref.py: no fixtures, no pytest hooks, nothing
imported from oracle/ (the host test passes the Python oracle's proj_add / proj_affine / mul_scalar into `check` as `ref`; without
it the model's own statement of those three is used, and the host test holds the two against each other).

Two curves: the reference curve A x^2 + y^2 = 1 + D x^2 y^2 and the a' = -1 curve -x'^2 + y^2 = 1 + D' x'^2 y^2 with x' = F x,
F = the smaller square root of -A, D' = -D / A.  Every constant is derived here from r, A, D and B8, not read from the header.
An item is a tuple of one or two raw vectors (tuples of ints): limbs of 29 bits (value = sum v[i] 2^(29 i)) per field element,
then flag or scalar words.  Points with a known multiple of the generator G0 = B8 + T8 of the whole group (order 8 l) are kept
in a table, so that the expected result of a 254-bit ladder costs 32 additions of precomputed points."""
import ctypes
import os
import random

import numpy as np

import field_ref as fr
from field_ref import R_MOD, RADIX, RINV, R1, M29, nform, lval, mont, dedup, vals_of_limbs, vals_of_words, words

A_REF, D_REF, B8 = fr.A_REF, fr.D_REF, fr.B8
SUBORDER = 2736030358979909402780800718157159386076813972158567259200215660948447373041       # l
ORDER = 8 * SUBORDER
_f = fr.modsqrt(-A_REF % R_MOD)
F = min(_f, R_MOD - _f)                                    # x' = F x
FINV = pow(F, -1, R_MOD)
DP = -D_REF * pow(A_REF, -1, R_MOD) % R_MOD                # D'
NINV = -pow(R_MOD, -1, RADIX) % RADIX                      # -r^-1 mod 2^261
C4R = 4 * R_MOD
TOP4 = fr.C4[8]                                            # the largest top limb fr_sub / fr_sub_lazy take in a subtrahend

OPS = dict(madd_t=0, madd=1, addpn_t=2, addpn=3, dbl_t=4, dbl=5, window=6, to_pniels=7, pn2ext_t=8, pn2ext=9, lift_t=10, lift=11,
           eq_niels=12, nfa_t=13, nfa=14, from_ref=15, ref_add=16, ref_mul8=17, ref_mul2=18, var_base=19, table=20, table_affine=21,
           mulw64=22, mulw64_t=23, mulw2=24, mulw2_t=25, mulw1=26, mulw1_t=27, fixed_entry=28, fixed_chain=29, fixed_flip=30)
FT_NWIN, FT_SLOTS = 3, 27                                  # the fixed table of the chain ops: W = 4, 3 windows of 9 slots
# record widths in words of tests/devfuzz/curve_ops.hpp: a, b, out, per-item scratch
WIDTHS = dict(madd_t=(36, 28, 36, 0), madd=(36, 28, 36, 0), addpn_t=(36, 37, 36, 0), addpn=(36, 37, 36, 0), dbl_t=(36, 0, 36, 0),
              dbl=(36, 0, 36, 0), window=(36, 38, 36, 0), to_pniels=(36, 0, 36, 0), pn2ext_t=(37, 0, 36, 0), pn2ext=(37, 0, 36, 0),
              lift_t=(27, 0, 36, 0), lift=(27, 0, 36, 0), eq_niels=(36, 27, 1, 0), nfa_t=(9, 9, 27, 0), nfa=(9, 9, 27, 0),
              from_ref=(9, 9, 36, 0), ref_add=(27, 27, 27, 0), ref_mul8=(18, 8, 18, 0), ref_mul2=(18, 2, 18, 0), var_base=(18, 8, 36, 324),
              table=(36, 0, 324, 324), table_affine=(36, 0, 324, 324), mulw64=(36, 8, 36, 324), mulw64_t=(36, 8, 36, 324),
              mulw2=(36, 8, 36, 324), mulw2_t=(36, 8, 36, 324), mulw1=(36, 8, 36, 324), mulw1_t=(36, 8, 36, 324),
              fixed_entry=(3, 0, 27, 0), fixed_chain=(1, 0, FT_SLOTS * 28, 960), fixed_flip=(4, 0, 2, 960))
MULW = dict(mulw64=(64, False), mulw64_t=(64, True), mulw2=(2, False), mulw2_t=(2, True), mulw1=(1, False), mulw1_t=(1, True))


# ---- the two curves in plain integers ---------------------------------------------------------------------------------------
def inv(v):
    return pow(v, -1, R_MOD)


def on_ref(p):
    return fr.on_curve(*p)


def on_m1(p):
    x, y = p
    return (-x * x + y * y - 1 - DP * x * x * y * y) % R_MOD == 0


def to_m1(p):
    return (F * p[0] % R_MOD, p[1])


def from_m1(p):
    return (FINV * p[0] % R_MOD, p[1])


def add_m1(p, q):
    """the affine group law of the a' = -1 curve"""
    (x1, y1), (x2, y2) = p, q
    t = DP * x1 * x2 * y1 * y2 % R_MOD
    return ((x1 * y2 + y1 * x2) * inv(1 + t) % R_MOD, (y1 * y2 + x1 * x2) * inv(1 - t) % R_MOD)


def neg(p):
    return (-p[0] % R_MOD, p[1])


def smul_m1(p, n):
    """n p by double-and-add (small n, or to pin the table-driven form)"""
    acc, e = (0, 1), p
    while n:
        if n & 1:
            acc = add_m1(acc, e)
        e = add_m1(e, e)
        n >>= 1
    return acc


def padd(P, Q):
    """the same law on projective triples (X : Y : Z), without an inversion"""
    X1, Y1, Z1 = P
    X2, Y2, Z2 = Q
    a, b, c = X1 * X2 % R_MOD, Y1 * Y2 % R_MOD, Z1 * Z2 % R_MOD
    e, cc = DP * a * b % R_MOD, c * c % R_MOD
    nx, dx, ny, dy = (X1 * Y2 + Y1 * X2) * c % R_MOD, (cc + e) % R_MOD, (b + a) * c % R_MOD, (cc - e) % R_MOD
    return (nx * dy % R_MOD, ny * dx % R_MOD, dx * dy % R_MOD)


def peq(P, Q):
    """equal as projective points, both with Z != 0"""
    return (P[2] % R_MOD != 0 and Q[2] % R_MOD != 0 and (P[0] * Q[2] - Q[0] * P[2]) % R_MOD == 0
            and (P[1] * Q[2] - Q[1] * P[2]) % R_MOD == 0)


def proj_add(p, q):
    """the reference's projective addition (add-2008-bbjlp on the reference curve), coordinate by coordinate"""
    (x1, y1, z1), (x2, y2, z2) = p, q
    a = z1 * z2 % R_MOD
    b, c, d = a * a % R_MOD, x1 * x2 % R_MOD, y1 * y2 % R_MOD
    e = D_REF * c * d % R_MOD
    f, g = (b - e) % R_MOD, (b + e) % R_MOD
    x3 = a * f * ((x1 + y1) * (x2 + y2) - c - d) % R_MOD
    y3 = a * g * (d - A_REF * c) % R_MOD
    return (x3, y3, f * g % R_MOD)


def proj_affine(p):
    x, y, z = p
    if z % R_MOD == 0:
        return (0, 0)
    zi = inv(z)
    return (x * zi % R_MOD, y * zi % R_MOD)


def mul_scalar(pt, n):
    """the reference's LSB-first double-and-add with the unified addition, one affine() at the end"""
    r, e = (0, 1, 1), (pt[0] % R_MOD, pt[1] % R_MOD, 1)
    for i in range(n.bit_length()):
        if (n >> i) & 1:
            r = proj_add(r, e)
        e = proj_add(e, e)
    return proj_affine(r)


class _Own:
    proj_add, proj_affine, mul_scalar = staticmethod(proj_add), staticmethod(proj_affine), staticmethod(mul_scalar)


# ---- the whole group through one generator -------------------------------------------------------------------------------------
TORSION_REF = fr.golden_points("torsion_points")           # j T8, j = 0 .. 7, on the reference curve
T8 = to_m1(TORSION_REF[1])
B8M = to_m1(B8)
G0 = add_m1(B8M, T8)                                       # order lcm(l, 8) = 8 l
LOG_B8 = 8 * pow(8, -1, SUBORDER) % ORDER                  # B8 = LOG_B8 G0: 1 mod l, 0 mod 8
LOG_T8 = SUBORDER * pow(SUBORDER, -1, 8) % ORDER           # T8 = LOG_T8 G0: 0 mod l, 1 mod 8
_G0_TABLE = []
_LOGS = {}


def g0_table():
    """d 256^w G0 for w < 32, d < 256, as (y - x, y + x, 2 D' x y) of the affine point (built once)"""
    if not _G0_TABLE:
        base = G0
        for _ in range(32):
            row = [(0, 1)]
            for _d in range(255):
                row.append(add_m1(row[-1], base))
            base = add_m1(row[-1], base)
            _G0_TABLE.append([((y - x) % R_MOD, (y + x) % R_MOD, 2 * DP * x * y % R_MOD) for x, y in row])
    return _G0_TABLE


def g0_mul(k):
    """k G0 as a projective triple"""
    k %= ORDER
    tab = g0_table()
    X, Y, Z, T = 0, 1, 1, 0
    for w in range(32):
        d = (k >> (8 * w)) & 255
        if d:                                                # the mixed addition in extended coordinates: 7 products
            ymx, ypx, t2d = tab[w][d]
            a, b, c, dd = (Y - X) * ymx % R_MOD, (Y + X) * ypx % R_MOD, T * t2d % R_MOD, 2 * Z
            e, f, g, h = b - a, dd - c, dd + c, b + a
            X, Y, Z, T = e * f % R_MOD, g * h % R_MOD, f * g % R_MOD, e * h % R_MOD
    return (X, Y, Z)


def g0_point(k):
    X, Y, Z = g0_mul(k)
    zi = inv(Z)
    p = (X * zi % R_MOD, Y * zi % R_MOD)
    _LOGS[p] = k % ORDER
    return p


def log_of(p):
    """k with p = k G0 for the points this module made (edge points and the random pool), else None"""
    edge_points()
    pool()
    return _LOGS.get(p)


_EDGE, _POOL = [], []
POOL_SIZE = 48


def edge_points():
    """the directed points, affine on the a' = -1 curve: the eight torsion points j T8 (the identity, (0, -1), the two points with
    y = 0), B8, -B8, 2 B8, (l - 1) B8 (= -B8: kept apart only as a scalar, see edge_scalars), B8 + T and -(B8 + T) for T of
    order 2, 4 and 8, two seeded points of the whole group"""
    if not _EDGE:
        ks = [j * LOG_T8 for j in range(8)] + [LOG_B8, -LOG_B8, 2 * LOG_B8, (SUBORDER - 1) * LOG_B8]
        for j in (4, 2, 1):                                  # j T8 has order 2, 4, 8
            ks += [LOG_B8 + j * LOG_T8, -(LOG_B8 + j * LOG_T8)]
        rnd = random.Random(0xC0B8)
        ks += [rnd.randrange(ORDER) | 1, rnd.randrange(ORDER) | 1]     # odd: generators of the whole group
        _EDGE.extend(dedup(g0_point(k) for k in ks))
    return _EDGE


def pool():
    """seeded points of the whole group with their logs: what the random sets draw from"""
    if not _POOL:
        rnd = random.Random(0xB8B8)
        for _ in range(POOL_SIZE):
            p = g0_point(rnd.randrange(ORDER))
            _POOL.extend([p, neg(p)])
            _LOGS[neg(p)] = (-_LOGS[p]) % ORDER
    return _POOL


def smul_known(p, n):
    """n p as a projective triple: through the generator's table when p's log is known"""
    k = log_of(p)
    if k is None:
        x, y = smul_m1(p, n % ORDER)
        return (x, y, 1)
    return g0_mul(k * n)


# ---- representations ----------------------------------------------------------------------------------------------------
def reps(v):
    """the canonical and the [r, 2r) Montgomery representative of the plain value v, as N-form limbs"""
    m = mont(v)
    return [nform(m), nform(m + R_MOD)]


def ext_coords(p, z):
    x, y = p
    return (x * z % R_MOD, y * z % R_MOD, z % R_MOD, x * y * z % R_MOD)


def edge_zs(p):
    """z = 1, r - 1, a seeded z, and for each coordinate that is not zero the z that makes that coordinate's Montgomery
    representative exactly 1 and exactly r - 1"""
    rnd = random.Random(0x2E + p[0] % 1000003)
    zs = [1, R_MOD - 1, rnd.randrange(2, R_MOD)]
    for c in ext_coords(p, 1):
        if c:
            for target in (1, R_MOD - 1):                   # c z 2^261 == target
                zs.append(target * inv(c * RADIX) % R_MOD)
    return dedup(zs)


def ext_reps(p, every=True, rnd=None):
    """extended representations (36 limbs) of the affine point p: every edge z, each coordinate canonical or + r -- all 16
    combinations when `every`, else all canonical, all + r, and two seeded mixtures"""
    out = []
    for z in edge_zs(p):
        c = ext_coords(p, z)
        masks = range(16) if every else (0, 15, rnd.randrange(1, 15), rnd.randrange(1, 15))
        for m in masks:
            out.append(sum((reps(c[i])[(m >> i) & 1] for i in range(4)), ()))
    return dedup(out)


def niels_coords(q):
    x, y = q
    return ((y - x) % R_MOD, (y + x) % R_MOD, 2 * DP * x * y % R_MOD)


def niels_reps(q):
    """Niels entries (27 limbs) of q: every component canonical or + r"""
    c = niels_coords(q)
    return [sum((reps(c[i])[(m >> i) & 1] for i in range(3)), ()) for m in range(8)]


def pniels_coords(q, z):
    x, y = q
    return ((y - x) * z % R_MOD, (y + x) * z % R_MOD, 2 * DP * x * y * z % R_MOD, 2 * z % R_MOD)


def pniels_reps(q, z, masks=range(16)):
    c = pniels_coords(q, z)
    return [sum((reps(c[i])[(m >> i) & 1] for i in range(4)), ()) for m in masks]


def mmul(a, b):
    """fr_mul on integers, representative for representative: (a b + m r) / 2^261 with m = -a b / r mod 2^261"""
    t = a * b
    return (t + (t * NINV % RADIX) * R_MOD) >> 261


def to_pniels_model(e):
    """ext_to_pniels on 36 limbs -> 36 limbs, limb for limb: Y + 4r - X, Y + X, T (2 D') by the Montgomery product, 2 Z"""
    X, Y, Z, T = (lval(e[9 * i:9 * i + 9]) for i in range(4))
    return nform(Y + C4R - X) + nform(Y + X) + nform(mmul(T, mont(2 * DP))) + nform(2 * Z)


def table_model(e, affine_base, layout):
    """vb_build_table on 36 limbs -> the integer values (ymx, ypx, t2d, z2) of the entries 1 .. 8, value for value: k P =
    (k - 1) P + P by ext_madd (affine_base) or ext_add_pn on the first entry, each sum through ext_to_pniels; the packed layout
    stores ymx weakly reduced (less floor(top limb / 3171407) r)"""
    def pn(X, Y, Z, T):
        return (Y + C4R - X, Y + X, mmul(T, mont(2 * DP)), 2 * Z)
    cur = tuple(lval(c) for c in split(e, 4))
    p1 = pn(*cur)
    out = [p1]
    for _ in range(7):
        X, Y, Z, T = cur
        a, b, c = mmul(Y + C4R - X, p1[0]), mmul(Y + X, p1[1]), mmul(T, p1[2])
        d = 2 * Z if affine_base else mmul(Z, p1[3])
        ee, f, g, h = b + C4R - a, d + C4R - c, d + c, b + a
        cur = (mmul(ee, f), mmul(g, h), mmul(f, g), mmul(ee, h))
        out.append(pn(*cur))
    if layout == 1:
        out = [(v[0] - (v[0] >> 232) // fr.TOP_DIV * R_MOD,) + v[1:] for v in out]
    return out


def split(v, n):
    return [tuple(v[9 * i:9 * i + 9]) for i in range(n)]


def plain(l):
    return lval(l) * RINV % R_MOD


def ext_affine(e):
    """the affine point of 36 limbs (Z != 0)"""
    X, Y, Z, _ = (plain(c) for c in split(e, 4))
    zi = inv(Z)
    return (X * zi % R_MOD, Y * zi % R_MOD)


def ext_valid(e):
    X, Y, Z, T = (plain(c) for c in split(e, 4))
    return Z != 0 and (T * Z - X * Y) % R_MOD == 0 and on_m1(ext_affine(e))


def niels_point(n):
    """the affine point of a Niels entry (27 limbs), or None when its third word is not 2 D' x y"""
    ymx, ypx, t2d = (plain(c) for c in split(n, 3))
    h = inv(2)
    q = ((ypx - ymx) * h % R_MOD, (ypx + ymx) * h % R_MOD)
    return q if t2d == 2 * DP * q[0] * q[1] % R_MOD and on_m1(q) else None


def pniels_proj(n, negate=False):
    """(2X : 2Y : 2Z) of a PNiels entry (36 limbs), the point negated on request"""
    ymx, ypx, _, z2 = (plain(c) for c in split(n, 4))
    X = (ypx - ymx) % R_MOD
    return (-X % R_MOD if negate else X, (ypx + ymx) % R_MOD, z2)


def pniels_valid(n):
    ymx, ypx, t2d, z2 = (plain(c) for c in split(n, 4))
    if z2 == 0 or (t2d * z2 - DP * (ypx - ymx) * (ypx + ymx)) % R_MOD:       # (2 D' T)(2 Z) = D' (2X)(2Y)
        return False
    zi = inv(z2)
    return on_m1(((ypx - ymx) * zi % R_MOD, (ypx + ymx) * zi % R_MOD))


# ---- scalars ---------------------------------------------------------------------------------------------------------------
def nibbles(v):
    return sum(v << (4 * i) for i in range(64))


def edge_scalars():
    """all below 2^254"""
    v = [0, 1, 2, 7, 8, 9, 15, 16, SUBORDER - 1, SUBORDER, SUBORDER + 1, ORDER - 1, (1 << 254) - 1]
    v += [nibbles(d) % (1 << 254) for d in (7, 8, 9)]           # the top nibble cut to two bits: 0x3777.., 0x0888.., 0x1999..
    for w in (0, 31, 62):
        v += [d << (4 * w) for d in (1, 7, 8, 9, 15)]
    v += [d << 252 for d in (1, 2, 3)]
    rnd = random.Random(0x5CA1A)
    v += [rnd.randrange(ORDER) for _ in range(6)]
    assert all(0 <= x < 1 << 254 for x in v)
    return dedup(v)


def recode(s, nwin=64):
    """the signed digits of vb_mul_windowed, least significant window first"""
    t = s + nibbles(8)
    return [((t >> (4 * j)) & 15) - 8 for j in range(nwin)]


# ---- off-curve operands of ref_add ---------------------------------------------------------------------------------------------
def vanishing_pairs():
    """(p, q, which) projective operands of the reference's addition with z1, z2 != 0 whose sum has f = 0 (which = 'f':
    D x1 x2 y1 y2 == z1^2 z2^2) or g = 0 ('g': == -z1^2 z2^2): y2 solved from seeded x1, y1, x2, z1, z2; z3 = f g = 0, so affine()
    answers (0, 0).  No ON-curve pair does this (the law is complete), so at least one operand is off the curve."""
    rnd = random.Random(0xF0F0)
    out = []
    for which, sign in (("f", 1), ("g", -1)):
        for k in range(6):
            x1, y1, x2 = (rnd.randrange(1, R_MOD) for _ in range(3))
            z1, z2 = (1, 1) if k < 3 else (rnd.randrange(1, R_MOD), rnd.randrange(1, R_MOD))
            if k == 1:
                x1, y1 = B8                                  # one operand on the curve
            p = (x1 * z1 % R_MOD, y1 * z1 % R_MOD, z1)
            y2 = sign * z1 * z1 * z2 * z2 * inv(D_REF * p[0] * x2 * p[1]) % R_MOD
            out.append((p, (x2, y2, z2), which))
    return out


def ref_edge_points():
    """the edge points on the reference curve"""
    return [from_m1(p) for p in edge_points()]


def flip_bits(w):
    """the bits of word w of a table entry that a test may flip: the entry stays N-form below 2r (29 bits of the limbs 0 .. 7; 21 of
    the top limb, which is at most 3171406 < 2^22), so that fixed_table_check_slot, which multiplies the entry it judges, stays
    inside fr_mul's contract"""
    return 21 if w % 9 == 8 else 29


# ---- edge sets -------------------------------------------------------------------------------------------------------------
def _pair_partners(p):
    return [p, neg(p), (0, 1)]


_CACHE = {}


def edge_set(op):
    if op not in _CACHE:
        _CACHE[op] = _edge_set(op)
    return _CACHE[op]


def _ext_all():
    """every representation of every edge point"""
    return [e for p in edge_points() for e in ext_reps(p)]


def _edge_set(op):  # noqa: C901
    pts = edge_points()
    rnd = random.Random(0xED6E + OPS[op])
    if op in ("madd_t", "madd", "addpn_t", "addpn", "window"):
        pn = op not in ("madd_t", "madd")
        out = []

        def entries(q, full):
            if not pn:
                es = niels_reps(q)
                return es if full else [es[0], es[7], es[rnd.randrange(1, 7)]]
            zs = edge_zs(q)
            if full:
                es = [e for z in zs[:3] for e in pniels_reps(q, z)]
                return es + [to_pniels_model(x) for x in ext_reps(q, False, rnd)]
            z = zs[rnd.randrange(len(zs))]
            return pniels_reps(q, z, (0, 15, rnd.randrange(1, 15))) + [to_pniels_model(x) for x in ext_reps(q, False, rnd)[:4]]

        def tail(negate, k):
            return (negate,) + ((k & 1,) if op == "window" else ())

        # P + (-P), P + P, P + O for every edge point: every representation of P against a few of the entry, and the other way round
        for p in pts:
            for q in _pair_partners(p):
                all_p, few_p = ext_reps(p), ext_reps(p, False, rnd)
                for negate in (0, 1):
                    ent = q if not negate else neg(q)        # the entry holds -q when the op negates it: the sum is p + q either way
                    few_e, all_e = entries(ent, False), entries(ent, True)
                    out += [(e, few_e[i % 2] + tail(negate, i)) for i, e in enumerate(all_p) if i % 2 == negate]
                    out += [(few_p[i % len(few_p)], n + tail(negate, i)) for i, n in enumerate(all_e)]
        # every ordered pair of edge points (the torsion pairs among them), representations taken in turn
        for i, p in enumerate(pts):
            rp = ext_reps(p, False, rnd)
            for j, q in enumerate(pts):
                for negate in (0, 1):
                    es = entries(q, False)
                    out.append((rp[(i + 3 * j) % len(rp)], es[(i + j) % len(es)] + tail(negate, i + j)))
        return dedup(out)
    if op in ("dbl_t", "dbl", "to_pniels", "table"):
        return [(e,) for e in _ext_all()]
    if op == "table_affine":
        out = []
        for p in pts:
            c = ext_coords(p, 1)
            out += [(sum((reps(c[i])[(m >> i) & 1] for i in range(4)), ()),) for m in range(16)]
        return dedup(out)
    if op in ("pn2ext_t", "pn2ext"):
        out = []
        for p in pts:
            for z in edge_zs(p):
                out += [(n + (negate,),) for n in pniels_reps(p, z) for negate in (0, 1)]
            out += [(to_pniels_model(e) + (negate,),) for e in ext_reps(p) for negate in (0, 1)]
        return dedup(out)
    if op in ("lift_t", "lift", "nfa_t", "nfa", "from_ref"):
        out = []
        for p in pts:
            x, y = p
            if op in ("lift_t", "lift"):
                c = ((y - x) % R_MOD, (y + x) % R_MOD, (2 * x * y if op == "lift_t" else 2 * DP * x * y) % R_MOD)
                out += [(sum((reps(c[i])[(m >> i) & 1] for i in range(3)), ()),) for m in range(8)]
            else:
                if op == "from_ref":
                    x, y = from_m1(p)
                out += [(a, b) for a in reps(x) for b in reps(y)]
        return dedup(out)
    if op == "eq_niels":
        out = []
        # ext_equals_niels subtracts 2X and 2Y with fr_sub, whose subtrahend stays below 4r - 2^232: X, Y < 2r - 2^231 (its callers
        # pass products of fr_mul, below 1.3 r) -- the representations with X or Y at 2r - 1 are outside this one op's contract
        fits = lambda e: 2 * lval(e[0:9]) >> 232 <= TOP4 and 2 * lval(e[9:18]) >> 232 <= TOP4      # noqa: E731
        for i, p in enumerate(pts):
            for e in filter(fits, ext_reps(p)):
                for q in (p, neg(p)):                        # equal in another scaling, and the nearest unequal point
                    out.append((e, niels_reps(q)[(len(out) * 5) % 8]))
            for j, q in enumerate(pts):
                few = list(filter(fits, ext_reps(p, False, rnd)))
                out.append((few[(i + j) % len(few)], niels_reps(q)[(i + 3 * j) % 8]))
        return dedup(out)
    if op == "ref_add":
        rp = ref_edge_points()
        zs = [1, R_MOD - 1, random.Random(0x2EF).randrange(2, R_MOD)]
        out = []

        def proj_reps(c, i):
            return sum((reps(c[k])[(i >> k) & 1] for k in range(3)), ())
        for i, p in enumerate(rp):                          # every ordered pair, scaled by the edge z values
            for j, q in enumerate(rp):
                for k, z1 in enumerate(zs):
                    z2 = zs[(k + i + j) % 3]
                    out.append((proj_reps((p[0] * z1 % R_MOD, p[1] * z1 % R_MOD, z1), i + k), proj_reps((q[0] * z2 % R_MOD, q[1] * z2 % R_MOD, z2), j + 2 * k)))
        for p, q, _ in vanishing_pairs():                   # f = 0 and g = 0 inside the addition, every representative
            out += [(proj_reps(p, m), proj_reps(q, m2)) for m in range(8) for m2 in (0, 7, m)]
        # z = 0 inputs and coordinates at 0, 1, r - 1 (+ r: 2r - 1), as raw representatives
        raw = [0, 1, R_MOD - 1, R_MOD, R_MOD + 1, 2 * R_MOD - 1]
        b8p = tuple(mont(c) for c in B8) + (R1,)
        for v in raw:
            for pos in range(3):
                c = list(b8p)
                c[pos] = v
                t = tuple(nform(x) for x in c)
                t = t[0] + t[1] + t[2]
                out += [(t, nform(b8p[0]) + nform(b8p[1]) + nform(b8p[2])), (nform(b8p[0]) + nform(b8p[1]) + nform(b8p[2]), t), (t, t)]
            out.append((nform(v) * 3, nform(v) * 3))
        return dedup(out)
    if op in ("ref_mul8", "ref_mul2", "var_base"):
        rp = ref_edge_points()
        sc = edge_scalars() if op != "ref_mul2" else [s for s in edge_scalars() if s < 1 << 64] + [(1 << 64) - 1, 1 << 63, 0x8888888888888888]
        if op != "ref_mul2":
            sc = sc + [(1 << 256) - 1, ORDER, ORDER + 1, 1 << 255]          # raw 256-bit scalars: these ops take any
        nw = 2 if op == "ref_mul2" else 8
        out = []
        for i, p in enumerate(rp):
            for j, s in enumerate(sc):
                m = (i + j) % 4
                out.append((reps(p[0])[m & 1] + reps(p[1])[m >> 1], words(s)[:nw]))
        # off the curve: the exact path (short scalars and a few wide ones), and the operands of the vanishing pairs as bases
        off = [(B8[0] + 1, B8[1]), (0, 0), (1, 1), (R_MOD - 1, R_MOD - 1), (0, 2), (2, 0)] + [p[:2] for p, _, _ in vanishing_pairs()[:3]]
        for i, p in enumerate(off):
            for s in (0, 1, 2, 3, 5, 0xffff, (1 << 64) - 1) + (() if nw == 2 else ((1 << 254) - 1, ORDER - 1)):
                out.append((reps(p[0])[i & 1] + reps(p[1])[(i >> 1) & 1], words(s)[:nw]))
        return dedup(out)
    if op in MULW:
        nwin = MULW[op][0]
        sc = edge_scalars() if nwin == 64 else list(range(1 << (4 * nwin - 2)))
        out = []
        for p in pts:
            full, few = ext_reps(p), ext_reps(p, False, rnd)
            out += [(few[(j * 7) % len(few)], words(s)) for j, s in enumerate(sc)]
            out += [(e, words(sc[(i * 5) % len(sc)])) for i, e in enumerate(full)]
        return dedup(out)
    if op == "fixed_entry":
        return dedup([((k, j, t),) for k in range(16) for j in (0, 1, 2, 31, 62) for t in (0, 1)])
    if op == "fixed_chain":
        return [((c,),) for c in range(1, 10)]
    if op == "fixed_flip":
        # one bit per used word of an entry, in a first, a middle and a last slot of each window
        return dedup([((3 + (s + w) % 6, 9 * j + s, w, (5 * w + s + j) % flip_bits(w)),) for j in range(FT_NWIN) for s in (0, 4, 8) for w in range(27)])
    raise ValueError(op)


# ---- seeded random inputs, inside the domain by construction --------------------------------------------------------------------
def _rand_z(rnd):
    return rnd.randrange(1, R_MOD)


def _rand_rep(rnd, v):
    return reps(v)[rnd.randrange(2)]


def _rand_ext(rnd, p, z=None):
    c = ext_coords(p, _rand_z(rnd) if z is None else z)
    return sum((_rand_rep(rnd, v) for v in c), ())


def _rand_entry(rnd, q, pn):
    if not pn:
        return sum((_rand_rep(rnd, v) for v in niels_coords(q)), ())
    if rnd.randrange(2):
        return to_pniels_model(_rand_ext(rnd, q))
    return sum((_rand_rep(rnd, v) for v in pniels_coords(q, _rand_z(rnd))), ())


def _rand_pair(rnd):
    """two points: mostly independent, one in eight related (equal, opposite, or one the identity or of small order)"""
    pl = pool()
    p = pl[rnd.randrange(len(pl))]
    k = rnd.randrange(32)
    if k == 0:
        return p, p
    if k == 1:
        return p, neg(p)
    if k == 2:
        return p, edge_points()[rnd.randrange(8)]
    if k == 3:
        return edge_points()[rnd.randrange(8)], p
    return p, pl[rnd.randrange(len(pl))]


def _rand_scalar(rnd, bound):
    return rnd.randrange(bound) if rnd.randrange(4) else rnd.getrandbits(rnd.randint(1, bound.bit_length() - 1))


def random_set(op, rnd, n):  # noqa: C901
    """n seeded random items for the op (the chain op has nine distinct inputs in all: they are repeated in turn, 72 at most)"""
    pl = pool()
    pick = lambda: pl[rnd.randrange(len(pl))]                # noqa: E731
    out = []
    if op in ("madd_t", "madd", "addpn_t", "addpn", "window"):
        pn = op not in ("madd_t", "madd")
        for _ in range(n):
            p, q = _rand_pair(rnd)
            negate = rnd.randrange(2)
            b = _rand_entry(rnd, q, pn) + (negate,) + ((rnd.randrange(2),) if op == "window" else ())
            out.append((_rand_ext(rnd, p), b))
    elif op in ("dbl_t", "dbl", "to_pniels", "table"):
        out = [(_rand_ext(rnd, pick()),) for _ in range(n)]
    elif op == "table_affine":
        out = [(_rand_ext(rnd, pick(), 1),) for _ in range(n)]
    elif op in ("pn2ext_t", "pn2ext"):
        out = [(_rand_entry(rnd, pick(), True) + (rnd.randrange(2),),) for _ in range(n)]
    elif op in ("lift_t", "lift"):
        for _ in range(n):
            x, y = pick()
            c = ((y - x) % R_MOD, (y + x) % R_MOD, (2 * x * y if op == "lift_t" else 2 * DP * x * y) % R_MOD)
            out.append((sum((_rand_rep(rnd, v) for v in c), ()),))
    elif op == "eq_niels":
        for _ in range(n):
            p, q = _rand_pair(rnd)
            if rnd.randrange(2):
                q = p
            out.append((_rand_ext(rnd, p), _rand_entry(rnd, q, False)))
    elif op in ("nfa_t", "nfa", "from_ref"):
        for _ in range(n):
            x, y = pick()
            if op == "from_ref":
                x, y = from_m1((x, y))
            out.append((_rand_rep(rnd, x), _rand_rep(rnd, y)))
    elif op == "ref_add":
        for _ in range(n):
            p, q = _rand_pair(rnd)
            k = rnd.randrange(8)
            trip = []
            for pt in (p, q):
                x, y = from_m1(pt)
                z = 1 if k == 0 else _rand_z(rnd)
                c = [x * z % R_MOD, y * z % R_MOD, z]
                if k == 1:                                   # any three values: the formula is total
                    c = [rnd.randrange(R_MOD) for _ in range(3)]
                trip.append(sum((_rand_rep(rnd, v) for v in c), ()))
            out.append(tuple(trip))
    elif op in ("ref_mul8", "ref_mul2", "var_base"):
        nw = 2 if op == "ref_mul2" else 8
        for _ in range(n):
            x, y = from_m1(pick())
            s = rnd.getrandbits(rnd.randint(1, 32 * nw))     # every length: the loop runs over bit_length() bits
            if rnd.randrange(64) == 0:                       # off the curve: the exact path, short scalars mostly
                x = (x + 1 + rnd.randrange(5)) % R_MOD
                s = rnd.getrandbits(rnd.choice((1, 2, 3, 8, 16, 32, 32 * nw)))
            out.append((_rand_rep(rnd, x) + _rand_rep(rnd, y), words(s)[:nw]))
    elif op in MULW:
        bound = 1 << (4 * MULW[op][0] - 2)
        out = [(_rand_ext(rnd, pick()), words(_rand_scalar(rnd, bound) if bound > 4 else rnd.randrange(bound))) for _ in range(n)]
    elif op == "fixed_entry":
        out = [((rnd.randrange(16), rnd.randrange(63), rnd.randrange(2)),) for _ in range(n)]
    elif op == "fixed_chain":
        out = [((1 + i % 9,),) for i in range(min(n, 72))]
    elif op == "fixed_flip":
        for _ in range(n):
            w = rnd.randrange(27)
            out.append(((1 + rnd.randrange(9), rnd.randrange(FT_SLOTS), w, rnd.randrange(flip_bits(w))),))
    else:
        raise ValueError(op)
    return out


# ---- domains (the contracts stated in the comments of curve.hpp / bjj_device.hpp) ---------------------------------------------
def _isn(l, bound):
    """N-form (limbs 0 .. 7 below 2^29) with a value below `bound`"""
    return len(l) == 9 and all(0 <= x <= M29 for x in l[:8]) and 0 <= l[8] and lval(l) < bound


def _ext_ok(e):
    """coordinates N-form < 2r (ext_madd, ext_add_pn, ext_dbl, ext_to_pniels), a point of the curve with T Z == X Y"""
    return all(_isn(c, 2 * R_MOD) for c in split(e, 4)) and ext_valid(e)


def _niels_ok(n):
    """entries N-form < 2r (ext_madd)"""
    return all(_isn(c, 2 * R_MOD) for c in split(n, 3)) and niels_point(n) is not None


def _pniels_ok(n):
    """entries carried: ymx < 8r (Y + 4r - X), ypx < 4r, z2 < 4r, t2d N-form < 4r with a top limb fr_sub_lazy takes (pniels_cneg)"""
    ymx, ypx, t2d, z2 = split(n, 4)
    return (_isn(ymx, 8 * R_MOD) and _isn(ypx, 4 * R_MOD) and _isn(t2d, 4 * R_MOD) and t2d[8] <= TOP4 and _isn(z2, 4 * R_MOD)
            and pniels_valid(n))


def _flag(v):
    return v in (0, 1)


def in_domain(op, item):  # noqa: C901
    wa, wb, _, _ = WIDTHS[op]
    a = item[0]
    b = item[1] if len(item) > 1 else None
    if len(a) != wa or (b is None) != (wb == 0) or (b is not None and len(b) != wb):
        return False
    w32 = lambda w: all(0 <= x < 1 << 32 for x in w)         # noqa: E731
    lt2r = lambda l: _isn(l, 2 * R_MOD)                      # noqa: E731
    if op in ("madd_t", "madd"):
        return _ext_ok(a) and _niels_ok(b[:27]) and _flag(b[27])
    if op in ("addpn_t", "addpn", "window"):
        return _ext_ok(a) and _pniels_ok(b[:36]) and all(_flag(v) for v in b[36:])
    if op in ("dbl_t", "dbl", "to_pniels", "table"):
        return _ext_ok(a)
    if op == "table_affine":
        return _ext_ok(a) and plain(a[18:27]) == 1           # affine_base: Z == 1
    if op in ("pn2ext_t", "pn2ext"):
        return _pniels_ok(a[:36]) and _flag(a[36])
    if op in ("lift_t", "lift"):
        ymx, ypx, t = (plain(c) for c in split(a, 3))
        x, y = (ypx - ymx) * inv(2) % R_MOD, (ypx + ymx) * inv(2) % R_MOD
        want = 2 * x * y if op == "lift_t" else 2 * DP * x * y
        return all(lt2r(c) for c in split(a, 3)) and (t - want) % R_MOD == 0
    if op == "eq_niels":                                     # fr_eq(., fr_dbl(X)): 2X and 2Y are subtrahends of fr_sub
        return _ext_ok(a) and _niels_ok(b) and 2 * lval(a[0:9]) >> 232 <= TOP4 and 2 * lval(a[9:18]) >> 232 <= TOP4
    if op in ("nfa_t", "nfa", "from_ref"):
        return lt2r(a) and lt2r(b)
    if op == "ref_add":
        return all(lt2r(c) for c in split(a, 3) + split(b, 3))
    if op in ("ref_mul8", "ref_mul2", "var_base"):
        return all(lt2r(c) for c in split(a, 2)) and w32(b)
    if op in MULW:
        return _ext_ok(a) and w32(b) and fr.wval(b) < 1 << (4 * MULW[op][0] - 2)      # no carry out of the top window
    if op == "fixed_entry":
        return 0 <= a[0] < 16 and 0 <= a[1] < 63 and _flag(a[2])
    if op == "fixed_chain":
        return 1 <= a[0] <= 9
    if op == "fixed_flip":
        return 1 <= a[0] <= 9 and 0 <= a[1] < FT_SLOTS and 0 <= a[2] < 27 and 0 <= a[3] < flip_bits(a[2])
    raise ValueError(op)


# ---- records and checks ------------------------------------------------------------------------------------------------------
def records(op, items):
    """(a, b) uint32 records for `items`; b is None for the ops with one operand"""
    wa, wb, _, _ = WIDTHS[op]
    a = np.array([it[0] for it in items], dtype=np.uint64).astype(np.uint32).reshape(len(items), wa)
    b = np.array([it[1] for it in items], dtype=np.uint64).astype(np.uint32).reshape(len(items), wb) if wb else None
    return a, b


def items_of(op, a, b):
    """the inverse of records"""
    if b is None:
        return [(tuple(int(x) for x in r),) for r in a]
    return [(tuple(int(x) for x in r), tuple(int(x) for x in s)) for r, s in zip(a, b)]


class _Rows:
    """the field elements of many records at once: raw integer values, plain values, N-form verdicts"""

    def __init__(self, arr, nel, offset=0):
        arr = np.asarray(arr, dtype=np.uint32)
        self.raw = [vals_of_limbs(arr[:, offset + 9 * k:offset + 9 * k + 9]) for k in range(nel)]
        self.low = [(arr[:, offset + 9 * k:offset + 9 * k + 8] <= M29).all(axis=1) for k in range(nel)]
        self.zero = [(arr[:, offset + 9 * k:offset + 9 * k + 9] == 0).all(axis=1) for k in range(nel)]

    def plain(self, i):
        return tuple(v[i] * RINV % R_MOD for v in self.raw)

    def nform_below(self, i, bounds):
        return all(self.low[k][i] and self.raw[k][i] < bd for k, bd in enumerate(bounds) if bd is not None)


def _ext_out(O, i, want, need_t):
    """an output Ext against the projective point `want`: N-form below 2r (what the next formula takes), Z != 0, the point, and
    T Z == X Y where T is asked for, T exactly the zero limbs where it is not"""
    X, Y, Z, T = O.plain(i)
    if not O.nform_below(i, (2 * R_MOD,) * 3 + ((2 * R_MOD,) if need_t else (None,))):
        return "not N-form below 2r"
    if not peq((X, Y, Z), want):
        return "point (%d : %d : %d), want (%d : %d : %d)" % ((X, Y, Z) + tuple(want))
    if need_t and (T * Z - X * Y) % R_MOD:
        return "T Z != X Y"
    if not need_t and not O.zero[3][i]:
        return "T not the zero limbs"
    return None


def _entry_out(E, i, want, strict_first=None):
    """an output PNiels against the projective point `want`: (ypx - ymx : ypx + ymx : z2) the point, t2d z2 == D' (2X)(2Y), bounds
    of the consumers (pniels_to_ext: ymx < 8r, ypx < 4r; pniels_cneg: t2d N-form < 4r)"""
    ymx, ypx, t2d, z2 = E.plain(i)
    if not E.nform_below(i, (8 * R_MOD, 4 * R_MOD, 4 * R_MOD, 4 * R_MOD)) or E.raw[2][i] >> 232 > TOP4:
        return "entry out of bounds"
    if not peq(((ypx - ymx) % R_MOD, (ypx + ymx) % R_MOD, z2), want):
        return "entry is another point"
    if (t2d * z2 - DP * (ypx - ymx) * (ypx + ymx)) % R_MOD:
        return "t2d inconsistent"
    return None


def _niels_limbs(q, tform):
    x, y = q
    return nform(mont(y - x)) + nform(mont(y + x)) + nform(mont(2 * x * y if tform else 2 * DP * x * y))


def _fixed_point(k, j):
    X, Y, Z = g0_mul(LOG_B8 * k * (1 << (4 * j)))
    zi = inv(Z)
    return (X * zi % R_MOD, Y * zi % R_MOD)


def check(op, items, out, ref=None, layout=0):  # noqa: C901
    """indices (with a reason) where the op's output is not what the integers say.  `ref`: an object with the reference's
    proj_add, proj_affine and mul_scalar (the Python oracle); the model's own statement of them when None."""
    ref = ref or _Own
    a, b = records(op, items)
    out = np.asarray(out, dtype=np.uint32)
    n = len(items)
    assert out.shape == (n, WIDTHS[op][2]), (op, out.shape)
    bad = []

    def note(i, why):
        if why:
            bad.append((i, why))
    if op in ("madd_t", "madd", "addpn_t", "addpn", "window", "dbl_t", "dbl"):
        P, O = _Rows(a, 4), _Rows(out, 4)
        pn = op in ("addpn_t", "addpn", "window")
        Q = None if b is None else _Rows(b, 4 if pn else 3)
        for i in range(n):
            p = P.plain(i)[:3]
            if op in ("dbl_t", "dbl"):
                want, need_t = padd(p, p), op == "dbl_t"
            else:
                e = Q.plain(i)
                negate = bool(b[i, 36 if pn else 27])
                x2 = (e[1] - e[0]) % R_MOD
                q = (-x2 % R_MOD if negate else x2, (e[1] + e[0]) % R_MOD, e[3] if pn else 2)
                if op == "window":
                    for _ in range(4):
                        p = padd(p, p)
                want = padd(p, q)
                need_t = bool(b[i, 37]) if op == "window" else op.endswith("_t")
            note(i, _ext_out(O, i, want, need_t))
    elif op == "to_pniels":
        P, E = _Rows(a, 4), _Rows(out, 4)
        for i in range(n):
            X, Y, Z, T = (P.raw[k][i] for k in range(4))
            why = _entry_out(E, i, P.plain(i)[:3])
            if not why and (E.raw[0][i] != Y + C4R - X or E.raw[1][i] != Y + X or E.raw[3][i] != 2 * Z or E.raw[2][i] != mmul(T, mont(2 * DP))):
                why = "not Y + 4r - X, Y + X, T (2 D') as the Montgomery product, 2 Z limb for limb"
            if not why and E.raw[2][i] >= 2 * R_MOD:
                why = "t2d not below 2r"
            note(i, why)
    elif op in ("pn2ext_t", "pn2ext"):
        O = _Rows(out, 4)
        for i in range(n):
            note(i, _ext_out(O, i, pniels_proj(items[i][0][:36], bool(a[i, 36])), op == "pn2ext_t"))
    elif op in ("lift_t", "lift"):
        N, O = _Rows(a, 3), _Rows(out, 4)
        for i in range(n):
            ymx, ypx, _ = N.plain(i)
            why = _ext_out(O, i, ((ypx - ymx) % R_MOD, (ypx + ymx) % R_MOD, 2), True) if O.raw[1][i] < 2 * R_MOD else None
            # Y is the carried sum of two components (< 4r when both are at + r: the table's own entries are canonical), Z is 2
            if not why and (O.raw[1][i] != N.raw[0][i] + N.raw[1][i] or O.raw[2][i] != 2 * R1 or O.raw[0][i] >= 2 * R_MOD
                            or not (O.low[0][i] and O.low[1][i] and O.low[2][i] and O.low[3][i])):
                why = "X, Y or Z out of form"
            if not why and (O.plain(i)[0] - (ypx - ymx)) % R_MOD:
                why = "X is not ypx - ymx"
            if not why and op == "lift_t" and O.raw[3][i] != N.raw[2][i]:
                why = "T form: T is not the third word as it is"
            if not why and (O.plain(i)[3] * 2 - O.plain(i)[0] * O.plain(i)[1]) % R_MOD:
                why = "T Z != X Y"
            note(i, why)
    elif op == "eq_niels":
        for i in range(n):
            want = ext_affine(items[i][0]) == niels_point(items[i][1])
            note(i, None if int(out[i, 0]) == int(want) else "verdict %d, want %d" % (out[i, 0], want))
    elif op in ("nfa_t", "nfa"):
        X, Y = _Rows(a, 1), _Rows(b, 1)
        for i in range(n):
            want = _niels_limbs((X.plain(i)[0], Y.plain(i)[0]), op == "nfa_t")
            note(i, None if tuple(int(v) for v in out[i]) == want else "limbs %s, want %s" % (out[i].tolist(), want))
    elif op == "from_ref":
        X, Y, O = _Rows(a, 1), _Rows(b, 1), _Rows(out, 4)
        for i in range(n):
            x, y = X.plain(i)[0], Y.plain(i)[0]
            why = _ext_out(O, i, (F * x % R_MOD, y, 1), True)
            if not why and (O.raw[1][i] != Y.raw[0][i] or O.raw[2][i] != R1):
                why = "Y is not y as it is, or Z is not one"
            note(i, why)
    elif op == "ref_add":
        P, Q, O = _Rows(a, 3), _Rows(b, 3), _Rows(out, 3)
        for i in range(n):
            want = tuple(v % R_MOD for v in ref.proj_add(P.plain(i), Q.plain(i)))
            if O.plain(i) != want or not O.nform_below(i, (2 * R_MOD,) * 3):
                note(i, "(%d, %d, %d), want (%d, %d, %d)" % (O.plain(i) + want))
    elif op in ("ref_mul8", "ref_mul2", "var_base"):
        P = _Rows(a, 2)
        S = vals_of_words(b) if op != "ref_mul2" else [fr.wval(tuple(r) + (0,) * 6) for r in b.tolist()]
        O = _Rows(out, 2 if op != "var_base" else 4)
        exact = ref is not _Own and op != "var_base"        # with the oracle at hand: its own bit-serial loop on every item
        for i in range(n):
            pt = P.plain(i)
            if exact or not on_ref(pt):
                want = tuple(v % R_MOD for v in ref.mul_scalar(pt, S[i]))
            else:                                            # on the curve the affine result is unique: the group law gives it
                X, Y, Z = smul_known(to_m1(pt), S[i])
                zi = inv(Z)
                want = (X * zi * FINV % R_MOD, Y * zi % R_MOD)
            if op == "var_base":
                X, Y, Z, _ = O.plain(i)
                ok = (O.nform_below(i, (2 * R_MOD,) * 3) and Z != 0 and (X - F * want[0] * Z) % R_MOD == 0 and (Y - want[1] * Z) % R_MOD == 0
                      and O.zero[3][i])
            else:
                ok = O.plain(i) == want and O.nform_below(i, (2 * R_MOD,) * 2)
            note(i, None if ok else "%s, want %s" % (O.plain(i), want))
    elif op in ("table", "table_affine"):
        P = _Rows(a, 4)
        E = [_Rows(out, 4, 36 * k) for k in range(9)]
        ident = nform(R1) + nform(R1) + (0,) * 9 + nform(2 * R1)
        for i in range(n):
            p = P.plain(i)[:3]
            why = None if tuple(int(v) for v in out[i, :36]) == ident else "entry 0 is not the identity (1, 1, 0, 2)"
            acc = p
            model = table_model(items[i][0], op == "table_affine", layout)
            for k in range(1, 9):
                why = why or _entry_out(E[k], i, acc)
                if not why and tuple(E[k].raw[c][i] for c in range(4)) != model[k - 1]:
                    why = "not the model's entry value for value"
                if layout == 1 and not why and not (E[k].raw[0][i] < 2 * R_MOD and all(E[k].raw[c][i] < 1 << 256 for c in range(4))):
                    why = "packed entry: ymx not weakly reduced or a component of 2^256 or more"
                if why:
                    why = "%s (entry %d)" % (why, k) if "(entry" not in why else why
                    break
                acc = padd(acc, p)
            note(i, why)
    elif op in MULW:
        nwin, final_t = MULW[op]
        P, O = _Rows(a, 4), _Rows(out, 4)
        S = vals_of_words(b)
        for i in range(n):
            p = P.plain(i)[:3]
            if nwin == 64:
                want = smul_known(ext_affine(items[i][0]), S[i])
            else:
                want, e, k = (0, 1, 1), p, S[i]
                while k:
                    if k & 1:
                        want = padd(want, e)
                    e, k = padd(e, e), k >> 1
            note(i, _ext_out(O, i, want, final_t))
    elif op == "fixed_entry":
        for i in range(n):
            k, j, t = items[i][0]
            want = _niels_limbs(_fixed_point(k, j), bool(t))
            note(i, None if tuple(int(v) for v in out[i]) == want else "limbs %s, want %s" % (out[i].tolist(), want))
    elif op == "fixed_chain":
        want = [_niels_limbs(_fixed_point(s % 9, s // 9), s < 9) for s in range(FT_SLOTS)]
        for i in range(n):
            for s in range(FT_SLOTS):
                row = out[i, 28 * s:28 * s + 28]
                if tuple(int(v) for v in row[:27]) != want[s] or row[27] != 0:
                    note(i, "slot %d: limbs %s count %d, want %s" % (s, row[:27].tolist(), row[27], want[s]))
                    break
    elif op == "fixed_flip":
        for i in range(n):
            note(i, None if out[i, 0] > 0 else "the flipped slot's check counts nothing")
    else:
        raise ValueError(op)
    return bad


def cpu_run(lib, op, a, b):
    """the op on the CPU harness (tests/emul/emul_curve_ops.cpp: the g++ build of curve_ops.hpp) -> (n, out words) uint32"""
    n = a.shape[0]
    wa, wb, wo, _ = WIDTHS[op]
    assert a.shape == (n, wa) and ((b is None and wb == 0) or b.shape == (n, wb))
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = None if b is None else np.ascontiguousarray(b, dtype=np.uint32)
    out = np.zeros((n, wo), dtype=np.uint32)
    vp = ctypes.c_void_p

    def part(lo, hi):
        return lib.emul_curve_op(ctypes.c_int(OPS[op]), a[lo:hi].ctypes.data_as(vp), None if b is None else b[lo:hi].ctypes.data_as(vp),
                                 out[lo:hi].ctypes.data_as(vp), ctypes.c_size_t(hi - lo))
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
