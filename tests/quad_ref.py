"""Plain-integer model and directed input sets for the four-lane ("quad") point arithmetic of csrc/k_small.hip: quad_dbl, quad_add,
quad_entry, quad_lift, quad_from_ref_affine, qtbl_build / qtbl_load, quad_walk, quad_walk_joint, quad_affine, quad_is_identity,
qfb_load, quad_mul_fixed_base, quad_add_fixed_base, as tests/devfuzz/quad_ops.hpp calls them.  Shared by
tests/test_quad_ops_host.py (the sets and the checker, judged without a GPU) and tests/test_gpu_quad_ops.py (the device).  Built
on tests/curve_ref.py: its constants, points with known logs, representations and scalars; nothing is read from the product's
headers.  A plain helper module: no fixtures, no pytest hooks.

INPUT DOMAINS -- what the producers inside k_small.hip can hand each function, not what curve.hpp admits.
  coordinate   an output of fr_mul, fr_reduce_weak, fr_one() or fr_to_mont_words: N-form (limbs 0 .. 7 below 2^29), value < 2r
  Ext          four coordinates of a point of the a' = -1 curve with T Z == X Y (quad_dbl, quad_entry, quad_affine and
               quad_is_identity never read T; the sets keep it consistent all the same)
  entry        an output of quad_entry -- ymx = fr_sub(Y, X) < 6r, ypx = fr_add < 4r, z2 = fr_dbl < 4r, t2d = fr_mul < 2r, all
               N-form -- or of qfb_load: canonical ymx, ypx, t2d and z2 = 2 (2^261 mod r).  The negated forms exist behind
               qtbl_load / qfb_load only, so `add`, `lift` and `table` send the entry through the table and the loader negates it.
  from_ref     y a coordinate; x a coordinate or fr_neg of one (bjj_k_eddsa_verify_small: -A, -+R): N-form, value <= 4r
  walk         scalar words below 2^(4 need - 2), 1 <= need <= 64: what recode_signed4 takes without a carry out of window
               need - 1 (eddsa_scalars: need = (bits + 5) >> 2; scalar_mod_order: below 8 l < 2^254, need = 64)
  affine,      any coordinates (the functions are coordinate-wise), Z != 0 for affine; beside the points of the curve the
  is_identity  sets hold triples that are no points, to reach the quotients 1 and r - 1 in x and the near misses of (0 : z : z)
  fb_*         scalar words below l (scalar_mod_l, verify_fb_scalar); slot below the table's size

OUTPUT BOUNDS, from the contract of csrc/fr.hpp (fr_mul: N-form result below 2r for operands whose product is below 2^261 r,
about 169 r^2):
  dbl, add, walk, walk_joint, fb_mul, fb_add   every coordinate leaves quad_finish: one fr_mul of E, F, G, H below 10r, so the
               product is below 100 r^2: N-form < 2r -- the domain of every consumer above
  entry        as the domain says; quad_add multiplies ymx (< 6r) by Y - X (< 6r, lazy): 36 r^2; quad_lift subtracts ymx by
               fr_sub8, which takes a subtrahend below 8r - 2^232
  lift         X, Y, Z leave fr_reduce_weak, T fr_mul: N-form < 2r; T the zero limbs without WITH_T
  table        entries 0 .. 8 as `entry`; a negative digit swaps ymx / ypx and gives 4r - t2d limb by limb (limbs <= 2^30,
               value <= 4r), which feeds one multiplication by an N-form T below 2r: 8 r^2
  affine       fr_mul(c, m) with c, m < 2r is below r + 4r / 169: ONE conditional subtraction makes it canonical, below r
"""
import random

import numpy as np

import curve_ref as cr
import field_ref as fr
from curve_ref import (C4R, DP, F, FINV, LOG_B8, ORDER, SUBORDER, TOP4, _Rows, dedup, edge_points, edge_zs, ext_coords, ext_reps,
                       inv, lval, mmul, mont, neg, nform, padd, peq, pool, reps, smul_known, split, words)
from field_ref import C4, M29, R1, R_MOD, RINV

OPS = dict(dbl=0, dbl4=1, add=2, entry=3, lift_t=4, lift=5, from_ref=6, table=7, walk=8, walk_joint=9, affine=10, is_identity=11,
           fb_load=12, fb_mul=13, fb_add=14)
# record widths in words of tests/devfuzz/quad_ops.hpp: a, b, out
WIDTHS = dict(dbl=(36, 0, 36), dbl4=(36, 0, 36), add=(36, 38, 36), entry=(36, 0, 36), lift_t=(38, 0, 36), lift=(38, 0, 36),
              from_ref=(9, 9, 36), table=(36, 0, 17 * 36), walk=(36, 9, 40), walk_joint=(72, 17, 40), affine=(36, 0, 16),
              is_identity=(36, 0, 1), fb_load=(2, 0, 36), fb_mul=(8, 0, 36), fb_add=(8, 36, 36))
# the lane function of libbjj_curve_test.so (tests/devfuzz/curve_ops.hpp) that does the same field operations in the same order:
# the results are compared limb for limb
LANE_OP = dict(dbl="dbl_t", add="addpn_t", entry="to_pniels", lift_t="pn2ext_t", lift="pn2ext", from_ref="from_ref", table="table")
FB_W = 8                                                    # the fixed-base table of the fb ops
FB_NWIN = (252 + FB_W - 1) // FB_W
FB_STRIDE = (1 << (FB_W - 1)) + 1
FB_SLOTS = FB_NWIN * FB_STRIDE
D2P_M, DPINV_M, F_M, FINV_M = mont(2 * DP), mont(inv(DP)), mont(F), mont(FINV)
TWO_R1 = 2 * R1                                             # fr_dbl(fr_one()): not reduced
IDENT_ENTRY = nform(R1) + nform(R1) + (0,) * 9 + nform(TWO_R1)
C8R = 8 * R_MOD


def reduce_weak(v):
    return v - (v >> 232) // fr.TOP_DIV * R_MOD


def need_of(bits):
    """eddsa_scalars: the windows a pair whose wider scalar has `bits` bits needs"""
    return 1 if bits <= 2 else min(64, (bits + 5) >> 2)


# ---- the formulas on raw integers, representative for representative ----------------------------------------------------------
def dbl_model(c):
    """quad_dbl (ext_dbl) on the raw values X, Y, Z, T -> raw values"""
    X, Y, Z, _ = c
    a, b, zz, ss = mmul(X, X), mmul(Y, Y), mmul(Z, Z), mmul(X + Y, X + Y)
    h = a + b
    e, g, f = ss + C8R - h, b + C4R - a, 2 * zz + a + C4R - b
    return (mmul(e, f), mmul(g, h), mmul(f, g), mmul(e, h))


def add_model(c, n):
    """quad_add (ext_add_pn) on raw values; n = (ymx, ypx, t2d, z2) as the loader hands it"""
    X, Y, Z, T = c
    a, b, cc, d = mmul(Y + C4R - X, n[0]), mmul(Y + X, n[1]), mmul(T, n[2]), mmul(Z, n[3])
    e, f, g, h = b + C4R - a, d + C4R - cc, d + cc, b + a
    return (mmul(e, f), mmul(g, h), mmul(f, g), mmul(e, h))


def entry_model(c):
    X, Y, Z, T = c
    return (Y + C4R - X, Y + X, mmul(T, D2P_M), 2 * Z)


def load_model(n, negate):
    """qtbl_load / qfb_load of a stored entry with the digit's sign: raw values (the negated t2d is 4r - t2d)"""
    return (n[1], n[0], C4R - n[2], n[3]) if negate else tuple(n)


def lift_model(n, with_t):
    """quad_lift (pniels_to_ext) of a loaded entry"""
    return (reduce_weak(n[1] + C8R - n[0]), reduce_weak(n[1] + n[0]), reduce_weak(n[3]), mmul(n[2], DPINV_M) if with_t else 0)


def table_model(c):
    """qtbl_build: the raw values of the entries 0 .. 8"""
    p1 = entry_model(c)
    out = [tuple(lval(x) for x in split(IDENT_ENTRY, 4)), p1]
    cur = c
    for _ in range(7):
        cur = add_model(cur, p1)
        out.append(entry_model(cur))
    return out


def raws(v, n):
    return tuple(lval(x) for x in split(v, n))


def fb_point(slot):
    """the affine point of slot k + FB_STRIDE j of the fixed-base table: k 2^(FB_W j) B8"""
    j, k = divmod(slot, FB_STRIDE)
    X, Y, Z = cr.g0_mul(LOG_B8 * k * (1 << (FB_W * j)))
    zi = inv(Z)
    return (X * zi % R_MOD, Y * zi % R_MOD)


_FB = {}


def fb_entry(slot):
    """the stored entry: canonical Montgomery y - x', y + x' and 2 x' y (window 0, the T form) or 2 D' x' y"""
    if slot not in _FB:
        x, y = fb_point(slot)
        _FB[slot] = (mont(y - x), mont(y + x), mont(2 * x * y if slot < FB_STRIDE else 2 * DP * x * y))
    return _FB[slot]


# ---- sets --------------------------------------------------------------------------------------------------------------------
def _pn_rec(n36, k, negate):
    return tuple(n36) + (k, negate)


def _coord_reps(c, m):
    return sum((reps(c[i])[(m >> i) & 1] for i in range(len(c))), ())


def scalar_edges():
    """the ladder scalars: curve_ref's (0, 1, l - 1 .. 8l - 1, 2^254 - 1, the nibble patterns 7, 8, 9 whose recoding carries through
    every window or nowhere) and 0x0808..08, a carry into every other window"""
    return dedup(cr.edge_scalars() + [sum(8 << (8 * i) for i in range(32)) % (1 << 254), sum(8 << (8 * i + 4) for i in range(31))])


PAIR_BITS = (1, 2, 3, 126, 127, 130, 131, 250)


def _bits_scalar(rnd, bits):
    return (1 << (bits - 1)) | rnd.getrandbits(bits - 1) if bits > 1 else 1


def fb_scalar_edges():
    """below l: digits at, below and above half a window (0x80 stays, 0x81 turns negative and carries), carries through every
    window, the ends of the range"""
    byt = lambda b: sum(b << (8 * i) for i in range(32))      # noqa: E731
    v = [0, 1, 2, 127, 128, 129, 255, 256, SUBORDER - 1, SUBORDER - 2, (SUBORDER - 1) // 2, 1 << 250, (1 << 250) - 1]
    v += [byt(b) % SUBORDER for b in (0x7f, 0x80, 0x81, 0xff, 0x01)] + [byt(b) % (1 << 250) for b in (0x7f, 0x80, 0x81, 0xff)]
    v += [d << (8 * w) for w in (0, 1, 15, 30) for d in (1, 127, 128, 129, 255)]
    rnd = random.Random(0xFB5CA1A)
    v += [rnd.randrange(SUBORDER) for _ in range(8)]
    assert all(0 <= x < SUBORDER for x in v)
    return dedup(v)


_CACHE = {}


def edge_set(op):
    if op not in _CACHE:
        _CACHE[op] = _edge_set(op)
    return _CACHE[op]


def _edge_set(op):  # noqa: C901
    pts = edge_points()
    rnd = random.Random(0x40AD + OPS[op])
    if op in ("dbl", "entry"):
        return [(e,) for e in cr._ext_all()]
    if op in ("dbl4", "table"):
        out = [(e,) for p in pts for e in ext_reps(p, False, rnd)]
        if op == "table":                                    # every representation of the points with X = 0, Y = 0 (T = 0 in both)
            out += [(e,) for p in pts if p[0] == 0 or p[1] == 0 for e in ext_reps(p)]
        return dedup(out)
    if op == "add":
        # curve_ref's set of ext_add_pn: P + (-P), P + P, P + O for every edge point (O + O among them), every ordered pair of
        # edge points, every representation of P and of the entry -- the negation now the loader's, the slots taken in turn
        out = []
        for i, (a, b) in enumerate(cr.edge_set("addpn")):
            out.append((a, _pn_rec(b[:36], 1 + i % 8 if b[36] else i % 9, b[36])))
        # the entries qfb_load hands on: canonical, z2 = 2 (2^261 mod r) unreduced; and digit 0 with the sign set (no negation)
        for i, p in enumerate(pts):
            for j, q in enumerate(pts):
                c = cr.pniels_coords(q, 1)
                e = _coord_reps(c[:3], 0) + nform(TWO_R1)
                out.append((ext_reps(p, False, rnd)[(i + j) % 4], _pn_rec(e, 1 + (i + j) % 8, (i ^ j) & 1)))
            out.append((ext_reps(p, False, rnd)[i % 4], _pn_rec(IDENT_ENTRY, 0, i & 1)))
            out.append((ext_reps(p, False, rnd)[i % 4], _pn_rec(cr.to_pniels_model(ext_reps(p, False, rnd)[0]), 0, 1)))
        return dedup(out)
    if op in ("lift_t", "lift"):
        out = []
        for p in pts:
            ents = [n for z in edge_zs(p) for n in cr.pniels_reps(p, z, (0, 15, rnd.randrange(1, 15)))]
            ents += [cr.to_pniels_model(e) for e in ext_reps(p)]
            ents.append(_coord_reps(cr.pniels_coords(p, 1)[:3], 0) + nform(TWO_R1))
            for i, n in enumerate(ents):
                out += [(_pn_rec(n, 1 + i % 8, 1),), (_pn_rec(n, i % 9, 0),)]
        out += [(_pn_rec(IDENT_ENTRY, 0, s),) for s in (0, 1)]      # what an item shorter than jw lifts
        return dedup(out)
    if op == "from_ref":
        out = []
        for p in pts:
            x, y = cr.from_m1(p)
            xs = reps(x) + [nform(4 * R_MOD - lval(v)) for v in reps(-x % R_MOD)]        # fr_neg of either representative of -x
            out += [(a, b) for a in xs for b in reps(y)]
        return dedup(out)
    if op == "walk":
        sc = scalar_edges()
        out = []
        for p in pts:
            full, few = ext_reps(p), ext_reps(p, False, rnd)
            out += [(few[(j * 7) % len(few)], words(s) + (64,)) for j, s in enumerate(sc)]
            out += [(e, words(sc[(i * 5) % len(sc)]) + (64,)) for i, e in enumerate(full)]
        return dedup(out)
    if op == "walk_joint":
        out = []
        pl = pool()
        for i, p in enumerate(pts):
            few = ext_reps(p, False, rnd)
            for j, bu in enumerate(PAIR_BITS):
                for k, bv in enumerate(PAIR_BITS):
                    q = pts[(i + j + k) % len(pts)] if (j + k) & 1 else pl[(i * 7 + j + k) % len(pl)]
                    u, v = _bits_scalar(rnd, bu), _bits_scalar(rnd, bv)
                    if k == j:
                        q, v = (p, u) if j & 1 else (neg(p), u)           # u P + u P and u P - u P: the sum doubles, or vanishes
                    e2 = ext_reps(q, False, rnd)[(i + k) % 4]
                    out.append((few[(j + k) % len(few)] + e2, words(u) + words(v) + (need_of(max(bu, bv)),)))
        return dedup(out)
    if op == "affine":
        out = [(e,) for p in pts for e in ext_reps(p)]
        # coordinate quotients 0, 1 and r - 1 in both outputs (no points of the curve: x = 1 / F is on it for no y here)
        for x in (0, 1, R_MOD - 1):
            for y in (0, 1, R_MOD - 1):
                for z in (1, R_MOD - 1, rnd.randrange(2, R_MOD), RINV, (R_MOD - 1) * RINV % R_MOD):
                    c = (F * x * z % R_MOD, y * z % R_MOD, z, 0)
                    out += [(_coord_reps(c, m),) for m in range(16)]
        return dedup(out)
    if op == "is_identity":
        out = [(e,) for p in pts for e in ext_reps(p, False, rnd)]
        zs = dedup([1, R_MOD - 1, rnd.randrange(2, R_MOD), RINV, (R_MOD - 1) * RINV % R_MOD] + [z for p in pts[:3] for z in edge_zs(p)])
        for z in zs:
            zr = reps(z)
            for X in (0, R_MOD):                             # (0 : z : z), X as 0 and as r, Y and Z in either representative
                out += [(nform(X) + y + zz + nform(0),) for y in zr for zz in zr]
            m = mont(z)
            for zz in zr:                                    # the near misses
                out.append((nform(1) + zz + zz + nform(0),))                                   # X = 1
                out.append((nform(R_MOD + 1) + zz + zz + nform(0),))
                out.append((nform(0) + nform(m + 1) + zz + nform(0),))                         # Y = Z + 1
                out.append((nform(0) + nform((m - 1) % R_MOD + R_MOD) + zz + nform(0),))       # Y = Z - 1
                out += [(nform(X) + y + zz + nform(0),) for X in (0, R_MOD) for y in reps(-z % R_MOD)]      # Y = -Z: the order-2 point
        return dedup(out)
    if op == "fb_load":
        return [((s, sg),) for s in range(FB_SLOTS) for sg in (0, 1)]
    if op == "fb_mul":
        return [(words(s),) for s in fb_scalar_edges()]
    if op == "fb_add":
        out = []
        for i, s in enumerate(fb_scalar_edges()):
            for p in (pts[i % len(pts)], (0, 1), cr.g0_point(-LOG_B8 * s), cr.g0_point(LOG_B8 * s)):      # any, O, -s B8, s B8
                out.append((words(s), ext_reps(p, False, rnd)[i % 4]))
        return dedup(out)
    raise ValueError(op)


def random_set(op, rnd, n):  # noqa: C901
    pl = pool()
    pick = lambda: pl[rnd.randrange(len(pl))]                 # noqa: E731
    if op in ("dbl", "dbl4", "entry", "table", "affine"):
        return [(cr._rand_ext(rnd, pick()),) for _ in range(n)]
    if op == "is_identity":
        out = []
        for _ in range(n):
            p = (0, 1) if rnd.randrange(4) == 0 else pick()
            out.append((cr._rand_ext(rnd, p),))
        return out
    if op == "add":
        out = []
        for _ in range(n):
            p, q = cr._rand_pair(rnd)
            sg = rnd.randrange(2)
            out.append((cr._rand_ext(rnd, p), _pn_rec(cr._rand_entry(rnd, q, True), rnd.randrange(1, 9) if sg else rnd.randrange(9), sg)))
        return out
    if op in ("lift_t", "lift"):
        return [(_pn_rec(cr._rand_entry(rnd, pick(), True), rnd.randrange(9), rnd.randrange(2)),) for _ in range(n)]
    if op == "from_ref":
        out = []
        for _ in range(n):
            x, y = cr.from_m1(pick())
            xl = cr._rand_rep(rnd, x) if rnd.randrange(2) else nform(4 * R_MOD - lval(cr._rand_rep(rnd, -x % R_MOD)))
            out.append((xl, cr._rand_rep(rnd, y)))
        return out
    if op == "walk":
        out = []
        for _ in range(n):
            if rnd.randrange(4):
                s, need = cr._rand_scalar(rnd, 1 << 254), 64
            else:
                bits = rnd.randint(1, 252)
                s, need = rnd.getrandbits(bits), need_of(bits)
            out.append((cr._rand_ext(rnd, pick()), words(s) + (need,)))
        return out
    if op == "walk_joint":
        out = []
        for _ in range(n):
            p, q = cr._rand_pair(rnd)
            bits = rnd.choice((rnd.randint(1, 252), rnd.randint(120, 132), 127))
            u, v = rnd.getrandbits(bits), rnd.getrandbits(rnd.randint(1, bits))
            if rnd.randrange(2):
                u, v = v, u
            out.append((cr._rand_ext(rnd, p) + cr._rand_ext(rnd, q), words(u) + words(v) + (need_of(bits),)))
        return out
    if op == "fb_load":
        return [((rnd.randrange(FB_SLOTS), rnd.randrange(2)),) for _ in range(n)]
    if op == "fb_mul":
        return [(words(cr._rand_scalar(rnd, SUBORDER)),) for _ in range(n)]
    if op == "fb_add":
        return [(words(cr._rand_scalar(rnd, SUBORDER)), cr._rand_ext(rnd, pick() if rnd.randrange(8) else (0, 1))) for _ in range(n)]
    raise ValueError(op)


def padded(items):
    """the items, the first ones repeated until there are more than 64 and no multiple of 16: more than one workgroup of 16
    items (and of the lane harness's 64), a partly filled last one"""
    out = list(items)
    k = 0
    while len(out) <= 64 or len(out) % 16 == 0:
        out.append(items[k % len(items)])
        k += 1
    return out


# ---- domains -----------------------------------------------------------------------------------------------------------------
def _coord(l):
    return cr._isn(l, 2 * R_MOD)


def _entry_ok(n):
    ymx, ypx, t2d, z2 = split(n, 4)
    return (cr._isn(ymx, 6 * R_MOD) and cr._isn(ypx, 4 * R_MOD) and cr._isn(t2d, 2 * R_MOD) and cr._isn(z2, 4 * R_MOD)
            and cr.pniels_valid(n))


def _w32(w):
    return all(0 <= x < 1 << 32 for x in w)


def in_domain(op, item):  # noqa: C901
    wa, wb, _ = WIDTHS[op]
    a = item[0]
    b = item[1] if len(item) > 1 else None
    if len(a) != wa or (b is None) != (wb == 0) or (b is not None and len(b) != wb):
        return False
    if op in ("dbl", "dbl4", "entry", "table"):
        return cr._ext_ok(a)
    if op == "add":
        return cr._ext_ok(a) and _entry_ok(b[:36]) and 0 <= b[36] <= 8 and b[37] in (0, 1)
    if op in ("lift_t", "lift"):
        return _entry_ok(a[:36]) and 0 <= a[36] <= 8 and a[37] in (0, 1)
    if op == "from_ref":
        return cr._isn(a, 4 * R_MOD + 1) and _coord(b)
    if op == "walk":
        return cr._ext_ok(a) and _w32(b[:8]) and 1 <= b[8] <= 64 and fr.wval(b[:8]) < 1 << (4 * b[8] - 2)
    if op == "walk_joint":
        return (cr._ext_ok(a[:36]) and cr._ext_ok(a[36:]) and _w32(b[:16]) and 1 <= b[16] <= 64
                and max(fr.wval(b[:8]), fr.wval(b[8:16])) < 1 << (4 * b[16] - 2))
    if op == "affine":
        return all(_coord(c) for c in split(a, 4)) and cr.plain(a[18:27]) != 0
    if op == "is_identity":
        return all(_coord(c) for c in split(a, 4))
    if op == "fb_load":
        return 0 <= a[0] < FB_SLOTS and a[1] in (0, 1)
    if op == "fb_mul":
        return _w32(a) and fr.wval(a) < SUBORDER
    if op == "fb_add":
        return _w32(a) and fr.wval(a) < SUBORDER and cr._ext_ok(b)
    raise ValueError(op)


# ---- records and checks --------------------------------------------------------------------------------------------------------
def records(op, items):
    wa, wb, _ = WIDTHS[op]
    a = np.array([it[0] for it in items], dtype=np.uint64).astype(np.uint32).reshape(len(items), wa)
    b = np.array([it[1] for it in items], dtype=np.uint64).astype(np.uint32).reshape(len(items), wb) if wb else None
    return a, b


def lane_records(op, items):
    """the records of the lane op LANE_OP[op] for the same items: the sign the loader applies (none on digit 0) as the lane op's
    `neg` word"""
    a, b = records(op, items)
    if op == "add":
        sg = ((b[:, 36] != 0) & (b[:, 37] != 0)).astype(np.uint32)
        return a, np.concatenate([b[:, :36], sg[:, None]], axis=1)
    if op in ("lift_t", "lift"):
        sg = ((a[:, 36] != 0) & (a[:, 37] != 0)).astype(np.uint32)
        return np.concatenate([a[:, :36], sg[:, None]], axis=1), None
    return a, b


def negated_entries(ent):
    """(n, 36) stored entries -> what the loader makes of them on a negative digit: ymx and ypx swapped, 4r - t2d limb by limb"""
    ent = np.asarray(ent, dtype=np.uint32)
    out = ent.copy()
    out[:, 0:9], out[:, 9:18] = ent[:, 9:18], ent[:, 0:9]
    out[:, 18:27] = np.array(C4, dtype=np.uint32)[None, :] - ent[:, 18:27]
    return out


def table_from_lane(lane_out):
    """the lane op `table`'s nine entries (n, 324) laid out as the quad op lays its seventeen out: d = -8 .. 8"""
    lane_out = np.asarray(lane_out, dtype=np.uint32)
    cols = [negated_entries(lane_out[:, 36 * k:36 * k + 36]) for k in range(8, 0, -1)] + [lane_out]
    return np.concatenate(cols, axis=1)


def wave_jw(items, pos=-1):
    """the window count of every item's wave: the largest `need` among the 16 items of its workgroup"""
    need = [it[1][pos] for it in items]
    return [max(need[i - i % 16:i - i % 16 + 16]) for i in range(len(items))]


def _vals_ok(O, i, want, nel=4):
    """the raw values of an output record against the model's, value for value, N-form"""
    if not all(O.low[k][i] for k in range(nel)):
        return "a limb of 30 bits or more"
    got = tuple(O.raw[k][i] for k in range(nel))
    if got != tuple(want):
        return "raw values %s, want %s" % (got, tuple(want))
    return None


def _point_out(O, i, want, need_t=True):
    """an output Ext against the projective point `want`: N-form below 2r, the point, T Z == X Y (or T the zero limbs)"""
    return cr._ext_out(O, i, want, need_t)


def check(op, items, out):  # noqa: C901
    """indices (with a reason) where the op's output is not what the integers say"""
    a, b = records(op, items)
    out = np.asarray(out, dtype=np.uint32)
    n = len(items)
    assert out.shape == (n, WIDTHS[op][2]), (op, out.shape)
    bad = []

    def note(i, why):
        if why:
            bad.append((i, why))
    if op in ("dbl", "dbl4", "add", "entry", "lift_t", "lift"):
        O = _Rows(out, 4)
        bound = (6, 4, 2, 4) if op == "entry" else (2, 2, 2, 2)
        for i in range(n):
            c = raws(items[i][0][:36], 4)
            if op == "dbl":
                want = dbl_model(c)
            elif op == "dbl4":
                want = dbl_model(dbl_model(dbl_model(dbl_model(c))))
            elif op == "entry":
                want = entry_model(c)
            else:
                rec = items[i][1] if op == "add" else items[i][0]
                e = load_model(raws(rec[:36], 4), bool(rec[36] and rec[37]))
                want = add_model(c, e) if op == "add" else lift_model(e, op == "lift_t")
            why = _vals_ok(O, i, want)
            if not why and not all(O.raw[k][i] < bound[k] * R_MOD for k in range(4)):
                why = "a component beyond its bound"
            note(i, why)
    elif op == "from_ref":
        X, Y, O = _Rows(a, 1), _Rows(b, 1), _Rows(out, 4)
        for i in range(n):
            x, y = X.raw[0][i], Y.raw[0][i]
            fx = mmul(x, F_M)
            why = _vals_ok(O, i, (fx, y, R1, mmul(fx, y)))
            if not why and not (O.raw[0][i] < 2 * R_MOD and O.raw[3][i] < 2 * R_MOD):
                why = "X or T not below 2r"
            note(i, why)
    elif op == "table":
        E = [_Rows(out, 4, 36 * k) for k in range(17)]
        for i in range(n):
            model = table_model(raws(items[i][0], 4))
            why = None
            for d in range(-8, 9):
                got = tuple(int(v) for v in out[i, 36 * (d + 8):36 * (d + 8) + 36])
                m = model[abs(d)]
                if d >= 0:
                    want = sum((nform(v) for v in m), ())
                    ok = all(E[d + 8].low[k][i] for k in range(4)) and m[0] < 6 * R_MOD and m[1] < 4 * R_MOD and m[2] < 2 * R_MOD and m[3] < 4 * R_MOD
                else:                                        # swapped, and 4r - t2d limb by limb: carry-less
                    want = nform(m[1]) + nform(m[0]) + tuple(c - x for c, x in zip(C4, nform(m[2]))) + nform(m[3])
                    ok = max(got[18:27]) <= 1 << 30
                if got != want or not ok:
                    why = "entry %d: %s, want %s" % (d, got, want)
                    break
            note(i, why)
    elif op in ("walk", "walk_joint"):
        O = _Rows(out, 4)
        jw = wave_jw(items)
        for i in range(n):
            if op == "walk":
                want = smul_known(cr.ext_affine(items[i][0]), fr.wval(items[i][1][:8]))
                need_t = jw[i] >= 2                          # quad_lift<false> leaves T the zero limbs; every quad_add computes it
            else:
                sc = items[i][1]
                want = padd(smul_known(cr.ext_affine(items[i][0][:36]), fr.wval(sc[:8])),
                            smul_known(cr.ext_affine(items[i][0][36:]), fr.wval(sc[8:16])))
                need_t = True
            why = _point_out(O, i, want, need_t)
            if not why and tuple(int(v) for v in out[i, 36:40]) != (jw[i],) * 4:
                why = "jw %s, want %d on the four lanes" % (out[i, 36:40].tolist(), jw[i])
            note(i, why)
    elif op == "affine":
        P = _Rows(a, 4)
        got = list(zip(fr.vals_of_words(out[:, :8]), fr.vals_of_words(out[:, 8:])))
        for i in range(n):
            X, Y, Z, _ = P.plain(i)
            zi = inv(Z)
            want = (X * zi * FINV % R_MOD, Y * zi % R_MOD)
            note(i, None if got[i] == want else "(%d, %d), want canonical (%d, %d)" % (got[i] + want))
    elif op == "is_identity":
        P = _Rows(a, 4)
        for i in range(n):
            X, Y, Z, _ = P.plain(i)
            want = int(X == 0 and Y == Z)
            note(i, None if int(out[i, 0]) == want else "verdict %d, want %d" % (out[i, 0], want))
    elif op == "fb_load":
        for i in range(n):
            slot, sg = items[i][0]
            ymx, ypx, t = fb_entry(slot)
            want = ((nform(ypx) + nform(ymx) + tuple(c - x for c, x in zip(C4, nform(t)))) if sg else (nform(ymx) + nform(ypx) + nform(t))) + nform(TWO_R1)
            got = tuple(int(v) for v in out[i])
            note(i, None if got == want else "slot %d sign %d: %s, want %s" % (slot, sg, got, want))
    elif op in ("fb_mul", "fb_add"):
        O = _Rows(out, 4)
        for i in range(n):
            want = cr.g0_mul(LOG_B8 * fr.wval(items[i][0]))
            if op == "fb_add":
                X, Y, Z, _ = (cr.plain(c) for c in split(items[i][1], 4))
                want = padd((X, Y, Z), want)
            note(i, _point_out(O, i, want, True))
    else:
        raise ValueError(op)
    return bad
