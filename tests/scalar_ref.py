"""Integer restatements and input sets for the scalar arithmetic of the library: integers mod l and mod 8l, the Montgomery
products mod l (fl_mul), the signers' wide reductions and the half-size pair (u, v) of the EdDSA fast path.  Shared by
tests/test_emul_bodies.py (the g++ build of the kernel bodies) and tests/test_gpu_scalar_fuzz.py (the same bodies on the
device, tests/devfuzz/scalar.hip).  A plain helper module: no fixtures, no pytest hooks.

Records are numpy uint32 arrays, one row per item, in the layout of tests/devfuzz/scalar_ops.hpp."""
import random
from fractions import Fraction

import numpy as np

R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
ORDER = 8 * L
RADIX = 1 << 261
RADIX_INV = pow(RADIX, -1, L)
L_R1, L_R2 = RADIX % L, (RADIX * RADIX) % L
M29 = (1 << 29) - 1

# op codes and record widths of tests/devfuzz/scalar_ops.hpp
OPS = dict(mod_l=0, mod_order=1, plain_mod_l=2, fl_mul=3, fl_canon4=4, digest=5, nonce=6, wide=7, verify_c=8, short_pair=9,
           euclid=10)
A_WORDS = dict(fl_mul=9, fl_canon4=9, digest=16, nonce=32, euclid=32)
B_WORDS = dict(fl_mul=9, verify_c=9)
OUT_WORDS = dict(fl_mul=9, fl_canon4=9, short_pair=17, euclid=18)
WIDE_WORD_COUNTS = list(range(8, 1025, 8))   # scalar_bytes: a multiple of 32 up to BJJ_MAX_SCALAR_BYTES = 4096


def a_words(op, nw=0):
    return nw if op == "wide" else A_WORDS.get(op, 8)


# ---- records ---------------------------------------------------------------------------------------------------------------
def words(vals, nw):
    """ints (each < 2^(32 nw)) -> (n, nw) uint32 little-endian words"""
    b = b"".join(int(v).to_bytes(4 * nw, "little") for v in vals)
    return np.frombuffer(b, dtype="<u4").reshape(len(vals), nw).astype(np.uint32)


def ints_of(arr):
    """(n, k) uint32 words -> ints"""
    arr = np.ascontiguousarray(arr, dtype="<u4")
    k = arr.shape[1]
    b = arr.tobytes()
    return [int.from_bytes(b[i:i + 4 * k], "little") for i in range(0, len(b), 4 * k)]


def nform(v):
    """N-form limbs of v < 2^264: limbs 0..7 < 2^29, the rest in limb 8"""
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def limbs(vals):
    return np.array([nform(v) for v in vals], dtype=np.uint32).reshape(len(vals), 9)


def limb_value(row, signed_top=False):
    top = int(row[8])
    if signed_top and top >= 1 << 31:
        top -= 1 << 32
    return sum(int(row[i]) << (29 * i) for i in range(8)) + (top << 232)


def is_nform(row):
    return all(int(x) <= M29 for x in row)


def dedup(vals):
    seen, out = set(), []
    for v in vals:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def rand_bits(rnd, n, maxbits):
    """n ints of random bit length 1..maxbits (uniform length, then uniform value), seeded"""
    return [rnd.getrandbits(rnd.randint(1, maxbits)) for _ in range(n)]


# ---- edge sets (explicit inputs; the random halves are seeded by the callers) ---------------------------------------------
def edges_mod_l():
    v = [q * L + d for q in range(44) for d in (-1, 0, 1)]
    v += [(t << 248) + d for t in range(256) for d in (-1, 0, (1 << 248) - 1)]
    v += [(1 << 256) - 1]
    return dedup(x for x in v if 0 <= x < 1 << 256)


def edges_mod_order():
    v = [q * ORDER + d for q in range(6) for d in (-1, 0, 1)]
    v += [(1 << 254) - 1, (1 << 254) + 1, (1 << 256) - 1, (1 << 255), 32 * L, 16 * L, 48 * L, 56 * L]
    v += edges_mod_l()
    return dedup(x for x in v if 0 <= x < 1 << 256)


def edges_plain_mod_l():
    v = [q * L + d for q in range(9) for d in (-1, 0, 1)] + [R_MOD - 1, R_MOD - 2]
    return dedup(x for x in v if 0 <= x < R_MOD)


def edges_fl_mul():
    """(a, b) pairs at the precondition a*b < l*2^261 (a, b < 2^261) and the operands the call sites produce"""
    bound = L * RADIX - 1
    pairs = []
    bs = [L + 1, L + 2, 2 * L - 1, 2 * L, 4 * L, (1 << 252) - 1, 1 << 252, 1 << 255, (1 << 256) - 1, 1 << 256, (1 << 260) - 1,
          1 << 260, (1 << 261) - 1, RADIX - L]
    bs += [(1 << k) + d for k in range(252, 261) for d in (-1, 1)]
    rnd = random.Random(0x5CA1A)
    bs += [L + rnd.getrandbits(rnd.randint(1, 260)) for _ in range(200)]
    for b in bs:
        if L < b < RADIX:
            a = bound // b
            if a < RADIX:
                pairs += [(a, b), (b, a), (a - 1, b)]
    ones = (1 << 261) - 1            # all-ones 29-bit limbs
    for x in (0, 1, L - 1, L, 2 * L - 1, ones, 1 << 260, (1 << 256) - 1, (1 << 251) - 1):
        for y in (0, 1, L_R1, L_R2, L - 1, 2 * L - 1):
            if x * y <= bound:
                pairs += [(x, y), (y, x)]
    pairs += [(ones, L - 1), (ones, L_R1), (ones, L_R2), (2 * L - 1, 2 * L - 1), ((1 << 251) - 1, 2 * L - 1)]
    return dedup(p for p in pairs if p[0] * p[1] <= bound)


def edges_fl_canon4():
    v = [0, 1, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 3 * L - 1, 3 * L, 3 * L + 1, 4 * L - 1]
    return dedup(v)


def boundary_edges(nbits, cuts):
    """inputs < 2^nbits around the chunk boundaries `cuts`: all-ones and single-bit chunks on each side, 2^c +- 1, and
    multiples of l +- 1 that straddle each boundary"""
    top = (1 << nbits) - 1
    bounds = [0] + list(cuts) + [nbits]
    v = [0, 1, top, top - 1, 1 << (nbits - 1), L, L - 1, L + 1]
    for lo, hi in zip(bounds, bounds[1:]):
        v += [((1 << hi) - 1) ^ ((1 << lo) - 1), 1 << lo, 1 << (hi - 1), (1 << hi) - 1]   # one chunk all ones / single bits
    for c in cuts:
        v += [(1 << c) - 1, 1 << c, (1 << c) + 1, 1 << (c - 1), (1 << (c + 1)) - 1, top ^ ((1 << c) - 1), top ^ (1 << c),
              top >> (nbits - c), top ^ (top >> (nbits - c))]
        q0 = (1 << c) // L
        v += [q * L + d for q in range(max(q0 - 2, 0), q0 + 3) for d in (-1, 0, 1)]
        q1 = ((1 << c) - 1) // L       # the largest multiple below the boundary, and with every bit above set
        v += [(q1 * L) | (top ^ ((1 << c) - 1)), top - ((top - (1 << c)) % L)]
    qt = top // L
    v += [q * L + d for q in range(qt - 2, qt + 1) for d in (-1, 0, 1)]
    return dedup(x for x in v if 0 <= x <= top)


def edges_digest():
    return boundary_edges(512, [261])


def edges_nonce():
    return boundary_edges(1024, [261, 522, 783])


def edges_wide(nw):
    """inputs of nw words for wide_scalar_mod_order: all ones, q*8l +- 1, 2^(3 + 261 c) +- 1 at every chunk boundary"""
    nbits = 32 * nw
    top = (1 << nbits) - 1
    v = [0, 1, 7, 8, top, top - 7, top >> 1, ORDER - 1, ORDER, ORDER + 1]
    qt = top // ORDER
    v += [q * ORDER + d for q in (1, 2, 3, qt - 1, qt) for d in (-1, 0, 1)]
    c = 0
    while 3 + 261 * c < nbits:
        b = 3 + 261 * c
        v += [(1 << b) - 1, 1 << b, (1 << b) + 1, top ^ ((1 << b) - 1), (((1 << b) - 1) // ORDER) * ORDER]
        c += 1
    return dedup(x for x in v if 0 <= x <= top)


# ---- the half-size pair ---------------------------------------------------------------------------------------------------
def euclid_stop(kappa):
    """(r0, t0, r1, t1) of the classical extended Euclid on (l, kappa), stopped at the first r1 < 2^126 (t signed)"""
    r0, t0, r1, t1 = L, 0, kappa, 1
    while r1 >= (1 << 126):
        q = r0 // r1
        r0, r1, t0, t1 = r1, r0 - q * r1, t1, t0 - q * t1
    return r0, t0, r1, t1


def pair_bits(kappa):
    """bit length max(bits(u), bits(|v|)) of the pair lattice_short_pair must select -- an independent restatement of the
    selection rule: (r1, t1) if t1 is odd, else the better of the previous pair and the non-degenerate next pair"""
    r0, t0, r1, t1 = euclid_stop(kappa)
    if t1 % 2:
        return max(r1.bit_length(), abs(t1).bit_length())
    best = max(r0.bit_length(), abs(t0).bit_length())
    q = r0 // r1
    r2, t2 = r0 - q * r1, t0 - q * t1
    if r2:
        best = min(best, max(r2.bit_length(), abs(t2).bit_length()))
    return best


def pair_outcome(kappa):
    """which branch the selection takes: 'odd', 'prev', 'next' or 'degenerate' (t1 even and the next pair is r = 0)"""
    r0, t0, r1, t1 = euclid_stop(kappa)
    if t1 % 2:
        return "odd"
    q = r0 // r1
    r2, t2 = r0 - q * r1, t0 - q * t1
    if r2 == 0:
        return "degenerate"
    return "next" if max(r2.bit_length(), abs(t2).bit_length()) < max(r0.bit_length(), abs(t0).bit_length()) else "prev"


def _cf_value(quots):
    x = Fraction(0)
    for a in reversed(quots):
        x = 1 / (a + x)
    return x


def edges_short_pair():
    """kappa < l: (i) the edge kappa of test_emul_bodies.py, (ii) kappa around l/q, (iii) kappa whose continued fraction
    kappa/l starts with chosen partial quotients, placed so that the remainder crosses 2^126 at the large one, (iv) kappa
    whose stopping t1 is even, with the previous, the next and the degenerate next pair"""
    ks = [0, 1, 2, 3, L - 1, L - 2, (L + 1) // 2, (L - 1) // 2, 1 << 126, (1 << 126) - 1, (1 << 126) + 1, 1 << 250, L // 3,
          L - (1 << 126), (1 << 200) + 1]
    qs = [1, 2, 3] + [(1 << k) + d for k in range(2, 251) for d in (-1, 0, 1)]
    for q in qs:
        ks += [L // q, (L - 1) // q, -(-L // q)]
    big = [1, (1 << 29) - 1, 1 << 29, (1 << 29) + 1, (1 << 53) - 1, (1 << 53) + 1, 1 << 53, 1 << 100]
    rnd = random.Random(0xCF)
    for A in big:
        for filler in (1, 2, 3, 7):
            for shift in range(-3, 4):
                # denominators grow by ~filler per step: aim the crossing of 2^126 by the remainder at the large quotient
                prefix = []
                den = 1
                while den * A < (1 << 125) >> max(shift, 0) << max(-shift, 0):
                    prefix.append(filler)
                    den = _cf_value(prefix).denominator
                    if len(prefix) > 400:
                        break
                for tail in ([1], [2, 1], [rnd.randint(1, 1 << 20)], [(1 << 29) - 1, 3]):
                    x = _cf_value(prefix + [A] + tail + [rnd.randint(1, 9) for _ in range(60)])
                    ks.append(int(L * x.numerator // x.denominator))
    for A in big:                       # every partial quotient the same
        x = _cf_value([A] * max(2, 260 // max(A.bit_length(), 1)))
        ks.append(int(L * x.numerator // x.denominator))
    # (iv) even t1 at the stop: kappa = r * t^-1 mod l puts the pair (r, t) on the Euclid sequence (|r t| < l / 2)
    for bits in (1, 2, 3, 10, 29, 53, 64, 100, 120, 124):
        for j in range(6):
            t = (rnd.getrandbits(bits) | 1) << rnd.randint(1, 3)
            for r in (1, rnd.getrandbits(125) | (1 << 124), (1 << 126) - 1 - rnd.getrandbits(20), rnd.getrandbits(126 - bits)):
                for sgn in (1, -1):
                    ks.append(r * pow(sgn * t, -1, L) % L)
    ks += [(L - 1) // q for q in (2, 4, 6, 8, 10, 12, 16, 20, 22, 24, 30, 34, 40, 44)]   # l mod kappa = 1: degenerate next pair
    return dedup(k % L for k in ks)


def edges_verify_c():
    """(s, |v|, neg): s at the mod-l boundary set, |v| from 1 to 250 bits (and the |v| of kappa = (l + 1)/2), both signs"""
    r0, t0, r1, t1 = euclid_stop((L + 1) // 2)
    vmax = abs(t1) if t1 % 2 else abs(t0)
    vs = [1, 3, vmax, L - 2 if (L - 2) % 2 else L - 4] + [(1 << b) - 1 for b in range(2, 251, 3)] + [(1 << b) + 1 for b in range(1, 250, 7)]
    vs = [v for v in vs if v < 1 << 250 or v == vmax]
    ss = edges_mod_l()
    return [(s, v, neg) for s in ss for v in vs for neg in (0, 1)]


def edges_euclid():
    """(r0, r1, t0, t1) with r0 = q r1 + delta, delta in {0, 1, r1 - 1}, r1 of 1..251 bits -- including r1 whose top 54 bits
    round UP in f64 -- and q at the 29-bit digit boundaries, the 53-bit mantissa and far beyond"""
    qs = [1, 2, (1 << 29) - 1, 1 << 29, (1 << 29) + 1, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, 1 << 58, 1 << 100, 1 << 249,
          (1 << 58) - 1, (1 << 87) - 1, 1 << 87, 3 << 28]
    rnd = random.Random(0xE0C1)
    r1s = []
    for b in list(range(1, 60)) + list(range(60, 252, 3)) + [251]:
        r1s += [(1 << b) - 1, 1 << (b - 1), (1 << (b - 1)) + 1, rnd.getrandbits(b) | (1 << (b - 1))]
        if b > 54:   # top 54 bits 1...1 (53 ones, then a one): rounds up to 2^b in f64
            r1s += [((1 << 54) - 1) << (b - 54), (((1 << 54) - 1) << (b - 54)) | rnd.getrandbits(b - 54)]
            r1s += [(((1 << 53) + 1) << (b - 54)) | 1]   # ...0 1 then a one: rounds up past the tie
    out = []
    for r1 in dedup(x for x in r1s if x > 0):
        for q in qs:
            for d in (0, 1, r1 - 1):
                r0 = q * r1 + d
                if r0 >= 1 << 252:
                    continue
                tb = max(1, 250 - q.bit_length())          # t0 + q t1 < 2^251
                t1 = rnd.getrandbits(rnd.randint(1, tb)) | 1
                t0 = rnd.getrandbits(rnd.randint(1, tb))
                out.append((r0, r1, t0, t1))
    return out


def random_euclid(rnd, n):
    out = []
    while len(out) < n:
        b1 = rnd.randint(1, 251)
        r1 = rnd.getrandbits(b1) | (1 << (b1 - 1))
        qb = rnd.randint(1, 252 - b1) if b1 < 252 else 1
        q = max(1, rnd.getrandbits(qb))
        d = rnd.randrange(r1)
        r0 = q * r1 + d
        if r0 >= 1 << 252:
            continue
        tb = max(1, 250 - q.bit_length())
        out.append((r0, r1, rnd.getrandbits(rnd.randint(1, tb)), rnd.getrandbits(rnd.randint(1, tb)) | 1))
    return out


# ---- records for the ops (a, b) and checks of the outputs against Python integers ----------------------------------------
def records(op, items, nw=0):
    """(a, b) uint32 records for `items` (ints, or tuples for fl_mul / verify_c / euclid)"""
    if op in ("mod_l", "mod_order", "plain_mod_l", "short_pair"):
        return words(items, 8), None
    if op in ("digest", "nonce", "wide"):
        return words(items, a_words(op, nw)), None
    if op == "fl_canon4":
        return limbs(items), None
    if op == "fl_mul":
        return limbs([a for a, _ in items]), limbs([b for _, b in items])
    if op == "verify_c":
        b = np.concatenate([words([v for _, v, _ in items], 8), np.array([[g] for _, _, g in items], dtype=np.uint32)], axis=1)
        return words([s for s, _, _ in items], 8), b
    if op == "euclid":
        return np.concatenate([words([x[j] for x in items], 8) for j in range(4)], axis=1), None
    raise ValueError(op)


def check(op, items, out):
    """indices (with a reason) where the op's output is not what the integers say"""
    bad = []
    if op in ("mod_l", "digest", "nonce"):
        for i, (x, y) in enumerate(zip(items, ints_of(out))):
            if y != x % L:
                bad.append((i, "want %d" % (x % L)))
    elif op in ("mod_order", "wide"):
        for i, (x, y) in enumerate(zip(items, ints_of(out))):
            if y != x % ORDER:
                bad.append((i, "want %d" % (x % ORDER)))
    elif op == "plain_mod_l":
        for i, (x, y) in enumerate(zip(items, ints_of(out))):
            if y != x % L:
                bad.append((i, "want %d" % (x % L)))
    elif op == "fl_canon4":
        for i, x in enumerate(items):
            if not is_nform(out[i]) or limb_value(out[i]) != x % L:
                bad.append((i, "fl_canon4"))
    elif op == "fl_mul":
        for i, (a, b) in enumerate(items):
            y = limb_value(out[i])
            if not is_nform(out[i]) or y >= 2 * L or (y - a * b * RADIX_INV) % L:
                bad.append((i, "fl_mul"))
    elif op == "verify_c":
        for i, ((s, v, neg), y) in enumerate(zip(items, ints_of(out))):
            want = ((-v if neg else v) * s) % L
            if y != want:
                bad.append((i, "want %d" % want))
    elif op == "short_pair":
        for i, k in enumerate(items):
            u, v = ints_of(out[i:i + 1, 0:8])[0], ints_of(out[i:i + 1, 8:16])[0]
            neg = int(out[i, 16])
            sv = -v if neg else v
            if neg not in (0, 1) or (u - sv * k) % L or v % 2 != 1 or v % L == 0 or max(u.bit_length(), v.bit_length()) != pair_bits(k):
                bad.append((i, "kappa %d: u %d v %d" % (k, u, sv)))
    elif op == "euclid":
        for i, (r0, r1, t0, t1) in enumerate(items):
            r0n, t0n = limb_value(out[i, 0:9], True), limb_value(out[i, 9:18], True)
            qd = r0 - r0n
            if r0n < 0 or qd % r1 or not 1 <= qd // r1 <= r0 // r1 or t0n != t0 + (qd // r1) * t1:
                bad.append((i, "r0 %d r1 %d: q %s of %d" % (r0, r1, Fraction(qd, r1), r0 // r1)))
    else:
        raise ValueError(op)
    return bad


def cpu_run(emul, op, a, b, nw=0):
    """the op on the CPU harness (tests/emul: emul_scalar_op, the g++ build of scalar_ops.hpp) -> (n, out words) uint32"""
    import ctypes
    n = a.shape[0]
    assert a.shape[1] == a_words(op, nw) and (b is None or b.shape == (n, B_WORDS[op]))
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = None if b is None else np.ascontiguousarray(b, dtype=np.uint32)
    out = np.zeros((n, OUT_WORDS.get(op, 8)), dtype=np.uint32)
    vp = ctypes.c_void_p
    rc = emul.emul_scalar_op(ctypes.c_int(OPS[op]), a.ctypes.data_as(vp), None if b is None else b.ctypes.data_as(vp),
                             out.ctypes.data_as(vp), ctypes.c_size_t(n), ctypes.c_int(nw))
    assert rc == 0
    return out


EDGE_SETS = dict(mod_l=edges_mod_l, mod_order=edges_mod_order, plain_mod_l=edges_plain_mod_l, fl_mul=edges_fl_mul,
                 fl_canon4=edges_fl_canon4, digest=edges_digest, nonce=edges_nonce, verify_c=edges_verify_c, euclid=edges_euclid,
                 short_pair=edges_short_pair)


def edge_set(op):
    """the explicit inputs of one op but `wide` (its records depend on the word count)"""
    return EDGE_SETS[op]()


def edge_sets():
    """{op: items} of every op but `wide`, euclid BEFORE short_pair: a Euclid step whose quotient can be too large makes the
    loop of lattice_short_pair endless instead of failing, so a caller that walks these in order fails at the step first"""
    return {op: fn() for op, fn in EDGE_SETS.items()}


def random_set(op, rnd, n, nw=0):
    """n seeded random inputs for the op"""
    if op == "mod_l" or op == "mod_order":
        return [rnd.getrandbits(256) for _ in range(n // 2)] + rand_bits(rnd, n - n // 2, 256)
    if op == "plain_mod_l":
        return [rnd.randrange(R_MOD) for _ in range(n)]
    if op == "fl_canon4":
        return [rnd.randrange(4 * L) for _ in range(n)]
    if op == "fl_mul":
        out = []
        for _ in range(n):
            a = rnd.getrandbits(rnd.randint(1, 261))
            lim = min(RADIX, (L * RADIX - 1) // a + 1) if a else RADIX
            out.append((a, rnd.randrange(lim)))
        return out
    if op == "digest":
        return [rnd.getrandbits(512) for _ in range(n)]
    if op == "nonce":
        return [rnd.getrandbits(1024) for _ in range(n)]
    if op == "wide":
        return [rnd.getrandbits(32 * nw) for _ in range(n)]
    if op == "verify_c":
        return [(rnd.getrandbits(256), rnd.getrandbits(rnd.randint(1, 250)) | 1, rnd.getrandbits(1)) for _ in range(n)]
    if op == "short_pair":
        return [rnd.randrange(L) for _ in range(n)]
    if op == "euclid":
        return random_euclid(rnd, n)
    raise ValueError(op)
