"""Plain-integer model of the baby-step table and of one item's walk in csrc/dlog.hpp, for tests/test_dlog_host.py and
tests/test_gpu_dlog_directed.py.  Python ints only; nothing is imported from the code under test or from oracle/.

The key of a point P = (x, y) is y in Montgomery form, y * 2^261 mod r (dlog_canon_y): the slot index is its low b + 2 bits, the tag
bits 32 .. 63 masked to tag_bits.  The table holds j * G for j = 0 .. 2^b in 2^(b+2) slots with linear probing.  WHICH slot an entry
sits in depends on who came first; the SET of occupied slots does not (occupied()), and an entry sits between its home and the end
of its cluster.  So a walk that starts at index `idx` certainly meets every entry whose home lies between idx and the end of idx's
cluster -- whatever the insertion order -- and that is all this model ever claims about a table built by atomics on the device.
For the CPU program, which inserts j = 0, 1, 2, ... in turn, Table.layout() gives the very slots and refused_hits the exact count.

craft() makes curve points whose key has a chosen index and tag: a false tag hit by construction, with full 32-bit tags."""
import functools

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
A, D = 168700, 168696
MONT = 1 << 261
MONT_INV = pow(MONT, -1, R)
UINT64_MAX = (1 << 64) - 1


# ---- the curve A x^2 + y^2 = 1 + D x^2 y^2 ---------------------------------------------------------------------------------
def on_curve(P):
    x, y = P
    return (A * x * x + y * y - 1 - D * x * x * y * y) % R == 0


def add(P, Q):
    (x1, y1), (x2, y2) = P, Q
    t = D * x1 * x2 * y1 * y2 % R
    return ((x1 * y2 + y1 * x2) * pow(1 + t, -1, R) % R, (y1 * y2 - A * x1 * x2) * pow(1 - t, -1, R) % R)


def neg(P):
    return (-P[0] % R, P[1])


def mul(P, k):
    acc = (0, 1)
    for bit in bin(k)[2:]:
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, P)
    return acc


def _padd(P, Q):
    """projective (X, Y, Z), x = X / Z, y = Y / Z: the complete addition, no inversion"""
    (x1, y1, z1), (x2, y2, z2) = P, Q
    a = z1 * z2 % R
    b = a * a % R
    c = x1 * x2 % R
    d = y1 * y2 % R
    e = D * c * d % R
    f, g = (b - e) % R, (b + e) % R
    return (a * f * ((x1 + y1) * (x2 + y2) - c - d) % R, a * g * (d - A * c) % R, f * g % R)


def _ys(points):
    """the affine y of projective points, with one inversion for all of them"""
    pre, run = [], 1
    for _, _, z in points:
        pre.append(run)
        run = run * z % R
    inv = pow(run, -1, R)
    out = [0] * len(points)
    for i in range(len(points) - 1, -1, -1):
        out[i] = points[i][1] * inv * pre[i] % R
        inv = inv * points[i][2] % R
    return out


def sqrt_mod(v):
    """Tonelli-Shanks; None when v is no square"""
    v %= R
    if v == 0:
        return 0
    if pow(v, (R - 1) // 2, R) != 1:
        return None
    s, q = 0, R - 1
    while q % 2 == 0:
        s, q = s + 1, q // 2
    z = 2
    while pow(z, (R - 1) // 2, R) == 1:
        z += 1
    m, c, t, x = s, pow(z, q, R), pow(v, q, R), pow(v, (q + 1) // 2, R)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2, i = t2 * t2 % R, i + 1
        b = pow(c, 1 << (m - i - 1), R)
        m, c = i, b * b % R
        t, x = t * c % R, x * b % R
    assert x * x % R == v
    return x


# ---- keys ------------------------------------------------------------------------------------------------------------------
def key(P):
    return P[1] * MONT % R


def idx_of(k, b):
    return k & ((1 << (b + 2)) - 1)


def tag_of(k, tag_bits=32):
    return (k >> 32) & ((1 << tag_bits) - 1)


def craft(idx, tag, b, rng):
    """a curve point whose key has this index (low b + 2 bits) and this 32-bit tag (bits 32 .. 63); the other bits from rng
    (random.Random).  A key >= r is no key; y^2 must leave x^2 = (1 - y^2) / (A - D y^2) a square, which about half of them do."""
    assert 0 <= idx < (1 << (b + 2)) and 0 <= tag < (1 << 32)
    for _ in range(400):
        k = rng.getrandbits(254)
        k = (k & ~((1 << 64) - 1)) | (tag << 32) | (rng.getrandbits(32) & ~((1 << (b + 2)) - 1)) | idx
        if k >= R:
            continue
        y = k * MONT_INV % R
        den = (A - D * y * y) % R
        if den == 0:
            continue
        x = sqrt_mod((1 - y * y) * pow(den, -1, R))
        if x is None:
            continue
        P = (x, y)
        assert on_curve(P) and key(P) == k and idx_of(k, b) == idx and tag_of(k) == tag
        return P
    raise AssertionError("no point for this index and tag")


# ---- the table -------------------------------------------------------------------------------------------------------------
def occupied(homes, nslots, order=None):
    """the set of slots that linear probing fills with entries of these homes, inserted in `order`"""
    full = set()
    for e in (order if order is not None else range(len(homes))):
        s = homes[e]
        while s in full:
            s = (s + 1) % nslots
        full.add(s)
    return full


class Table:
    """j * G for j = 0 .. 2^b: keys, homes, the occupied slots, clusters"""

    def __init__(self, G, b):
        self.G, self.b, self.nslots, self.mask = G, b, 1 << (b + 2), (1 << (b + 2)) - 1
        pts, acc, g = [], (0, 1, 1), (G[0], G[1], 1)
        for _ in range((1 << b) + 1):
            pts.append(acc)
            acc = _padd(acc, g)
        self.ys = _ys(pts)
        self.keys = [y * MONT % R for y in self.ys]
        self.homes = [idx_of(k, b) for k in self.keys]
        self.j_of_y = {y: j for j, y in enumerate(self.ys)}
        assert len(self.j_of_y) == len(self.ys)                     # two different j never share y
        self.occ = occupied(self.homes, self.nslots)
        assert len(self.occ) == len(self.ys) < self.nslots
        self.neg_half = neg(mul(G, 1 << b))
        self.neg_stride = neg(mul(G, 2 << b))
        self._by_home = {}
        for j, h in enumerate(self.homes):
            self._by_home.setdefault(h, []).append(j)

    def run_from(self, idx):
        """the slots a walk from idx reads before the empty one that ends it, in order"""
        out, s = [], idx
        while s in self.occ:
            out.append(s)
            s = (s + 1) & self.mask
        return out

    def certain_after(self, idx):
        """the entries that a walk from idx meets whatever the insertion order was: those whose home the walk reads"""
        return [j for s in self.run_from(idx) for j in self._by_home.get(s, ())]

    def wraps(self, idx):
        run = self.run_from(idx)
        return bool(run) and run[-1] < run[0]

    def layout(self, order=None):
        """slot -> j for the given insertion order (default j = 0, 1, 2, ...: the CPU program's)"""
        slots = {}
        for j in (order if order is not None else range(len(self.homes))):
            s = self.homes[j]
            while s in slots:
                s = (s + 1) & self.mask
            slots[s] = j
        assert set(slots) == self.occ
        return slots

    def cut_point(self, i):
        return (1 << self.b) + i * (2 << self.b)


@functools.lru_cache(maxsize=None)
def table(G, b):
    return Table(G, b)


def steps_of(b, range_bits):
    return 1 if range_bits <= b + 1 else 1 << (range_bits - b - 1)


def walk_ys(P, T, nsteps):
    """y of Q_i = P - (2^b + i 2^(b+1)) G for i = 0 .. nsteps - 1"""
    q = _padd((P[0], P[1], 1), (T.neg_half[0], T.neg_half[1], 1))
    s = (T.neg_stride[0], T.neg_stride[1], 1)
    qs = []
    for _ in range(nsteps):
        qs.append(q)
        q = _padd(q, s)
    return _ys(qs)


def walk(P, G, b, range_bits, tag_bits, layout=None):
    """One item as dlog_step / dlog_confirm walk it -> (refused, end): refused = [(step, j)] of the candidates that confirmation
    refuses before the walk ends, end = (step, j) of the confirmed hit or None.  With a layout (Table.layout()) the walk is that of
    this very table; without one, refused holds only what is refused in every table of (G, b) -- entries homed at or behind the
    walk's index -- and the step of the true hit contributes nothing."""
    T = table(G, b)
    tmask = (1 << tag_bits) - 1
    refused = []
    for i, y in enumerate(walk_ys(P, T, steps_of(b, range_bits))):
        k = y * MONT % R
        idx, tag = idx_of(k, b), (k >> 32) & tmask
        true_j = T.j_of_y.get(y)
        if layout is not None:
            for s in T.run_from(idx):
                j = layout[s]
                if (T.keys[j] >> 32) & tmask == tag:
                    if j == true_j:
                        return refused, (i, j)
                    refused.append((i, j))
            assert true_j is None
        else:
            if true_j is not None:
                return refused, (i, true_j)
            refused += [(i, j) for j in T.certain_after(idx) if (T.keys[j] >> 32) & tmask == tag]
    return refused, None


def refused_hits(P, G, b, range_bits, tag_bits, layout=None):
    return len(walk(P, G, b, range_bits, tag_bits, layout)[0])


# ---- constructed false hits --------------------------------------------------------------------------------------------------
def tag_hits(P, T, range_bits):
    """[(step, j)] for every step of the item at which ANY entry of the table carries the 32-bit tag of Q_i, wherever it sits: a
    superset of the candidates the walk can meet, in every table of (G, b)"""
    by_tag = {}
    for j, k in enumerate(T.keys):
        by_tag.setdefault(tag_of(k), []).append(j)
    return [(i, j) for i, y in enumerate(walk_ys(P, T, steps_of(T.b, range_bits))) for j in by_tag.get(tag_of(y * MONT % R), ())]


def hit_sites(T):
    """Where a false hit can be planted so that the walk meets it in every table of (G, b), as (idx, e): a walk from idx stops at
    entry e.  first: idx opens a cluster and e alone is homed there, so e sits AT idx (probe offset 0).  behind: idx is the home of
    another entry and e is homed further along the same cluster, so the walk passes at least one foreign slot (offset > 0).
    wrapped: behind, with the end of the table between idx and the home of e."""
    first, behind, wrapped = [], [], []
    for idx in sorted(T._by_home):
        if (idx - 1) & T.mask not in T.occ and len(T._by_home[idx]) == 1:
            first.append((idx, T._by_home[idx][0]))
        for s in T.run_from(idx)[1:]:
            for e in T._by_home.get(s, ()):
                (wrapped if s < idx else behind).append((idx, e))
    return {"first": first, "behind": behind, "wrapped": wrapped}


def false_hit_item(T, step, idx, e, rng):
    """-> (P, Q): Q's key has index idx and the 32-bit tag of entry e, its y is no entry's, and P = Q + c_step G, so that giant step
    `step` of item P looks up Q"""
    while True:
        Q = craft(idx, tag_of(T.keys[e]), T.b, rng)
        if Q[1] not in T.j_of_y:
            break
    P = add(Q, mul(T.G, T.cut_point(step)))
    assert on_curve(P)
    return P, Q


def wrapped_base(B, b, first=161, tries=4000):
    """k and the table of k * B, k >= first, whose probe runs cross the end of the table with an entry homed on either side"""
    for k in range(first, first + tries):
        T = table(mul(B, k), b)
        if T.mask in T._by_home and hit_sites(T)["wrapped"]:
            return k, T
    raise AssertionError("no base with a wrapped probe run")


def false_hit_items(T, range_bits, extra_steps, rng, kinds=("first", "behind")):
    """One item per step and kind of site: the first two giant steps, a middle one, the last of the range, `extra_steps` (those below
    the number of steps), and one step beyond the range, whose hit is never reached -> [dict(P, Q, step, idx, e, kind)]"""
    n = steps_of(T.b, range_bits)
    steps = sorted({s for s in [0, 1, n // 2, n - 1] + list(extra_steps) if 0 <= s < n}) + [n]
    sites, out = hit_sites(T), []
    for kind in kinds:
        assert sites[kind], kind
        for k, step in enumerate(steps):
            idx, e = sites[kind][(k * 7) % len(sites[kind])]
            P, Q = false_hit_item(T, step, idx, e, rng)
            out.append(dict(P=P, Q=Q, step=step, idx=idx, e=e, kind=kind))
    return out


def assert_false_hit(T, it, range_bits):
    """what the model proves of a constructed item: at its step, and at no other step of the range, Q_i shares index-run and 32-bit
    tag with an entry -- e, which the walk from idx meets in every table of (G, b) -- while its y is no entry's; so the walk has
    exactly that candidate to refuse and never a hit to confirm.  That P has NO logarithm in the range is not claimed here."""
    n = steps_of(T.b, range_bits)
    P, Q, step, idx, e = it["P"], it["Q"], it["step"], it["idx"], it["e"]
    assert len({tag_of(k) for k in T.keys}) == len(T.keys)          # no second entry can stop the walk before e
    assert idx_of(key(Q), T.b) == idx and tag_of(key(Q)) == tag_of(T.keys[e]) and Q[1] != T.ys[e] and Q[1] not in T.j_of_y
    assert e in T.certain_after(idx)
    if it["kind"] == "first":
        assert T.run_from(idx)[0] == idx == T.homes[e] and (idx - 1) & T.mask not in T.occ
    else:
        assert T.homes[e] != idx and idx in T._by_home
    if it["kind"] == "wrapped":
        assert T.homes[e] < idx and T.wraps(idx)
    assert walk_ys(P, T, step + 1)[step] == Q[1]
    want = [(step, e)] if step < n else []
    assert tag_hits(P, T, range_bits) == want
    assert walk(P, T.G, T.b, range_bits, 32) == (want, None)
    return len(want)
