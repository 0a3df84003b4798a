"""The plain-integer model of include/bjj_hip_dleq.h and its directed inputs; holds no tests.

The model is written once over a small arithmetic BACKEND -- mul(points, scalars), add(points, points), hash5(rows) on lists of
integers -- and has two of them: PyBackend over the pure-Python oracle (oracle/bjj_oracle.py: mul_scalar, proj_add, proj_affine,
poseidon; the module is handed in by the caller, the CPU tests take it from the `pyoracle` fixture) and CBackend over the C oracle
(conftest.Oracle), which is what the GPU tests use.  Everything else here is integers: the curve equation, the reductions, the
canonical-encoding rule, z = w' + c sk' mod l."""
import random

import numpy as np

Q = 21888242871839275222246405745257275088548364400416034343698204186575808495617       # r, the field
L = 2736030358979909402780800718157159386076813972158567259200215660948447373041         # l, the prime subgroup order
ORDER8 = 8 * L
A_REF, D_REF = 168700, 168696
B8 = (5299619240641551281634865583518297030282874472190772894086521144482721001553,
      16950150798460657717958625567821834550301663161624707787222815936182638968203)
M256 = (1 << 256) - 1
IDENTITY = (0, 1)
T2 = (0, Q - 1)                                                                          # the point of order 2


def on_curve(p):
    x, y = p[0] % Q, p[1] % Q
    return (A_REF * x * x + y * y - 1 - D_REF * x * x * y * y) % Q == 0


def red(p):
    return (p[0] % Q, p[1] % Q)


def neg(p):
    return ((Q - p[0]) % Q, p[1] % Q)


def le(v, size=32):
    return int(v).to_bytes(size, "little")


def pack_points(pts):
    return np.frombuffer(b"".join(le(x) + le(y) for x, y in pts), np.uint8).reshape(len(pts), 64).copy()


def pack_scalars(ks):
    return np.frombuffer(b"".join(le(k) for k in ks), np.uint8).reshape(len(ks), 32).copy()


def _bytes(a):
    return bytes(a) if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a, np.uint8).tobytes()


def unpack_points(a):
    b = _bytes(a)
    return [(int.from_bytes(b[i:i + 32], "little"), int.from_bytes(b[i + 32:i + 64], "little")) for i in range(0, len(b), 64)]


def unpack_scalars(a):
    b = _bytes(a)
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


# ---- the two backends ---------------------------------------------------------------------------------------------------------------
class PyBackend:
    """o: the pure-Python oracle module (mul_scalar, proj_add, proj_affine, poseidon)"""

    def __init__(self, o):
        self.o = o

    def mul(self, pts, ks):
        return [tuple(self.o.mul_scalar(p, k)) for p, k in zip(pts, ks)]

    def add(self, ps, qs):
        return [tuple(self.o.proj_affine(self.o.proj_add((*p, 1), (*q, 1)))) for p, q in zip(ps, qs)]

    def hash5(self, rows):
        return [self.o.poseidon(list(r)) for r in rows]


class CBackend:
    """o: conftest.Oracle, the C restatement of the reference (batched, threaded)"""

    def __init__(self, o):
        self.o = o

    def mul(self, pts, ks):
        return unpack_points(self.o.mul_var_base(pack_points(pts), pack_scalars(ks))) if len(pts) else []

    def add(self, ps, qs):
        return unpack_points(self.o.point_add(pack_points(ps), pack_points(qs))) if len(ps) else []

    def hash5(self, rows):
        if not len(rows):
            return []
        a = np.frombuffer(b"".join(le(v) for r in rows for v in r), np.uint8)
        return unpack_scalars(self.o.poseidon5(a))


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def mul_pair(be, P, a, Qp, b, A=None):
    """-> (out, ok): out[i] = A[i] + (a[i] mod 8l) P[i] + (b[i] mod 8l) Q[i], coordinates reduced mod r first; ok 2 and (0, 0) when P,
    Q or A fails the curve equation"""
    n = len(P)
    A = [IDENTITY] * n if A is None else A
    good = [on_curve(P[i]) and on_curve(Qp[i]) and on_curve(A[i]) for i in range(n)]
    idx = [i for i in range(n) if good[i]]
    t1 = be.mul([red(P[i]) for i in idx], [a[i] % ORDER8 for i in idx])
    t2 = be.mul([red(Qp[i]) for i in idx], [b[i] % ORDER8 for i in idx])
    s = be.add(be.add([red(A[i]) for i in idx], t1), t2)
    out, ok = [(0, 0)] * n, [2] * n
    for k, i in enumerate(idx):
        out[i], ok[i] = s[k], 1
    return out, ok


def challenge(be, tag, C1, D, A, B):
    """c = Poseidon5(Poseidon5(tag, C1, D), A, B), everything reduced mod r, as an integer below r"""
    h = be.hash5([(tag % Q, *red(c1), *red(d)) for c1, d in zip(C1, D)])
    return be.hash5([(h[i], *red(A[i]), *red(B[i])) for i in range(len(h))])


def dleq_tag(be, G, PK, label=0):
    return be.hash5([(*red(G), *red(PK), label % Q)])[0]


def dleq_verify(be, G, PK, tag, C1, D, A, B, z):
    """-> ok: 2 = C1 or D off the curve; else 0 = a coordinate of A or B >= r, z >= l, A or B off the curve, or an equation fails; 1"""
    n = len(C1)
    ok = [0] * n
    run = []
    for i in range(n):
        if not (on_curve(C1[i]) and on_curve(D[i])):
            ok[i] = 2
        elif max(*A[i], *B[i]) < Q and z[i] < L and on_curve(A[i]) and on_curve(B[i]):
            run.append(i)
    if not run:
        return ok
    c = challenge(be, tag, [C1[i] for i in run], [D[i] for i in run], [A[i] for i in run], [B[i] for i in run])
    k = len(run)
    lhs1 = be.mul([red(G)] * k, [z[i] for i in run])
    rhs1 = be.add([A[i] for i in run], be.mul([red(PK)] * k, c))
    lhs2 = be.mul([red(C1[i]) for i in run], [z[i] for i in run])
    rhs2 = be.add([B[i] for i in run], be.mul([red(D[i]) for i in run], c))
    for j, i in enumerate(run):
        ok[i] = 1 if lhs1[j] == rhs1[j] and lhs2[j] == rhs2[j] else 0
    return ok


def dleq_prove(be, G, sk, tag, C1, w):
    """-> (D, A, B, z, ok) with sk' = sk mod l, w' = w mod l; ok 2 and zeros for a C1 off the curve"""
    n = len(C1)
    skr = sk % L
    idx = [i for i in range(n) if on_curve(C1[i])]
    c1 = [red(C1[i]) for i in idx]
    wr = [w[i] % L for i in idx]
    Dp = be.mul(c1, [skr] * len(idx))
    Ap = be.mul([red(G)] * len(idx), wr)
    Bp = be.mul(c1, wr)
    c = challenge(be, tag, c1, Dp, Ap, Bp)
    D, A, B, z, ok = [(0, 0)] * n, [(0, 0)] * n, [(0, 0)] * n, [0] * n, [2] * n
    for k, i in enumerate(idx):
        D[i], A[i], B[i], z[i], ok[i] = Dp[k], Ap[k], Bp[k], (wr[k] + (c[k] % L) * skr) % L, 1
    return D, A, B, z, ok


# ---- directed inputs ----------------------------------------------------------------------------------------------------------------
EDGE_SCALARS = (0, 1, L, ORDER8 - 1, ORDER8, M256)


def world(be, torsion, seed=0xD1E0):
    """the points the directed sets are made of.  torsion: the eight points j T8 of tests/curve_ref.py (TORSION_REF), j = 0 .. 7"""
    rng = random.Random(seed)
    s1, s2, s3 = be.mul([B8] * 3, [rng.randrange(1, L) for _ in range(3)])
    full = be.add([s1], [tuple(torsion[1])])[0]                                            # order 8l
    gen = be.add([s2], [tuple(torsion[3])])[0]                                             # another one: the G of a custom table
    big = (s1[0] + Q, s1[1])
    assert big[0] <= M256 and on_curve(big) and not on_curve((s1[0] ^ 1, s1[1])) and not on_curve((0, 0))
    return {"s1": s1, "s2": s2, "s3": s3, "full": full, "gen": gen, "big": big, "off": (s1[0] ^ 1, s1[1]), "off_y": (s2[0], s2[1] ^ 4),
            "torsion": [tuple(t) for t in torsion], "b8": B8}


def pair_directed(be, W, seed=0xD1E1):
    """-> (P, a, Q, b, A, names): Q = P, Q = -P, a = b; sums that vanish and addends that cancel them; the edge scalars against each
    other; torsion points and the identity on every side; coordinates >= r; an off-curve P, Q, A, each alone; (0, 0) on each side"""
    rng = random.Random(seed)
    rs = lambda: rng.getrandbits(256)   # noqa: E731
    s1, s2, s3, full, big, tor = W["s1"], W["s2"], W["s3"], W["full"], W["big"], W["torsion"]
    rows = []

    def add(name, P, a, Qp, b, A=IDENTITY):
        rows.append((name, P, a, Qp, b, A))
    k = rs()
    add("Q=P", s1, rs(), s1, rs())
    add("Q=P full", full, rs(), full, rs(), s2)
    add("Q=-P", s1, rs(), neg(s1), rs())
    add("a=b", s1, k, s2, k)
    add("a=b Q=P", full, k, full, k)
    add("a=b Q=-P: O", full, k, neg(full), k)                                              # a P + b Q = O
    add("b=8l-a Q=P: O", full, 5, full, ORDER8 - 5, s3)
    add("a=b Q=-P: O, A=O", s2, k, neg(s2), k, IDENTITY)
    for a in EDGE_SCALARS:
        for b in EDGE_SCALARS:
            add("edge %x %x" % (a % 997, b % 997), full, a, s2, b, s1)
    add("edge no addend", s1, M256, full, ORDER8 - 1)
    for j in range(8):
        add("torsion P %d" % j, tor[j], rs(), s1, rs(), tor[(3 * j + 1) % 8])
        add("torsion Q %d" % j, full, rs(), tor[j], rs())
        add("torsion both %d" % j, tor[j], rs(), tor[(j + 5) % 8], rs(), tor[7 - j])
    add("identity everywhere", IDENTITY, rs(), IDENTITY, rs(), IDENTITY)
    add("x>=r in P", big, rs(), s2, rs(), s3)
    add("x>=r in Q", s2, rs(), big, rs())
    add("x>=r in A", s2, rs(), s3, rs(), big)
    add("y>=r", (0, 1 + Q), rs(), s1, rs(), (0, Q - 1 + Q))
    add("off P", W["off"], rs(), s2, rs(), s3)
    add("off Q", s1, rs(), W["off_y"], rs(), s3)
    add("off A", s1, rs(), s2, rs(), W["off"])
    add("(0,0) P", (0, 0), rs(), s2, rs(), s3)
    add("(0,0) Q", s1, rs(), (0, 0), rs())
    add("(0,0) A", s1, rs(), s2, rs(), (0, 0))
    P, a, Qp, b, A = ([r[i] for r in rows] for i in range(1, 6))
    # A = -(a P + b Q): the result is the identity
    base = [i for i, r in enumerate(rows) if r[0] in ("Q=P", "Q=P full", "a=b", "torsion P 3", "x>=r in P", "edge no addend")]
    sums, ok = mul_pair(be, [P[i] for i in base], [a[i] for i in base], [Qp[i] for i in base], [b[i] for i in base])
    assert ok == [1] * len(base)
    for i, s in zip(base, sums):
        rows.append(("A=-(aP+bQ) of " + rows[i][0], P[i], a[i], Qp[i], b[i], neg(s)))
    names = [r[0] for r in rows]
    return tuple([r[i] for r in rows] for i in range(1, 6)) + (names,)


def random_pair(be, W, n, seed):
    """n seeded items: points k B8 + j T8, scalars of 256 random bits -> (P, a, Q, b, A)"""
    rng = random.Random(seed)
    pts = be.add(be.mul([B8] * (3 * n), [rng.randrange(1, L) for _ in range(3 * n)]), [W["torsion"][rng.randrange(8)] for _ in range(3 * n)])
    return pts[:n], [rng.getrandbits(256) for _ in range(n)], pts[n:2 * n], [rng.getrandbits(256) for _ in range(n)], pts[2 * n:]


def dleq_directed(be, W, G, sk, sk2, tag, seed=0xD1E2):
    """The statement is PK = (sk mod l) G.  -> a list of (name, C1, D, A, B, z, pinned): valid proofs and one-field mutations.
    pinned: the verdict the contract states outright (None: whatever the model says); the caller checks the model against it."""
    rng = random.Random(seed)
    n = 12
    C1 = be.mul([B8] * n, [rng.randrange(1, L) for _ in range(n)])
    w = [rng.getrandbits(256) for _ in range(n)]
    w[3], w[4] = 0, L                                                                      # w == 0 (mod l): A = B = the identity
    D, A, B, z, ok = dleq_prove(be, G, sk, tag, C1, w)
    assert ok == [1] * n and A[3] == IDENTITY and B[4] == IDENTITY
    D2 = be.mul(C1, [sk2 % L] * n)
    out = []

    def add(name, i, pinned, c1=None, d=None, a=None, b=None, zz=None):
        out.append((name, c1 or C1[i], d or D[i], a or A[i], b or B[i], z[i] if zz is None else zz, pinned))
    for i in range(n):
        add("valid %d" % i, i, 1)
    add("bit of z", 0, 0, zz=z[0] ^ (1 << 77))
    add("bit 0 of z", 1, 0, zz=z[1] ^ 1)
    add("bit of A.x", 0, 0, a=(A[0][0] ^ (1 << 100), A[0][1]))
    add("bit of A.y", 1, 0, a=(A[1][0], A[1][1] ^ 8))
    add("bit of B.x", 2, 0, b=(B[2][0] ^ 1, B[2][1]))
    add("bit of B.y", 5, 0, b=(B[5][0], B[5][1] ^ (1 << 200)))
    add("C1 of another item", 0, 0, c1=C1[1])
    add("D = sk2 C1", 2, 0, d=D2[2])
    add("A and B swapped", 6, 0, a=B[6], b=A[6])
    add("A = -A", 7, 0, a=neg(A[7]))
    add("z + l", 0, 0, zz=z[0] + L)
    add("z = 2^256 - 1", 0, 0, zz=M256)
    for i in range(n):
        if A[i][0] + Q <= M256:
            add("A.x + r", i, 0, a=(A[i][0] + Q, A[i][1]))
            break
    for i in range(n):
        if B[i][1] + Q <= M256:
            add("B.y + r", i, 0, b=(B[i][0], B[i][1] + Q))
            break
    add("off-curve A", 0, 0, a=W["off"])
    add("off-curve B", 0, 0, b=W["off_y"])
    add("A = (0, 0)", 0, 0, a=(0, 0))
    add("off-curve C1", 0, 2, c1=W["off"])
    add("off-curve D", 0, 2, d=W["off_y"])
    add("C1 = (0, 0)", 0, 2, c1=(0, 0))
    add("off-curve D and a bad z", 0, 2, d=(0, 0), zz=M256)
    add("C1.x + r stays valid", 8, 1 if C1[8][0] + Q <= M256 else None,
        c1=(C1[8][0] + Q, C1[8][1]) if C1[8][0] + Q <= M256 else None)
    # D' = D + T2 with a proof MADE for it: c' = H(tag, C1, D', A, B), z' = w' + c' sk'.  The first equation holds, the second reads
    # z' C1 = B + c' D + c' T2 and holds exactly when c' is even -- the subgroup caveat of the header, pinned here to the model
    Dt = be.add(D, [T2] * n)
    ct = challenge(be, tag, C1, Dt, A, B)
    zt = [(w[i] % L + (ct[i] % L) * (sk % L)) % L for i in range(n)]
    even = next(i for i in range(n) if ct[i] % 2 == 0)
    odd = next(i for i in range(n) if ct[i] % 2 == 1)
    add("D + T2, c even", even, 1, d=Dt[even], zz=zt[even])
    add("D + T2, c odd", odd, 0, d=Dt[odd], zz=zt[odd])
    return out


def dleq_wrong_statements(tag):
    """(name, what changes) for the mutations that are not per item: a wrong tag, the wrong PK table"""
    return [("wrong tag", (tag + 1) % Q), ("tag + r is the same tag", tag + Q if tag + Q <= M256 else tag)]
