"""Cases shared by tests/test_dlog_host.py and tests/test_gpu_dlog.py: the test chooses m and computes P = m * G with an oracle it is
handed (the pure-Python one on the CPU, the C one on the GPU box), so the expectation never comes from the code under test.

A case list is a list of (record, truth): record = (x, y) as it goes into the call (possibly x + r), truth = the only m with
m * G = P when that m is known to be small (an int), NOT_IN_RANGE when the only logarithm is known to be astronomically large (or there
is none), OFF_CURVE for a record that fails the curve equation.  expected() turns truths into (m, ok) for one range_bits."""
import numpy as np

Q = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ORDER = 21888242871839275222246405745257275088614511777268538073601725287587578984328
SUBORDER = ORDER >> 3
NOT_IN_RANGE, OFF_CURVE = "not in range", "off curve"
UINT64_MAX = (1 << 64) - 1


def m_values(b, ranges, seed, n_random):
    """directed m for a table of b baby bits searched with every range_bits of `ranges`, then n_random seeded ones"""
    stride = 2 << b
    ms = [0, 1, (1 << b) - 1, 1 << b, (1 << b) + 1]
    for r in ranges:
        steps = max(1, (1 << r) // stride)
        for k in sorted({1, max(1, steps // 2), steps}):           # the first, a middle and the last giant step
            ms += [k * stride - 1, k * stride, k * stride + 1]
        ms += [(1 << r) - 1, 1 << r, (1 << r) + 5]
    ms += [(1 << b) - 3, 10]                                        # in the baby table, beyond a range_bits of 3
    rng = np.random.default_rng(seed)
    top = 1 << max(ranges)
    ms += [int(v) for v in rng.integers(0, top + top // 8, n_random)]   # a ninth of them beyond the widest range
    return ms


def build(mul, add, G, b, ranges, torsion, seed, n_random=200):
    """mul(P, [k...]) -> [k * P ...], add(P, Q) -> P + Q (affine int pairs).  torsion: a point of order 8."""
    ms = m_values(b, ranges, seed, n_random)
    pts = mul(G, ms)
    cases = [(p, m) for p, m in zip(pts, ms)]
    negs = [1, 2, (1 << b) - 1, 1 << b, 5]
    for j, p in zip(negs, mul(G, negs)):                            # -j * G: the y of j * G, and not j
        cases.append((((Q - p[0]) % Q, p[1]), NOT_IN_RANGE))
    for p in mul(G, [ORDER - 1, SUBORDER - 1]):
        cases.append((p, NOT_IN_RANGE))
    for p in mul(G, [3, (1 << b) + 2]):                             # m * G + T
        cases.append((add(p, torsion), NOT_IN_RANGE))
    cases.append(((0, 1), 0))                                       # the identity
    cases.append(((pts[5][0], (pts[5][1] + 1) % Q), OFF_CURVE))
    cases.append(((0, 0), OFF_CURVE))
    cases.append(((pts[6][0] + Q, pts[6][1]), ms[6]))               # x + r: reduced
    return cases


def interleave(cases):
    """found and not-found items alternate, so that the lanes of one wave finish at different steps"""
    small = [c for c in cases if isinstance(c[1], int)]
    other = [c for c in cases if not isinstance(c[1], int)]
    small.sort(key=lambda c: c[1])
    out = []
    lo, hi = 0, len(small) - 1
    while lo <= hi or other:                                        # smallest, largest, one that is never found, ...
        if lo <= hi:
            out.append(small[lo]); lo += 1
        if other:
            out.append(other.pop())
        if lo <= hi:
            out.append(small[hi]); hi -= 1
    return out


def expected(cases, range_bits):
    m, ok = [], []
    for _, truth in cases:
        if truth == OFF_CURVE:
            m.append(UINT64_MAX); ok.append(2)
        elif truth == NOT_IN_RANGE or truth >= (1 << range_bits):
            m.append(UINT64_MAX); ok.append(0)
        else:
            m.append(truth); ok.append(1)
    return m, ok
