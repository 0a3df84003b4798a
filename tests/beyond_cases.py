"""Inputs shared by tests/test_gpu_beyond_one_grid.py; holds no tests.  Everything here is plain numpy over arrays the GPU test has
produced with the library's oracle-tested entry points: where the trips of a grid-strided kernel begin, which items go to the C
oracle, directed scalars placed into later trips, a corruption plan for signatures (the kinds of signer_cases.DIRECTED) that
reaches every trip, and the 16 kinds of points of tests/test_gpu_common_scalar.py laid out over an array of any length."""
import numpy as np

import signer_cases as sc
from bases_cases import directed, scalar_array
from conftest import pack

Q, L = sc.Q, sc.L
ORDER8 = 8 * L


# ---- trips of a grid of R resident lanes ----------------------------------------------------------------------------------------
def trips(n, R):
    """[lo, hi) of every trip a grid of R lanes makes over n items"""
    return [(lo, min(lo + R, n)) for lo in range(0, n, R)]


def oracle_subset(n, R, seed):
    """the items that go to the C oracle: all of the last trip, the first 64 of every trip, every 257th, and 2 048 seeded ones
    outside the last trip (every 257th of 2 R items is only about R / 128) -> sorted unique indices"""
    t = trips(n, R)
    last_lo = t[-1][0]
    parts = [np.arange(last_lo, n), np.arange(0, n, 257), np.random.default_rng(seed).integers(0, last_lo, 2048)]
    parts += [np.arange(lo, min(lo + 64, hi)) for lo, hi in t]
    sub = np.unique(np.concatenate(parts))
    assert int((sub < last_lo).sum()) >= 2000
    return sub


def placed_scalars(n, R, widths, seed):
    """bases_cases.scalar_array (the directed scalars lead the first trip), with the same directed scalars again from item R on
    and as the last items of the array: the second trip and the ragged tail meet the mod-8l edges and the all-negative pattern"""
    a = scalar_array(n, widths, seed)
    d = pack(directed(widths)).reshape(-1, 32)[:40]
    assert R + len(d) <= n - len(d)
    a[R:R + len(d)] = d
    a[n - len(d):] = d
    return a


# ---- signatures: which items are corrupted, and how ---------------------------------------------------------------------------------
KINDS = tuple(k for k in sc.DIRECTED if k not in ("valid", "valid2"))   # "s+l", "msg=Q" and "R.x+r" stay valid signatures
OFF_CURVE_R, MSG_ABOVE_Q = KINDS.index("flip R.y"), KINDS.index("msg=Q+1")


def corruption_plan(n, R, last_kind):
    """row -> kind (an index into KINDS): 1 item in 8 all over the array, the kinds in turn, so every trip but a short last one
    holds hundreds of each; every kind once more in the first 57 items of the last trip; the last item, which is the only one of
    the ragged wave when n = 2 R + 65, carries `last_kind`"""
    plan = {i: (i // 8) % len(KINDS) for i in range(5, n, 8)}
    lo = trips(n, R)[-1][0]
    for k in range(len(KINDS)):
        if lo + 5 * k + 1 < n:
            plan[lo + 5 * k + 1] = k
    plan[n - 1] = last_kind
    return plan


def messages_to_sign(msgs, plan):
    """the "msg=Q" items are signed over 0 and presented as Q: the reference wraps Q to 0"""
    m = msgs.copy()
    rows = [i for i, k in plan.items() if KINDS[k] == "msg=Q"]
    m[rows] = 0
    return m


def _int(row):
    return int.from_bytes(row.tobytes(), "little")


def _put(row, v):
    row[:] = np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


def corrupt(Rp, S, M, plan):
    """applies the plan in place to R (n, 64), S (n, 32), msg (n, 32): signer_cases.directed, item by item"""
    for i, k in plan.items():
        kind = KINDS[k]
        if kind == "s+l":
            _put(S[i], _int(S[i]) % L + L)
        elif kind == "s=2^256-1":
            S[i] = 0xFF
        elif kind == "msg=Q":
            _put(M[i], Q)
        elif kind == "msg=Q+1":
            _put(M[i], Q + 1)
        elif kind == "flip s":
            S[i, 77 // 8] ^= np.uint8(1 << (77 % 8))
        elif kind == "flip msg":
            M[i, 0] ^= np.uint8(1 << 5)
        elif kind == "flip R.x":
            Rp[i, 100 // 8] ^= np.uint8(1 << (100 % 8))
        elif kind == "flip R.y":
            Rp[i, 32] ^= np.uint8(1 << 3)
        elif kind == "R=identity":
            Rp[i] = 0
            Rp[i, 32] = 1
        elif kind == "R=(0,0)":
            Rp[i] = 0
        elif kind == "R=order 2":
            Rp[i, :32] = 0
            _put(Rp[i, 32:], Q - 1)
        elif kind == "R.x+r":
            _put(Rp[i, :32], _int(Rp[i, :32]) + Q)          # < 2^256: the record is reduced mod r, the signature stays valid
        else:
            raise AssertionError(kind)


def kinds_in(plan, lo, hi):
    return {k for i, k in plan.items() if lo <= i < hi}


# ---- the 16 kinds of points of tests/test_gpu_common_scalar.py ------------------------------------------------------------------------
def mixed_points(sub, shifted, nontrivial, j):
    """(n, 64) records: item i is of kind j[i] % 16 -- B8, the identity, three of low order, five subgroup points sub[i], three
    torsion-shifted ones shifted[i], one with x + r in the record, one off the curve (x ^ 1), (0, 0) -> (records, on the curve)"""
    n = len(sub)
    i = np.arange(n)
    k = np.asarray(j) % 16
    low = pack(list(nontrivial)).reshape(7, 64)
    out = np.array(sub, np.uint8).reshape(n, 64)
    out[k == 0] = pack([sc.B8]).reshape(1, 64)
    out[k == 1] = pack([(0, 1)]).reshape(1, 64)
    out[k == 2] = pack([(0, Q - 1)]).reshape(1, 64)
    out[k == 3] = low[i[k == 3] % 7]
    out[k == 4] = low[(3 * i[k == 4] + 1) % 7]
    sh = (k >= 10) & (k <= 12)
    out[sh] = np.asarray(shifted, np.uint8).reshape(n, 64)[sh]
    for r in np.nonzero(k == 13)[0]:
        _put(out[r, :32], _int(out[r, :32]) + Q)             # x >= r, < 2^256
    out[k == 14, 0] ^= np.uint8(1)                          # off the curve
    out[k == 15] = 0
    return out, k < 14


def on_curve(rec):
    x, y = _int(rec[:32]) % Q, _int(rec[32:]) % Q
    return (168700 * x * x + y * y - 1 - 168696 * x * x * y * y) % Q == 0
