"""Inputs shared by the signer-set tests on the GPU (tests/test_gpu_signer_set.py); holds no tests.  Built per key with
tests/signer_cases.py (key_point, bulk, directed) and the C oracle, then interleaved by a seeded permutation.

The key list begins with an ordinary key, a key of order 8l (torsion component), B8 itself, an ordinary key whose record holds
x + r (unreduced), the identity, and a duplicate of the first key; further ordinary keys pad it up to k.  Every key that is asked
for gets signed items (1 in 8 with a bit flipped, signer_cases.bulk); the first two keys also get the DIRECTED items, which end the
array.  1 item in 16 of the others has its index moved to a different signer: a valid signature presented under the wrong key."""
import numpy as np

import signer_cases as sc
from conftest import ints, pack, unpack

Q = sc.Q


def key_list(oracle, golden, k):
    """-> (points, scalars, torsion flags, records): points[j] is key j reduced mod r, records the (k, 64) uint8 array handed to
    bjj_signer_set_create (record 3 holds x + r)"""
    tors = [ints(t) for t in golden["gpu_expected"]["torsion_points"]]
    scalars = [sc.KEY_SCALAR, sc.KEY_SCALAR + 12345, 1, sc.KEY_SCALAR + 999, 0, sc.KEY_SCALAR][:k]
    scalars += [(sc.KEY_SCALAR + 5000 + 7919 * j) % sc.L for j in range(len(scalars), k)]
    pts = unpack(oracle.mul_fixed_base(sc.rec(scalars)), 2)
    torsion = [False] * k
    if k > 1:
        pts[1] = sc.key_point(oracle, scalars[1], tors[1])
        torsion[1] = True
    if k > 2:
        assert pts[2] == sc.B8
    if k > 4:
        assert pts[4] == (0, 1)
    recs = list(pts)
    if k > 3:
        recs[3] = (pts[3][0] + Q, pts[3][1])
    records = pack(recs).reshape(k, 64)
    records.setflags(write=False)
    return pts, scalars, torsion, records


def dataset(oracle, keys, n, schnorr, seed, signers=None):
    """n items under the keys `signers` (default: all) of key_list's result -> dict(idx (n,) uint32, R, S, msg, want): the bulk
    items interleaved, the directed items of keys 0 and 1 last; want = the oracle's verdicts with the key records gathered by
    index, checked to hold at least n / 2 ones and n / 16 zeros (otherwise the INPUTS are wrong) and never rewritten"""
    pts, scalars, torsion, records = keys
    k = len(pts)
    signers = list(range(k)) if signers is None else sorted(signers)
    with_directed = [j for j in (0, 1) if j in signers]
    nb = n - len(with_directed) * len(sc.DIRECTED)
    assert nb >= len(signers)
    parts, idx = [], []
    for pos, j in enumerate(signers):
        cnt = nb // len(signers) + (1 if pos < nb % len(signers) else 0)
        parts.append(sc.bulk(oracle, pts[j], scalars[j], cnt, seed + 31 * j, schnorr, torsion[j]))
        idx += [j] * cnt
    rng = np.random.default_rng(seed ^ 0x5E75)
    perm = rng.permutation(nb)
    R, S, M = (np.concatenate([p[c] for p in parts])[perm] for c in range(3))
    idx = np.asarray(idx, np.uint32)[perm]
    if len(signers) > 1:
        moved = np.nonzero(rng.integers(0, 16, nb) == 0)[0]
        where = np.searchsorted(np.asarray(signers), idx[moved])                          # signers is ascending
        idx[moved] = np.asarray(signers, np.uint32)[(where + 1 + rng.integers(0, len(signers) - 1, moved.size)) % len(signers)]   # a different signer
    for j in with_directed:
        R2, S2, M2 = sc.directed(oracle, pts[j], scalars[j], seed + 0xD1 + j, schnorr, torsion[j])
        R, S, M = np.concatenate([R, R2]), np.concatenate([S, S2]), np.concatenate([M, M2])
        idx = np.concatenate([idx, np.full(len(sc.DIRECTED), j, np.uint32)])
    want = (oracle.verify_schnorr if schnorr else oracle.verify)(np.ascontiguousarray(records[idx]), R, S, M)
    ones, zeros = int((want == 1).sum()), int((want == 0).sum())
    print("[k = %d %s] oracle: %d ones, %d zeros of %d" % (k, "schnorr" if schnorr else "eddsa", ones, zeros, n))
    assert ones >= n // 2 and zeros >= n // 16, (k, schnorr, ones, zeros)
    for a in (idx, R, S, M, want):
        a.setflags(write=False)
    return dict(idx=idx, R=R, S=S, msg=M, want=want)


PATTERNS = ("random", "all_equal", "round_robin", "sorted_blocks", "last_signer")


def arrange(d, k, pattern):
    """positions of d's items, len(d['idx']) of them, in the order of an index pattern.  Items are only rearranged or repeated,
    each keeping its own index, so the expected verdicts are the oracle's, gathered by the same positions."""
    idx = d["idx"]
    n = idx.size
    if pattern == "random":                                # as built: a seeded permutation, the directed items last
        return np.arange(n)
    if pattern in ("all_equal", "last_signer"):            # one signer for the whole call
        own = np.nonzero(idx == (0 if pattern == "all_equal" else k - 1))[0]
        return np.resize(own, n)
    if pattern == "sorted_blocks":
        return np.argsort(idx, kind="stable")
    order = np.argsort(idx, kind="stable")                 # round robin: consecutive items under consecutive signers
    rank = np.empty(n, np.int64)
    start = np.searchsorted(idx[order], idx[order], side="left")
    rank[order] = np.arange(n) - start
    return np.lexsort((idx, rank))
