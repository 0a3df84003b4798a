#!/usr/bin/env python3
"""
Regenerates tests/golden/msm_expected.json: known answers of bjj_msm (Q = sum k_i * P_i) for the `-m gpu` tests, computed by the
Python oracle as the reference's own fold -- acc = acc.add(&P_i.mul_scalar(k_i).projective()) from (0, 1, 1), then acc.affine()
(src/lib.rs:149-164, 88-131, 70-85).  Inputs come from the SplitMix64 generator of oracle/bjj_oracle.py with a seed of their own,
so the file is reproducible byte for byte (tests/test_msm_host.py checks that).

Run from the repo root:  python tests/golden/make_msm_expected.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import bjj_oracle as o  # noqa: E402

SEED_MSM = 0x424A4A5F4D534D21
ORDER8 = o.ORDER


def hx(v):
    return "0x%x" % v


def fold(points, scalars):
    acc = (0, 1, 1)
    for p, k in zip(points, scalars):
        m = o.mul_scalar(p, k)
        acc = o.proj_add(acc, (m[0], m[1], 1))
    return o.proj_affine(acc)


def cases():
    rng = o.SplitMix64(SEED_MSM)
    pt = lambda: o.mul_scalar(o.B8, rng.u256() % o.SUBORDER)   # noqa: E731  a random point of the prime-order subgroup
    torsion = [o.mul_scalar(o.T8, j) for j in range(8)]
    edge = [0, 1, ORDER8 - 1, ORDER8, ORDER8 + 1, (1 << 256) - 1, o.SUBORDER, (1 << 254) - 1]
    out = []
    for n in (1, 2, 3, 5, 8, 13):                               # random points and scalars
        P = [pt() for _ in range(n)]
        out.append(("random", P, [rng.u256() for _ in range(n)]))
    for n in (2, 4, 9):                                         # torsion-shifted points
        P = [o.proj_affine(o.proj_add((*pt(), 1), (*torsion[rng.next() % 8], 1))) for _ in range(n)]
        out.append(("torsion_shifted", P, [rng.u256() for _ in range(n)]))
    out.append(("torsion_only", torsion, [rng.u256() for _ in range(8)]))
    out.append(("identity", [(0, 1)] * 3, [rng.u256() for _ in range(3)]))
    p, q = pt(), pt()
    out.append(("duplicates", [p, p, q, p, q], [rng.u256() for _ in range(5)]))
    k = rng.u256()
    out.append(("cancelling_pair", [p, (o.Q - p[0], p[1])], [k, k]))                      # P, -P: the identity
    out.append(("cancelling_mixed", [p, q, (o.Q - p[0], p[1])], [k, rng.u256(), k]))
    P = [pt() for _ in range(len(edge))]
    out.append(("edge_scalars", P, edge))
    out.append(("zero_scalars", P[:4], [0, 0, 0, 0]))
    out.append(("equal_scalars", [pt() for _ in range(7)], [k] * 7))
    out.append(("one_bucket", [pt() for _ in range(6)], [(1 << 255) // 3] * 6))             # 0x5555..: one digit value per window
    out.append(("order_multiples", P[:3], [ORDER8, 2 * ORDER8, 2 * ORDER8 + 5]))
    for n in (17, 33):                                          # a few longer ones
        P = [pt() for _ in range(n)]
        out.append(("random", P, [rng.u256() for _ in range(n)]))
    return out


def main():
    doc = {"comment": "bjj_msm known answers: the reference fold of mul_scalar + PointProjective::add from the identity, then affine "
                      "(tests/golden/make_msm_expected.py)",
           "cases": []}
    for name, P, K in cases():
        assert all(0 <= k < 1 << 256 for k in K), name     # the 32-byte scalar records of the C ABI
        q = fold(P, K)
        doc["cases"].append({"name": name, "points": [[hx(x), hx(y)] for x, y in P], "scalars": [hx(k) for k in K],
                             "result": [hx(q[0]), hx(q[1])]})
    with open(os.path.join(HERE, "msm_expected.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
