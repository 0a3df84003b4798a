#!/usr/bin/env python3
"""Developer tool: bjj_point_sum_dev at n = 2^20 points beside the two routes a caller had before it, with device events in one
process on the same inputs: bjj_msm_batch_dev with every scalar 1, and -- for the single sum -- a halving tree of bjj_point_add_dev
(log2 n launches over ping-pong buffers).  Rows: one segment; 2^10 equal segments; 2^18 segments of 4; 2^20 singletons; one
segment of 2^19 followed by 2^19 singletons.  The forms of a row alternate as in dlog_probe.py: three warm-up calls each, then
--rounds rounds of --inner back-to-back calls between one pair of events; a row is the median of the rounds with the smallest and
the largest.  Every result is checked before its times are reported: the point sum against the batched MSM byte for byte (all terms
added, and once more with random signs against the scalars 1 and 8l - 1), the tree against the point sum.

  python tools/point_sum_probe.py [--out profiles/point_sum.txt] [--log2n 20] [--rounds 7] [--inner 3] [--rows m1,m2^10,...]"""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dlog_probe import measure  # noqa: E402

L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
K1_MULS_PER_S = 1.8e9 * 16 * 7     # K1: 1.8 G fixed-base multiplications/s, 16 mixed additions of 7 field multiplications each
EST_MULS_PER_POINT = 12            # one complete addition (7-8 multiplications) plus the curve check


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--rows", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import babyjubjub_rs_amd as bjj
    from babyjubjub_rs_amd import workload as w
    lg = args.log2n
    n = 1 << lg
    tile = int(re.search(r"^#define PSUM_TILE (\d+)\b", open(os.path.join(ROOT, "babyjubjub-rs_amd", "csrc", "point_sum.hpp")).read(),
                         flags=re.M).group(1))
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    s = st.cuda_stream
    ctx = bjj.Context(0, 0)
    est_us = n * EST_MULS_PER_POINT / K1_MULS_PER_S * 1e6
    lines = ["# bjj_point_sum_dev, n = 2^%d points (PSUM_TILE = %d), device events; ms per call: median of %d rounds of %d calls after 3"
             % (lg, tile, args.rounds, args.inner),
             "# warm-up calls [smallest .. largest round]; M points/s from the median.  msm_batch: bjj_msm_batch_dev, every scalar 1,",
             "# window_bits 0; tree: %d launches of bjj_point_add_dev over halves.  Compute estimate: %d field multiplications per point at"
             % (lg, EST_MULS_PER_POINT),
             "# K1's rate (%.3g/s) = %.0f us per call.  context: B8 table of %d-bit windows" % (K1_MULS_PER_S, est_us, ctx.info().window_bits),
             "%-64s %-29s %8s" % ("row / form", "ms", "M/s")]

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)

    pts = ctx.mul_fixed_base(w.scalars_254(n, 0x95))   # points of the prime-order subgroup
    d_pts = up(pts)
    ones = np.zeros((n, 32), np.uint8)
    ones[:, 0] = 1
    d_ones = up(ones)
    neg = (w.splitmix64(0x5157, n) & np.uint64(1)).astype(np.uint8)
    d_neg = up(neg)
    signed = ones.copy()
    signed[neg != 0] = np.frombuffer((8 * L - 1).to_bytes(32, "little"), np.uint8)
    d_signed = up(signed)
    half = n // 2
    rows = {
        "m = 1": [0, n],
        "m = 2^10 equal segments": list(range(0, n + 1, n >> 10)),
        "m = 2^%d segments of 4" % (lg - 2): list(range(0, n + 1, 4)),
        "m = 2^%d singletons" % lg: list(range(n + 1)),
        "one segment of 2^%d, then 2^%d singletons" % (lg - 1, lg - 1): [0] + list(range(half, n + 1)),
    }
    want = [r for r in args.rows.split(",") if r]
    for name, off in rows.items():
        if want and not any(name.startswith(r) for r in want):
            continue
        m = len(off) - 1
        d_off = up(np.asarray(off, np.uint64))
        out = {f: torch.full((m * 64,), 0xEE, dtype=torch.uint8, device=dev) for f in ("point_sum", "point_sum signed", "msm_batch", "check")}
        sw = {f: torch.full((m,), 0xEE, dtype=torch.int64, device=dev) for f in out}
        fns = {
            "point_sum": lambda: ctx.point_sum_dev(d_pts.data_ptr(), None, n, d_off.data_ptr(), m, out["point_sum"].data_ptr(),
                                                   sw["point_sum"].data_ptr(), s),
            "point_sum signed": lambda: ctx.point_sum_dev(d_pts.data_ptr(), d_neg.data_ptr(), n, d_off.data_ptr(), m,
                                                          out["point_sum signed"].data_ptr(), sw["point_sum signed"].data_ptr(), s),
            "msm_batch": lambda: ctx.msm_batch_dev(d_pts.data_ptr(), d_ones.data_ptr(), n, d_off.data_ptr(), m, out["msm_batch"].data_ptr(),
                                                   sw["msm_batch"].data_ptr(), 0, s),
        }
        if m == 1:
            ping = [torch.empty(n * 64, dtype=torch.uint8, device=dev), torch.empty(half * 64, dtype=torch.uint8, device=dev)]

            def tree():
                src, cnt, t = d_pts, n, 1
                while cnt > 1:
                    cnt //= 2
                    ctx.point_add_dev(src.data_ptr(), src.data_ptr() + cnt * 64, cnt, ping[t].data_ptr(), s)
                    src, t = ping[t], t ^ 1
                return src
            fns["tree"] = tree
        with torch.cuda.stream(st):
            t = measure(torch, fns, st, args.rounds, args.inner)
            ctx.msm_batch_dev(d_pts.data_ptr(), d_signed.data_ptr(), n, d_off.data_ptr(), m, out["check"].data_ptr(), sw["check"].data_ptr(), 0, s)
            last = tree() if m == 1 else None
        torch.cuda.synchronize()
        assert all(bool((v == -1).all()) for v in sw.values()), "status words"
        assert bool((out["point_sum"] == out["msm_batch"]).all()), "bjj_point_sum_dev differs from bjj_msm_batch_dev (all added)"
        assert bool((out["point_sum signed"] == out["check"]).all()), "bjj_point_sum_dev differs from bjj_msm_batch_dev (signed)"
        if m == 1:
            assert bool((last[:64] == out["point_sum"]).all()), "the point_add tree differs from bjj_point_sum_dev"
        for f in fns:
            lines.append("%-64s %8.3f [%7.3f .. %7.3f] %8.2f" % (name + ": " + f, t[f][0], t[f][1], t[f][2], n / t[f][0] / 1e3))
        lines.append("%-64s %8.1fx (median / median; largest point_sum round against smallest msm_batch round: %.1fx)"
                     % (name + ": msm_batch / point_sum", t["msm_batch"][0] / t["point_sum"][0], t["msm_batch"][1] / t["point_sum"][2]))
        del out, sw, d_off
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
