#!/usr/bin/env python3
"""Developer tool: bjj_msm_dev timed with device events (median of --reps after one warm-up call), against what callers compose
today -- bjj_mul_var_base_dev, then a tree of bjj_point_add_dev -- on the same inputs.

  python tools/msm_probe.py sizes  [--lo 10 --hi 24 --step 2]   size sweep: library window, composition, ratio
  python tools/msm_probe.py windows [--lo 10 --hi 24 --step 2]  every forced c = 4..20 per size (sets kMsmAutoWindow, bjj_hip.hip)
  python tools/msm_probe.py skew   [--log2n 20]                 random vs all-scalars-equal vs every digit in one bucket vs half zero
  python tools/msm_probe.py one    [--log2n 20]                 one library-window call after a warm-up (run it under
                                                                rocprofv3 --kernel-trace --stats for the per-kernel times)
Inputs: P_i = k_i * B8 (device fixed-base), scalars uniform 256-bit (SplitMix64, babyjubjub_rs_amd/workload.py)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import babyjubjub_rs_amd as bjj  # noqa: E402
from babyjubjub_rs_amd import workload as w  # noqa: E402

DEV = torch.device("cuda", 0)


def inputs(ctx, n, stream):
    sc = torch.from_numpy(w.scalars_254(n).reshape(-1)).to(DEV)
    pts = torch.empty(n * 64, dtype=torch.uint8, device=DEV)
    ctx.mul_fixed_base_dev(sc.data_ptr(), n, pts.data_ptr(), stream)
    scal = torch.from_numpy(w.random_u256(w.SEED_SCALARS ^ 0x4D53, n).reshape(-1)).to(DEV)
    torch.cuda.synchronize()
    return pts, scal


def timed(fn, stream, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


class Msm:
    def __init__(self, ctx, st):
        self.ctx, self.st = ctx, st
        self.out = torch.zeros(64, dtype=torch.uint8, device=DEV)
        self.status = torch.zeros(2, dtype=torch.int64, device=DEV)

    def __call__(self, pts, sc, n, c=0):
        self.ctx.msm_dev(pts.data_ptr(), sc.data_ptr(), n, self.out.data_ptr(), self.status.data_ptr(), c, self.st.cuda_stream)

    def result(self):
        assert int(self.status[0]) == -1
        return self.out.cpu().numpy().copy()


class Composition:
    """bjj_mul_var_base_dev, then log2(n) levels of bjj_point_add_dev (an odd tail item waits for the next level)"""

    def __init__(self, ctx, st, n):
        self.ctx, self.st, self.n = ctx, st, n
        self.a = torch.empty(n * 64, dtype=torch.uint8, device=DEV)
        self.b = torch.empty(((n + 1) // 2) * 64, dtype=torch.uint8, device=DEV)

    def __call__(self, pts, sc):
        s = self.st.cuda_stream
        self.ctx.mul_var_base_dev(pts.data_ptr(), sc.data_ptr(), self.n, self.a.data_ptr(), s)
        cur, nxt, m = self.a, self.b, self.n
        while m > 1:
            h = m // 2
            self.ctx.point_add_dev(cur.data_ptr(), cur.data_ptr() + h * 64, h, nxt.data_ptr(), s)
            if m % 2:   # the odd item is carried along to the next level
                nxt[h * 64:(h + 1) * 64].copy_(cur[(m - 1) * 64:m * 64])
            cur, nxt, m = nxt, cur, h + (m % 2)
        self.last = cur

    def result(self):
        return self.last[:64].cpu().numpy().copy()


def sizes(ctx, st, args):
    print("# bjj_msm_dev vs bjj_mul_var_base_dev + bjj_point_add_dev tree (device events, median of %d)" % args.reps)
    print("%10s %4s %10s %14s %8s %12s" % ("n", "c", "msm ms", "compose ms", "ratio", "M points/s"))
    for lg in range(args.lo, args.hi + 1, args.step):
        n = 1 << lg
        pts, sc = inputs(ctx, n, st.cuda_stream)
        m, comp = Msm(ctx, st), Composition(ctx, st, n)
        with torch.cuda.stream(st):
            t_m = timed(lambda: m(pts, sc, n), st, args.reps)
            t_c = timed(lambda: comp(pts, sc), st, args.reps)
        assert (m.result() == comp.result()).all(), "msm and composition disagree at n = %d" % n
        print("%10d %4s %10.3f %14.3f %8.2f %12.1f" % (n, "auto", t_m, t_c, t_c / t_m, n / t_m / 1e3), flush=True)
        del pts, sc, comp
        torch.cuda.empty_cache()


def windows(ctx, st, args):
    print("# bjj_msm_dev, every forced window c (device events, median of %d); * = fastest" % args.reps)
    for lg in range(args.lo, args.hi + 1, args.step):
        n = 1 << lg
        pts, sc = inputs(ctx, n, st.cuda_stream)
        m = Msm(ctx, st)
        row, ref = {}, None
        with torch.cuda.stream(st):
            for c in range(4, 21):
                row[c] = timed(lambda: m(pts, sc, n, c), st, args.reps)
                r = m.result()
                assert ref is None or (r == ref).all(), "c = %d disagrees at n = %d" % (c, n)
                ref = r
            auto = timed(lambda: m(pts, sc, n, 0), st, args.reps)
        best = min(row, key=row.get)
        print("n = 2^%-2d  auto %.3f ms   " % (lg, auto) + "  ".join("c%d %.3f%s" % (c, t, "*" if c == best else "") for c, t in row.items()),
              flush=True)
        del pts, sc
        torch.cuda.empty_cache()


def skew(ctx, st, args):
    n = 1 << args.log2n
    pts, sc = inputs(ctx, n, st.cuda_stream)
    m = Msm(ctx, st)
    k = torch.from_numpy(np.frombuffer((0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDE).to_bytes(32, "little"), np.uint8)
                         .copy()).to(DEV)
    u = torch.from_numpy(np.frombuffer(sum(1 << (16 * j) for j in range(16)).to_bytes(32, "little"), np.uint8).copy()).to(DEV)
    equal = k.repeat(n)
    bucket = u.repeat(n)
    half = sc.clone().view(n, 32)
    half[::2] = 0
    half = half.reshape(-1)
    print("# skewed inputs, n = 2^%d (device events, median of %d)" % (args.log2n, args.reps))
    with torch.cuda.stream(st):
        base = {}
        for c in (0, 16):
            base[c] = timed(lambda: m(pts, sc, n, c), st, args.reps)
            print("%-36s c=%-4s %9.3f ms" % ("random scalars", c or "auto", base[c]), flush=True)
        for name, s, c in (("all scalars equal", equal, 0), ("all scalars equal", equal, 16), ("every digit in one bucket (c = 16)", bucket, 16),
                           ("half of the scalars zero", half, 0)):
            t = timed(lambda: m(pts, s, n, c), st, args.reps)
            print("%-36s c=%-4s %9.3f ms   x%.2f of random" % (name, c or "auto", t, t / base[c]), flush=True)


def one(ctx, st, args):
    n = 1 << args.log2n
    pts, sc = inputs(ctx, n, st.cuda_stream)
    m = Msm(ctx, st)
    with torch.cuda.stream(st):
        m(pts, sc, n)
        torch.cuda.synchronize()
        m(pts, sc, n)
        torch.cuda.synchronize()
    print("one call done, n = 2^%d" % args.log2n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["sizes", "windows", "skew", "one"])
    ap.add_argument("--lo", type=int, default=10)
    ap.add_argument("--hi", type=int, default=24)
    ap.add_argument("--step", type=int, default=2)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    ctx = bjj.Context(0, 16)   # the fixed-base table only generates the points here
    st = torch.cuda.Stream(device=DEV)
    {"sizes": sizes, "windows": windows, "skew": skew, "one": one}[args.what](ctx, st, args)
    ctx.close()


if __name__ == "__main__":
    main()
