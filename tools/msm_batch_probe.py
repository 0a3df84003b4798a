#!/usr/bin/env python3
"""Developer tool: bjj_msm_batch_dev timed with device events (median of --reps after one warm-up call).

  python tools/msm_batch_probe.py sweep  [--out profiles/msm_batch_window_sweep.txt]
        forced c = 4..16 and the library's choice at mean segment lengths 2^4, 2^6, 2^8, 2^10, 2^12, 2^16 with n = 2^20
        (sets kMsmBatchAutoWindow, bjj_hip.hip)
  python tools/msm_batch_probe.py versus [--out profiles/msm_batch_vs_loop.txt]
        m x length = 16 x 2^16, 1024 x 2^10, 2^14 x 2^6: the batched call against (a) a loop of bjj_msm_dev over the segments and
        (b) bjj_mul_var_base_dev over all items + a bjj_point_add_dev tree over item-major data; then m = 1 at 2^20 against bjj_msm_dev
  python tools/msm_batch_probe.py one    [--log2m 10 --log2len 10]
        one library-window call after a warm-up (run it under rocprofv3 --kernel-trace --stats for the per-kernel times)

Every step (one shape) of sweep / versus runs in a child process of its own under --step-timeout seconds; the first step that
fails or runs out of time ends the run -- nothing is tried again.  A forced width whose scratch would exceed --max-gib is
reported as "-" without a call.  Inputs: P_i = k_i * B8 (device fixed-base), scalars uniform 256-bit, equal-length segments."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWEEP_LENGTHS = (4, 6, 8, 10, 12, 16)
VERSUS_SHAPES = ((4, 16), (10, 10), (14, 6))   # log2 m, log2 length
LOG2N = 20


def scratch_bytes(n, m, c):
    """what bjjk::msm_batch_layout asks for, to within the alignment padding"""
    W, B = (255 + c - 1) // c, 1 << (c - 1)
    keys = m * W * B
    return n * (164 + 8 * W) + keys * 172 + 2 * m * W * (B // 8) * 160 + n * W * 160 // 2


def keys_fit(m, c):
    return m * ((255 + c - 1) // c) * (1 << (c - 1)) < 1 << 31


# ---- child side: one shape ------------------------------------------------------------------------------------------------------
def _gpu():
    import numpy as np
    import torch
    import babyjubjub_rs_amd as bjj
    from babyjubjub_rs_amd import workload as w
    return np, torch, bjj, w


def timed(torch, fn, stream, reps):
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


class Shape:
    def __init__(self, lgm, lglen):
        np, torch, bjj, w = _gpu()
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.ctx = bjj.Context(0, 16)   # the fixed-base table only generates the points here
        self.st = torch.cuda.Stream(device=self.dev)
        self.m, self.length = 1 << lgm, 1 << lglen
        self.n = n = self.m * self.length
        sc = torch.from_numpy(w.scalars_254(n).reshape(-1)).to(self.dev)
        self.pts = torch.empty(n * 64, dtype=torch.uint8, device=self.dev)
        self.ctx.mul_fixed_base_dev(sc.data_ptr(), n, self.pts.data_ptr(), self.st.cuda_stream)
        self.sc = torch.from_numpy(w.random_u256(w.SEED_SCALARS ^ 0x4D53, n).reshape(-1)).to(self.dev)
        self.off = torch.arange(0, n + 1, self.length, dtype=torch.int64, device=self.dev)
        self.out = torch.zeros(self.m * 64, dtype=torch.uint8, device=self.dev)
        self.status = torch.zeros(self.m + 1, dtype=torch.int64, device=self.dev)
        torch.cuda.synchronize()

    def batch(self, c=0):
        self.ctx.msm_batch_dev(self.pts.data_ptr(), self.sc.data_ptr(), self.n, self.off.data_ptr(), self.m, self.out.data_ptr(),
                               self.status.data_ptr(), c, self.st.cuda_stream)

    def batch_result(self):
        assert bool((self.status[:self.m] == -1).all())
        return self.out.cpu().numpy().reshape(self.m, 64).copy()

    def loop(self, out, status, segments=None):
        """(a): one bjj_msm_dev per segment"""
        p, s, ln = self.pts.data_ptr(), self.sc.data_ptr(), self.length
        for k in range(self.m if segments is None else segments):
            self.ctx.msm_dev(p + k * ln * 64, s + k * ln * 32, ln, out.data_ptr() + k * 64, status.data_ptr() + 16 * k, 0, self.st.cuda_stream)


def step_sweep(args):
    sh = Shape(LOG2N - args.log2len, args.log2len)
    torch = sh.torch
    row, ref = {}, None
    with torch.cuda.stream(sh.st):
        for c in list(range(4, 17)) + [0]:
            if c and (not keys_fit(sh.m, c) or scratch_bytes(sh.n, sh.m, c) > args.max_gib << 30):
                row[c] = None
                continue
            row[c] = timed(torch, lambda: sh.batch(c), sh.st, args.reps)
            r = sh.batch_result()
            assert ref is None or (r == ref).all(), "c = %d disagrees" % c
            ref = r
    print(json.dumps({"log2len": args.log2len, "ms": row}))


def step_versus(args):
    sh = Shape(args.log2m, args.log2len)
    torch, m, ln, n = sh.torch, sh.m, sh.length, sh.n
    res = {"log2m": args.log2m, "log2len": args.log2len}
    with torch.cuda.stream(sh.st):
        res["batch_ms"] = timed(torch, sh.batch, sh.st, args.reps)
        want = sh.batch_result()
        # (a)
        out, status = torch.zeros(m * 64, dtype=torch.uint8, device=sh.dev), torch.zeros(2 * m, dtype=torch.int64, device=sh.dev)
        sh.loop(out, status, min(m, 8))   # warm-up: the first segments only (the scratch set has its size after one call)
        torch.cuda.synchronize()
        res["loop_ms"] = timed(torch, lambda: sh.loop(out, status), sh.st, 1 if m > 1024 else args.reps) if m > 1 else None
        if m > 1:
            assert (out.cpu().numpy().reshape(m, 64) == want).all(), "loop and batch disagree"
        # (b): item-major data (item t of segment s at t * m + s): every level of the tree adds two contiguous halves
        if m > 1:
            tp = sh.pts.view(m, ln, 64).transpose(0, 1).contiguous().view(-1)
            ts = sh.sc.view(m, ln, 32).transpose(0, 1).contiguous().view(-1)
            a, b = torch.empty(n * 64, dtype=torch.uint8, device=sh.dev), torch.empty(n * 32, dtype=torch.uint8, device=sh.dev)
            s = sh.st.cuda_stream

            def compose():
                sh.ctx.mul_var_base_dev(tp.data_ptr(), ts.data_ptr(), n, a.data_ptr(), s)
                cur, nxt, k = a, b, n
                while k > m:
                    k //= 2
                    sh.ctx.point_add_dev(cur.data_ptr(), cur.data_ptr() + k * 64, k, nxt.data_ptr(), s)
                    cur, nxt = nxt, cur
                compose.last = cur
            res["compose_ms"] = timed(torch, compose, sh.st, args.reps)
            assert (compose.last[:m * 64].cpu().numpy().reshape(m, 64) == want).all(), "composition and batch disagree"
        else:   # m = 1: the batched entry against bjj_msm_dev itself, interleaved
            o1, s1 = torch.zeros(64, dtype=torch.uint8, device=sh.dev), torch.zeros(2, dtype=torch.int64, device=sh.dev)
            single = lambda: sh.ctx.msm_dev(sh.pts.data_ptr(), sh.sc.data_ptr(), n, o1.data_ptr(), s1.data_ptr(), 0, sh.st.cuda_stream)  # noqa: E731
            pairs = [(timed(torch, single, sh.st, args.reps), timed(torch, sh.batch, sh.st, args.reps)) for _ in range(3)]
            res["msm_dev_ms"], res["batch_ms"] = statistics.median(p[0] for p in pairs), statistics.median(p[1] for p in pairs)
            assert (o1.cpu().numpy() == want[0]).all()
    print(json.dumps(res))


def one(args):
    sh = Shape(args.log2m, args.log2len)
    with sh.torch.cuda.stream(sh.st):
        sh.batch()
        sh.torch.cuda.synchronize()
        sh.batch()
        sh.torch.cuda.synchronize()
    sh.batch_result()
    print("one call done, m = 2^%d segments of 2^%d points" % (args.log2m, args.log2len))


# ---- parent side: one child per step, the first failure ends the run --------------------------------------------------------------
def run_step(args, extra):
    cmd = [sys.executable, os.path.abspath(__file__), "_step"] + extra + ["--reps", str(args.reps), "--max-gib", str(args.max_gib)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)   # TimeoutExpired ends the run
    if r.returncode != 0:
        raise SystemExit("step %s failed with exit status %d: stopping" % (" ".join(extra), r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


def emit(lines, path):
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if path:
        with open(path, "w") as f:
            f.write(text)


def sweep(args):
    lines = ["# bjj_msm_batch_dev, n = 2^%d in equal segments, forced window c and the library's choice (device events, median of %d after a"
             % (LOG2N, args.reps), "# warm-up); ms per call; * = fastest forced c; - = key range >= 2^31 or scratch above %d GiB (not run)" % args.max_gib,
             "%-14s %8s  " % ("m x length", "auto") + " ".join("%8s" % ("c%d" % c) for c in range(4, 17))]
    for lg in SWEEP_LENGTHS:
        row = {int(k): v for k, v in run_step(args, ["sweep", "--log2len", str(lg)])["ms"].items()}
        ran = {c: t for c, t in row.items() if c and t is not None}
        best = min(ran, key=ran.get)
        cells = " ".join("%8s" % ("-" if row[c] is None else "%.3f%s" % (row[c], "*" if c == best else "")) for c in range(4, 17))
        lines.append("%-14s %8.3f  %s" % ("2^%d x 2^%d" % (LOG2N - lg, lg), row[0], cells))
        emit(lines, args.out)


def versus(args):
    lines = ["# bjj_msm_batch_dev (library window) against (a) a loop of bjj_msm_dev over the segments and (b) bjj_mul_var_base_dev over all",
             "# items + a bjj_point_add_dev tree over item-major data; device events, median of %d after a warm-up (loops of more than" % args.reps,
             "# 1024 calls: one timed pass); ms per whole batch",
             "%-14s %12s %12s %12s %10s %10s" % ("m x length", "batch", "(a) loop", "(b) compose", "(a)/batch", "(b)/batch")]
    for lgm, lglen in VERSUS_SHAPES:
        r = run_step(args, ["versus", "--log2m", str(lgm), "--log2len", str(lglen)])
        lines.append("%-14s %12.3f %12.3f %12.3f %10.2f %10.2f" % ("2^%d x 2^%d" % (lgm, lglen), r["batch_ms"], r["loop_ms"], r["compose_ms"],
                                                                 r["loop_ms"] / r["batch_ms"], r["compose_ms"] / r["batch_ms"]))
        emit(lines, args.out)
    r = run_step(args, ["versus", "--log2m", "0", "--log2len", str(LOG2N)])
    lines.append("m = 1, 2^%d points: bjj_msm_batch_dev %.3f ms, bjj_msm_dev %.3f ms (%+.2f %%; medians of 3 interleaved rounds)"
                 % (LOG2N, r["batch_ms"], r["msm_dev_ms"], 100.0 * (r["batch_ms"] / r["msm_dev_ms"] - 1.0)))
    emit(lines, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["sweep", "versus", "one", "_step"])
    ap.add_argument("step", nargs="?", choices=["sweep", "versus"])
    ap.add_argument("--log2m", type=int, default=10)
    ap.add_argument("--log2len", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-gib", type=int, default=24)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.what == "_step":
        {"sweep": step_sweep, "versus": step_versus}[args.step](args)
    else:
        {"sweep": sweep, "versus": versus, "one": one}[args.what](args)


if __name__ == "__main__":
    main()
