#!/usr/bin/env python3
"""Developer tool: bjj_mul_bases_dev against what callers compose without it, n = 2^20, one process, device events.  The forms
of one context alternate: after three warm-up calls of each, --rounds rounds time --inner back-to-back calls of every form
between one pair of events, in an order that rotates from round to round; a row gives the median over the rounds and the
smallest and largest round.

  python tools/bases_probe.py [--out profiles/bases_vs_var_base.txt] [--log2n 20] [--rounds 7] [--inner 10]

  (a) {P} at W = 16 and W = 23 against bjj_mul_var_base_dev of the same points and scalars, and against bjj_mul_fixed_base_dev on a
      context of the same W (B8: one window fewer at W = 23, the same number at W = 16)
  (b) {NULL} against bjj_mul_fixed_base_dev: the same table, so the difference is the new kernel's overhead over K1
  (c) {NULL, P} against bjj_mul_fixed_base_dev + bjj_mul_var_base_dev + bjj_point_add_dev (the ElGamal second component)
Every pair is checked for equal bytes before its times are reported.  P = k * B8 + T8 (order 8l)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(torch, fns, stream, rounds, inner):
    """{name: (median, min, max)} in ms per call of the callables of `fns` (a dict), alternating as the module text says"""
    names = list(fns)
    for name in names:
        for _ in range(3):
            fns[name]()
    torch.cuda.synchronize()
    ms = {name: [] for name in names}
    for r in range(rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(inner):
                fns[name]()
            b.record(stream)
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / inner)
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import babyjubjub_rs_amd as bjj
    from babyjubjub_rs_amd import workload as w
    n = 1 << args.log2n
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    s = st.cuda_stream
    sc = [torch.from_numpy(w.random_u256(w.SEED_SCALARS ^ (0xBA5E + j), n).reshape(-1)).to(dev) for j in range(2)]
    outs = {k: torch.empty(n * 64, dtype=torch.uint8, device=dev) for k in ("P", "var", "k1", "null", "two", "c1", "c2", "comp")}
    lines = ["# bjj_mul_bases_dev against the calls it replaces, n = 2^%d items, device events; the forms alternate, %d rounds of %d"
             % (args.log2n, args.rounds, args.inner), "# calls each after 3 warm-up calls; ms per call: median of the rounds [smallest .. largest round]",
             "# (ratio: the other side's median over bjj_mul_bases_dev's)",
             "%-4s %-3s %-22s %-24s   %-48s %-27s %6s" % ("case", "W", "bjj_mul_bases_dev", "ms", "against", "ms", "ratio")]

    def cell(t):
        return "%7.3f [%6.3f .. %6.3f]" % t

    def row(case, W, what, t_new, against, t_old):
        lines.append("%-4s %-3d %-22s %-24s   %-48s %-27s %6.2f" % (case, W, what, cell(t_new), against, cell(t_old), t_old[0] / t_new[0]))

    with open(os.path.join(ROOT, "tests", "golden", "gpu_expected.json")) as f:
        tors = json.load(f)["torsion_points"][1]
    t8 = np.frombuffer(b"".join(int(v, 16).to_bytes(32, "little") for v in tors), np.uint8)
    for W in (16, 23):
        ctx = bjj.Context(0, W)
        P = ctx.point_add(ctx.mul_fixed_base(w.scalars_254(1, offset=77)), t8.reshape(1, 64)).copy()
        base = ctx.base(P, W)
        pts = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(P, (n, 64))).reshape(-1)).to(dev)
        s0, s1 = sc[0].data_ptr(), sc[1].data_ptr()

        def compose():
            ctx.mul_fixed_base_dev(s0, n, outs["c1"].data_ptr(), s)
            ctx.mul_var_base_dev(pts.data_ptr(), s1, n, outs["c2"].data_ptr(), s)
            ctx.point_add_dev(outs["c1"].data_ptr(), outs["c2"].data_ptr(), n, outs["comp"].data_ptr(), s)
        fns = {"P": lambda: ctx.mul_bases_dev([base], [s0], n, outs["P"].data_ptr(), s),
               "var": lambda: ctx.mul_var_base_dev(pts.data_ptr(), s0, n, outs["var"].data_ptr(), s),
               "k1": lambda: ctx.mul_fixed_base_dev(s0, n, outs["k1"].data_ptr(), s),
               "null": lambda: ctx.mul_bases_dev([None], [s0], n, outs["null"].data_ptr(), s),
               "two": lambda: ctx.mul_bases_dev([None, base], [s0, s1], n, outs["two"].data_ptr(), s),
               "comp": compose}
        with torch.cuda.stream(st):
            t = measure(torch, fns, st, args.rounds, args.inner)
        torch.cuda.synchronize()
        for x, y in (("P", "var"), ("null", "k1"), ("two", "comp")):
            assert bool(torch.equal(outs[x], outs[y])), "results disagree: %s, %s" % (x, y)
        what = "{P}, %d windows" % base.info()[1]
        row("a", W, what, t["P"], "bjj_mul_var_base_dev, same points and scalars", t["var"])
        row("a", W, what, t["P"], "bjj_mul_fixed_base_dev (B8, %d windows)" % ctx.info().n_windows, t["k1"])
        row("b", W, "{NULL}", t["null"], "bjj_mul_fixed_base_dev (the same table)", t["k1"])
        row("c", W, "{NULL, P}", t["two"], "mul_fixed_base + mul_var_base + point_add (_dev)", t["comp"])
        ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
