#!/usr/bin/env python3
"""Developer tool: bjj_dlog_dev at n = 2^20 over B8 tables of several widths, with device events in one process, beside
bjj_mul_var_base_dev on the same count -- the other half of an ElGamal decryption.  Per table: the time bjj_dlog_table_create takes
(build and self-check, a host clock around the synchronous call), bjj_dlog_table_check alone, the table's bytes; then the search with
every item found (m uniform in [0, 2^range_bits)) and with no item in range (the worst case: every giant step of the range).  The
forms of a block alternate as in bases_probe.py: three warm-up calls each, then --rounds rounds of --inner back-to-back calls between
one pair of events; a row is the median of the rounds with the smallest and the largest.  A walk of more than 2^12 giant steps
takes seconds per call: such a row has one warm-up call and 3 rounds of 1 call, and says so.  Every result is checked before its
times are reported.

  python tools/dlog_probe.py [--out profiles/dlog.txt] [--log2n 20] [--tables 16,20,22,24] [--rounds 5] [--inner 3] [--wide 24:40]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import statistics  # noqa: E402

SEED_M = 0xD106D106


def measure(torch, fns, stream, rounds, inner, warm=3):
    """{name: (median, min, max)} in ms per call of the callables of `fns`: the scheme of bases_probe.measure with the number of
    warm-up calls as a parameter (a walk of 2^15 steps takes seconds per call)"""
    names = list(fns)
    for name in names:
        for _ in range(warm):
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
    ap.add_argument("--tables", default="16,20,22,24")
    ap.add_argument("--range-bits", type=int, default=32)
    ap.add_argument("--wide", default="24:40", help="baby_bits:range_bits of one more, longer row ('' = none)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
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
    ctx = bjj.Context(0, 0)
    lines = ["# bjj_dlog_dev over B8, n = 2^%d items, device events; ms per call: median of %d rounds of %d calls after 3 warm-up calls"
             % (args.log2n, args.rounds, args.inner),
             "# (rows marked '3 x 1': 1 warm-up call, 3 rounds of 1 call) [smallest .. largest round]; M/s from the median.",
             "# found: m uniform in [0, 2^range_bits); none: no item in range (every giant step of the range is walked).",
             "#  create = bjj_dlog_table_create (build + self-check), check = bjj_dlog_table_check: host",
             "# clock around the synchronous call, one call each.  context: B8 table of %d-bit windows" % ctx.info().window_bits,
             "%-58s %-29s %8s" % ("form", "ms", "M/s")]

    def row(name, t):
        lines.append("%-58s %8.3f [%7.3f .. %7.3f] %8.2f" % (name, t[0], t[1], t[2], n / t[0] / 1e3))

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)

    def scalars(vals):
        a = np.zeros((n, 4), dtype=np.uint64)
        a[:, 0] = vals
        return a.view(np.uint8).reshape(n, 32)

    raw = w.splitmix64(SEED_M, n)
    inputs = {}

    def workload(range_bits):
        if range_bits not in inputs:
            m = raw & np.uint64((1 << range_bits) - 1)
            far = m + np.uint64(1 << 50)                      # a small logarithm, but beyond every range the header admits
            inputs[range_bits] = (m, up(ctx.mul_fixed_base(scalars(m))), up(ctx.mul_fixed_base(scalars(far))))
        return inputs[range_bits]

    # the yardstick: the variable-base multiplication of the same count, same process, same card
    m32, d_found32, _ = workload(args.range_bits)
    d_sc = up(w.random_u256(w.SEED_SCALARS, n))
    d_out = torch.empty(n * 64, dtype=torch.uint8, device=dev)
    with torch.cuda.stream(st):
        t = measure(torch, {"var": lambda: ctx.mul_var_base_dev(d_found32.data_ptr(), d_sc.data_ptr(), n, d_out.data_ptr(), s)}, st,
                    args.rounds, args.inner)
    row("bjj_mul_var_base_dev (the other half of a decryption)", t["var"])

    def job(b, rb):                                           # a walk of more than 2^12 steps takes seconds per call: fewer of them
        long_walk = rb - b - 1 > 12
        return (b, rb, 3 if long_walk else args.rounds, 1 if long_walk else args.inner, 1 if long_walk else 3)
    jobs = [job(int(b), args.range_bits) for b in args.tables.split(",") if b]
    if args.wide:
        jobs.append(job(*(int(v) for v in args.wide.split(":"))))
    made = {}
    for b, rb, rounds, inner, warm in jobs:
        if b not in made:
            t0 = time.perf_counter()
            try:
                made[b] = ctx.dlog_table(None, b)
            except bjj.BjjError as e:
                lines.append("# baby_bits = %d: not measured, the table could not be created (%s)" % (b, e))
                continue
            t1 = time.perf_counter()
            assert made[b].check() == 0
            t2 = time.perf_counter()
            lines.append("# baby_bits = %d: table %.1f MiB (%d entries); create %.1f ms, check %.1f ms"
                         % (b, made[b].info()[2] / 2.0 ** 20, made[b].info()[1], (t1 - t0) * 1e3, (t2 - t1) * 1e3))
        table = made[b]
        m, d_found, d_none = workload(rb)
        d_m = {k: torch.full((n,), 0xEE, dtype=torch.int64, device=dev) for k in ("found", "none")}
        d_ok = {k: torch.full((n,), 0xEE, dtype=torch.uint8, device=dev) for k in ("found", "none")}
        fns = {"found": lambda: ctx.dlog_dev(table, d_found.data_ptr(), n, rb, d_m["found"].data_ptr(), d_ok["found"].data_ptr(), s),
               "none": lambda: ctx.dlog_dev(table, d_none.data_ptr(), n, rb, d_m["none"].data_ptr(), d_ok["none"].data_ptr(), s)}
        with torch.cuda.stream(st):
            t = measure(torch, fns, st, rounds, inner, warm)
        torch.cuda.synchronize()
        assert bool((d_ok["found"] == 1).all()) and (d_m["found"].cpu().numpy().view(np.uint64) == m).all(), "wrong logarithms (found)"
        assert bool((d_ok["none"] == 0).all()) and bool((d_m["none"] == -1).all()), "wrong results (none)"
        steps = 1 if rb <= b + 1 else 1 << (rb - b - 1)
        note = "" if (rounds, inner) == (args.rounds, args.inner) else ", %d x %d" % (rounds, inner)
        row("bjj_dlog_dev baby_bits = %d range_bits = %d (%d steps%s) found" % (b, rb, steps, note), t["found"])
        row("bjj_dlog_dev baby_bits = %d range_bits = %d (%d steps%s) none" % (b, rb, steps, note), t["none"])
        del d_m, d_ok
    for table in made.values():
        table.close()
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
