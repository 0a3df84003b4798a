#!/usr/bin/env python3
"""Developer tool: bjj_elgamal_encrypt_dev against the calls it replaces, n = 2^20, one process, device events.  The forms of one
context alternate: after three warm-up calls of each, --rounds rounds time --inner back-to-back calls of every form between one
pair of events, in an order that rotates from round to round; a row gives the median over the rounds and the smallest and
largest round.

  python tools/elgamal_probe.py [--out profiles/elgamal_encrypt.txt] [--log2n 20] [--rounds 7] [--inner 10]

At (context W, key W) = (23, 23) and (16, 16), g = NULL (the context's B8 table), PK = k * B8:
  enc     bjj_elgamal_encrypt_dev(m, r)  against  bjj_mul_bases_dev({NULL}, {r}) + bjj_mul_bases_dev({NULL, pk}, {m as 32 bytes, r})
  rerand  bjj_elgamal_encrypt_dev(NULL, r, add = C)  against  bjj_mul_bases_dev({NULL}, {r}) + bjj_mul_bases_dev({NULL, pk}, {0, r})
          + two bjj_point_add_dev (what a caller composes today; the zero m array keeps the composition's second call as it is)
Every pair is checked for equal bytes before its times are reported.  A fused row whose range overlaps the other side's is a tie."""
import argparse
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
    r = torch.from_numpy(w.random_u256(w.SEED_SCALARS ^ 0xE16A, n).reshape(-1)).to(dev)
    m64 = np.random.default_rng(0xE16A).integers(0, 1 << 64, size=n, dtype=np.uint64)
    m32 = np.zeros((n, 32), np.uint8)
    m32[:, :8] = m64.view(np.uint8).reshape(n, 8)
    d_m, d_m32 = torch.from_numpy(m64.view(np.uint8)).to(dev), torch.from_numpy(m32.reshape(-1)).to(dev)
    d_zero32 = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    o = {k: torch.empty(n * 64, dtype=torch.uint8, device=dev) for k in ("f1", "f2", "p1", "p2", "a1", "a2", "rf1", "rf2", "rp1", "rp2", "rc1", "rc2")}
    d_ok = torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()   # the inputs were copied on torch's stream; everything below runs on `st`
    lines = ["# bjj_elgamal_encrypt_dev against the calls it replaces, n = 2^%d items, device events; the forms alternate, %d rounds of %d"
             % (args.log2n, args.rounds, args.inner), "# calls each after 3 warm-up calls; ms per call: median of the rounds [smallest .. largest round]",
             "# (ratio: the fused call's median over the composition's; tie: the two ranges overlap)",
             "%-7s %-7s %-27s   %-58s %-27s %6s  %s" % ("row", "W g/pk", "bjj_elgamal_encrypt_dev ms", "against", "ms", "ratio", "verdict")]

    def cell(t):
        return "%7.3f [%6.3f .. %6.3f]" % t

    def row(case, W, t_new, against, t_old):
        overlap = t_new[2] >= t_old[1] and t_old[2] >= t_new[1]
        verdict = "tie" if overlap else "faster" if t_new[0] < t_old[0] else "SLOWER"
        lines.append("%-7s %-7s %-27s   %-58s %-27s %6.2f  %s" % (case, "%d/%d" % (W, W), cell(t_new), against, cell(t_old), t_new[0] / t_old[0], verdict))

    for W in (23, 16):
        ctx = bjj.Context(0, W)
        pk = ctx.base(ctx.mul_fixed_base(w.scalars_254(1, offset=77)).copy(), W)
        P = lambda k: o[k].data_ptr()
        # a ciphertext to re-randomise: any curve points serve
        ctx.mul_bases_dev([None], [d_m32.data_ptr()], n, P("a1"), s)
        ctx.mul_bases_dev([pk], [r.data_ptr()], n, P("a2"), s)

        def compose():
            ctx.mul_bases_dev([None], [r.data_ptr()], n, P("p1"), s)
            ctx.mul_bases_dev([None, pk], [d_m32.data_ptr(), r.data_ptr()], n, P("p2"), s)

        def compose_rerand():
            ctx.mul_bases_dev([None], [r.data_ptr()], n, P("rp1"), s)
            ctx.mul_bases_dev([None, pk], [d_zero32.data_ptr(), r.data_ptr()], n, P("rp2"), s)
            ctx.point_add_dev(P("a1"), P("rp1"), n, P("rc1"), s)
            ctx.point_add_dev(P("a2"), P("rp2"), n, P("rc2"), s)
        fns = {"enc": lambda: ctx.elgamal_encrypt_dev(pk, d_m.data_ptr(), r.data_ptr(), n, P("f1"), P("f2"), stream=s),
               "comp": compose,
               "rerand": lambda: ctx.elgamal_encrypt_dev(pk, None, r.data_ptr(), n, P("rf1"), P("rf2"), d_add_c1=P("a1"), d_add_c2=P("a2"),
                                                         d_ok=d_ok.data_ptr(), stream=s),
               "comp_rerand": compose_rerand}
        with torch.cuda.stream(st):
            t = measure(torch, fns, st, args.rounds, args.inner)
        torch.cuda.synchronize()
        for x, y in (("f1", "p1"), ("f2", "p2"), ("rf1", "rc1"), ("rf2", "rc2")):
            assert bool(torch.equal(o[x], o[y])), "results disagree: %s, %s" % (x, y)
        assert bool((d_ok == 1).all())
        row("enc", W, t["enc"], "mul_bases({NULL},{r}) + mul_bases({NULL,pk},{m,r}) (_dev)", t["comp"])
        row("rerand", W, t["rerand"], "the same two (m = 0) + 2 x point_add (_dev)", t["comp_rerand"])
        ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
