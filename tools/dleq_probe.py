#!/usr/bin/env python3
"""Developer tool: the three _dev calls of include/bjj_hip_dleq.h against the calls they replace, n = 2^20, one process, the same
inputs, device events.  The forms of one context alternate: after three warm-up calls of each, --rounds rounds time --inner
back-to-back calls of every form between one pair of events, in an order that rotates from round to round; a row gives the median
over the rounds and the smallest and largest round.

  python tools/dleq_probe.py [--out profiles/dleq.txt] [--log2n 20] [--rounds 7] [--inner 5]

  pair    bjj_mul_pair_dev(P, a, Q, b, A)  against  2 x bjj_mul_var_base_dev + 2 x bjj_point_add_dev, and against the two
          bjj_mul_var_base_dev alone with ONE bjj_point_add_dev (add = NULL on the fused side): the row the operation count speaks of
  verify  bjj_dleq_verify_dev  against  what a caller composes today: 2 x bjj_poseidon5_dev (the 160-byte records assembled by
          device copies, counted), z G and c PK by bjj_mul_bases_dev (two calls of one base each: a caller has no -c on the device to
          make it one), z C1 and c D by 2 x bjj_mul_var_base_dev, 2 x bjj_point_add_dev, and the comparison of the two pairs of arrays
          (on the device); at (context W, key W) = (23, 23) and (16, 16)
  prove   bjj_dleq_prove_dev  against  its parts: bjj_mul_common_dev, bjj_mul_bases_dev, bjj_mul_var_base_dev, 2 x bjj_poseidon5_dev
          (w is given below l, so the parts need no reduction of their own; z's integer arithmetic is NOT in the parts' time)
Every pair is checked for equal results before its times are reported.  A row whose ranges overlap is a tie."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L = 2736030358979909402780800718157159386076813972158567259200215660948447373041


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
    ap.add_argument("--inner", type=int, default=5)
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
    sk = 0x1F2E3D4C5B6A79881726354453627180_0F1E2D3C4B5A6978 % L
    tag = 0x0123456789ABCDEF00112233445566778899AABBCCDDEEFF
    tag_rec = torch.from_numpy(np.frombuffer(tag.to_bytes(32, "little"), np.uint8).copy()).to(dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).to(dev)   # noqa: E731
    buf = lambda width: torch.empty(n * width, dtype=torch.uint8, device=dev)   # noqa: E731
    d_a, d_b, d_k = (up(w.random_u256(w.SEED_SCALARS ^ x, n)) for x in (0xD1E0, 0xD1E1, 0xD1E2))
    wl = w.random_u256(w.SEED_SCALARS ^ 0xD1E3, n).reshape(n, 32).copy()
    wl[:, 31] &= 0x03                                                          # below 2^250 < l
    d_w = up(wl)
    lines = ["# the _dev calls of bjj_hip_dleq.h against the calls they replace, n = 2^%d items, device events; the forms alternate, %d rounds"
             % (args.log2n, args.rounds), "# of %d calls each after 3 warm-up calls; ms per call: median of the rounds [smallest .. largest round]" % args.inner,
             "# (ratio: the new call's median over the replaced calls'; tie: the two ranges overlap)",
             "%-8s %-6s %-27s   %-62s %-27s %6s  %s" % ("row", "W", "new call ms", "against", "ms", "ratio", "verdict")]

    def cell(t):
        return "%7.3f [%6.3f .. %6.3f]" % t

    def row(case, W, t_new, against, t_old):
        overlap = t_new[2] >= t_old[1] and t_old[2] >= t_new[1]
        verdict = "tie" if overlap else "faster" if t_new[0] < t_old[0] else "SLOWER"
        lines.append("%-8s %-6s %-27s   %-62s %-27s %6.2f  %s" % (case, W, cell(t_new), against, cell(t_old), t_new[0] / t_old[0], verdict))

    for W in (23, 16):
        ctx = bjj.Context(0, W)
        pk = ctx.base(ctx.mul_common(sk, ctx.mul_fixed_base([1]))[0].copy(), W)
        d_p, d_q, d_add = buf(64), buf(64), buf(64)
        torch.cuda.synchronize()   # the inputs were copied on torch's stream; everything below runs on `st`
        ctx.mul_fixed_base_dev(d_k.data_ptr(), n, d_p.data_ptr(), s)              # C1 = k B8: points of the subgroup
        ctx.mul_fixed_base_dev(d_a.data_ptr(), n, d_q.data_ptr(), s)
        ctx.mul_fixed_base_dev(d_b.data_ptr(), n, d_add.data_ptr(), s)
        ctx.sync()
        o = {k: buf(64) for k in ("f", "f0", "t1", "t2", "s1", "c", "c0", "D", "A", "B", "eD", "eA", "eB", "l1", "cpk", "l2", "cd", "r1", "r2")}
        z, ez_h, ez_c, d_h, d_c = buf(32), buf(32), buf(32), buf(32), buf(32)
        rec = torch.empty(n, 160, dtype=torch.uint8, device=dev)
        ok = {k: torch.empty(n, dtype=torch.uint8, device=dev) for k in ("pair", "pair0", "prove", "common", "verify")}
        P = lambda k: o[k].data_ptr()   # noqa: E731

        if W == 23:   # bjj_mul_pair uses no fixed-base table: measured once
            def pair_parts():
                ctx.mul_var_base_dev(d_p.data_ptr(), d_a.data_ptr(), n, P("t1"), s)
                ctx.mul_var_base_dev(d_q.data_ptr(), d_b.data_ptr(), n, P("t2"), s)
                ctx.point_add_dev(d_add.data_ptr(), P("t1"), n, P("s1"), s)
                ctx.point_add_dev(P("s1"), P("t2"), n, P("c"), s)

            def pair_parts0():
                ctx.mul_var_base_dev(d_p.data_ptr(), d_a.data_ptr(), n, P("t1"), s)
                ctx.mul_var_base_dev(d_q.data_ptr(), d_b.data_ptr(), n, P("t2"), s)
                ctx.point_add_dev(P("t1"), P("t2"), n, P("c0"), s)
            fns = {"pair": lambda: ctx.mul_pair_dev(d_p.data_ptr(), d_a.data_ptr(), d_q.data_ptr(), d_b.data_ptr(), d_add.data_ptr(), n, P("f"),
                                                    ok["pair"].data_ptr(), s),
                   "parts": pair_parts,
                   "pair0": lambda: ctx.mul_pair_dev(d_p.data_ptr(), d_a.data_ptr(), d_q.data_ptr(), d_b.data_ptr(), None, n, P("f0"),
                                                     ok["pair0"].data_ptr(), s),
                   "parts0": pair_parts0}
            with torch.cuda.stream(st):
                t = measure(torch, fns, st, args.rounds, args.inner)
            torch.cuda.synchronize()
            assert bool(torch.equal(o["f"], o["c"])) and bool(torch.equal(o["f0"], o["c0"])) and bool((ok["pair"] == 1).all())
            row("pair", "-", t["pair"], "2 x mul_var_base + 2 x point_add (_dev)", t["parts"])
            row("pair A=O", "-", t["pair0"], "2 x mul_var_base + point_add (_dev)", t["parts0"])

        # ---- prove against its parts ----
        def hash_parts(c1, D, A, B):
            with torch.cuda.stream(st):
                rec[:, :32] = tag_rec
                rec[:, 32:96] = c1.view(n, 64)
                rec[:, 96:] = D.view(n, 64)
            ctx.poseidon5_dev(rec.data_ptr(), n, d_h.data_ptr(), s)
            with torch.cuda.stream(st):
                rec[:, :32] = d_h.view(n, 32)
                rec[:, 32:96] = A.view(n, 64)
                rec[:, 96:] = B.view(n, 64)
            ctx.poseidon5_dev(rec.data_ptr(), n, d_c.data_ptr(), s)

        def prove_parts():
            ctx.mul_common_dev(sk, d_p.data_ptr(), None, n, P("eD"), ok["common"].data_ptr(), stream=s)
            ctx.mul_bases_dev([None], [d_w.data_ptr()], n, P("eA"), s)
            ctx.mul_var_base_dev(d_p.data_ptr(), d_w.data_ptr(), n, P("eB"), s)
            hash_parts(d_p, o["eD"], o["eA"], o["eB"])
        fns = {"prove": lambda: ctx.dleq_prove_dev(sk, tag, d_p.data_ptr(), d_w.data_ptr(), n, P("D"), P("A"), P("B"), z.data_ptr(),
                                                   ok["prove"].data_ptr(), stream=s),
               "parts": prove_parts}
        with torch.cuda.stream(st):
            t = measure(torch, fns, st, args.rounds, args.inner)
        torch.cuda.synchronize()
        assert all(bool(torch.equal(o[x], o[y])) for x, y in (("D", "eD"), ("A", "eA"), ("B", "eB"))) and bool((ok["prove"] == 1).all())
        sample = np.arange(0, n, max(1, n // 4096))
        cs, ws, zs = (x.view(n, 32)[sample].cpu().numpy() for x in (d_c, d_w, z))
        val = lambda r_: int.from_bytes(bytes(r_), "little")   # noqa: E731
        assert all(val(zz) == (val(ww) + val(cc) % L * sk) % L for zz, ww, cc in zip(zs, ws, cs)), "z differs from w + c sk"
        row("prove", str(W), t["prove"], "mul_common + mul_bases + mul_var_base + 2 x poseidon5 (_dev)", t["parts"])

        # ---- verify against the composition ----
        def verify_parts():
            hash_parts(d_p, o["D"], o["A"], o["B"])
            ctx.mul_bases_dev([None], [z.data_ptr()], n, P("l1"), s)
            ctx.mul_bases_dev([pk], [d_c.data_ptr()], n, P("cpk"), s)
            ctx.point_add_dev(P("A"), P("cpk"), n, P("r1"), s)
            ctx.mul_var_base_dev(d_p.data_ptr(), z.data_ptr(), n, P("l2"), s)
            ctx.mul_var_base_dev(P("D"), d_c.data_ptr(), n, P("cd"), s)
            ctx.point_add_dev(P("B"), P("cd"), n, P("r2"), s)
            with torch.cuda.stream(st):
                ok["common"].copy_(((o["l1"].view(n, 64) == o["r1"].view(n, 64)).all(dim=1) & (o["l2"].view(n, 64) == o["r2"].view(n, 64)).all(dim=1)))
        fns = {"verify": lambda: ctx.dleq_verify_dev(pk, tag, d_p.data_ptr(), P("D"), P("A"), P("B"), z.data_ptr(), n, ok["verify"].data_ptr(), stream=s),
               "parts": verify_parts}
        with torch.cuda.stream(st):
            t = measure(torch, fns, st, args.rounds, args.inner)
        torch.cuda.synchronize()
        assert bool((ok["verify"] == 1).all()) and bool((ok["common"] == 1).all())
        row("verify", str(W), t["verify"], "2 x poseidon5 + 2 x mul_bases + 2 x mul_var_base + 2 x point_add", t["parts"])
        del o
        ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
