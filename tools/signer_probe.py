#!/usr/bin/env python3
"""Developer tool: bjj_eddsa_verify_signer_dev / bjj_schnorr_verify_signer_dev against the generic verifiers on the same inputs with
the key replicated, and against bjj_poseidon5_dev on the same count (the floor: every verification holds one permutation).
n = 2^20, one process, device events.  The forms alternate: after three warm-up calls of each, --rounds rounds time --inner
back-to-back calls of every form between one pair of events, in an order that rotates from round to round; a row gives the median
over the rounds and the smallest and largest round.  Every pair is checked for equal bytes before its times are reported.

  python tools/signer_probe.py [--out profiles/signer_verify.txt] [--log2n 20] [--rounds 7] [--inner 10]

Workload: the cfg-4 one under ONE key -- R = rho*B8, S = rho + 8*hm*k mod l (Schnorr: rho + h*k), 1 item in 64 with one seeded bit
flipped in S, msg or R.y.  The context has the default 23-bit B8 table; the signer's table has W = 16 and W = 23."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bases_probe import measure  # noqa: E402


def one_key_workload(ctx, n, schnorr):
    """(A (1, 64), R, S, msg) built with the library's own fixed-base and Poseidon kernels, as bench.py builds cfg 4"""
    import numpy as np
    from babyjubjub_rs_amd import workload as w
    k = w.to_ints(w.random_u256(w.SEED_KEYS, 1))[0] % w.L_ORDER
    rho = [v % w.L_ORDER for v in w.to_ints(w.random_u256(w.SEED_NONCES, n))]
    msg = w.random_u256(w.SEED_MSGS, n, top_bits_cleared=3)
    A = ctx.mul_fixed_base(w.from_ints([k]))
    R = ctx.mul_fixed_base(w.from_ints(rho))
    Arep = np.ascontiguousarray(np.broadcast_to(A, (n, 64)))
    h = w.to_ints(ctx.poseidon5(np.concatenate([Arep, R, msg] if schnorr else [R, Arep, msg], axis=1)))
    S = w.from_ints([(rho[i] + (h[i] if schnorr else 8 * h[i]) * k) % w.L_ORDER for i in range(n)])
    r = w.splitmix64(w.SEED_BAD, n)
    idx = np.nonzero((r & np.uint64(63)) == 0)[0]
    which = ((r[idx] >> np.uint64(6)) % np.uint64(3)).astype(np.int64)
    bit = ((r[idx] >> np.uint64(8)) % np.uint64(250)).astype(np.int64)
    for t, (arr, col0) in enumerate(((S, 0), (msg, 0), (R, 32))):
        sel = which == t
        arr[idx[sel], bit[sel] // 8 + col0] ^= (1 << (bit[sel] % 8)).astype(np.uint8)
    return A, Arep, R, S, msg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import babyjubjub_rs_amd as bjj
    n = 1 << args.log2n
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    s = st.cuda_stream
    ctx = bjj.Context(0, 0)
    lines = ["# verification against one signer's table and the generic verifier on the same inputs (key replicated), n = 2^%d items,"
             % args.log2n, "# device events; the forms alternate, %d rounds of %d calls each after 3 warm-up calls; ms per call: median of the"
             % (args.rounds, args.inner), "# rounds [smallest .. largest round]; M/s from the median; context: B8 table of %d-bit windows"
             % ctx.info().window_bits, "%-44s %-27s %8s" % ("form", "ms", "M/s")]

    def row(name, t):
        lines.append("%-44s %7.3f [%6.3f .. %6.3f] %8.1f" % (name, t[0], t[1], t[2], n / t[0] / 1e3))

    for schnorr in (False, True):
        A, Arep, R, S, msg = one_key_workload(ctx, n, schnorr)
        d = {k: torch.from_numpy(v.reshape(-1)).to(dev) for k, v in (("pk", Arep), ("R", R), ("S", S), ("msg", msg))}
        hin = torch.zeros(n * 160, dtype=torch.uint8, device=dev)
        hout = torch.empty(n * 32, dtype=torch.uint8, device=dev)
        oks = {k: torch.full((n,), 0xEE, dtype=torch.uint8, device=dev) for k in ("w16", "w23", "generic")}
        bases = {16: ctx.base(A, 16), 23: ctx.base(A, 23)}
        p = [d[k].data_ptr() for k in ("R", "S", "msg")]
        if schnorr:
            fns = {"w16": lambda: ctx.schnorr_verify_signer_dev(bases[16], *p, n, oks["w16"].data_ptr(), s),
                   "w23": lambda: ctx.schnorr_verify_signer_dev(bases[23], *p, n, oks["w23"].data_ptr(), s),
                   "generic": lambda: ctx.schnorr_verify_dev(d["pk"].data_ptr(), *p, n, oks["generic"].data_ptr(), s)}
        else:
            fns = {"w16": lambda: ctx.eddsa_verify_signer_dev(bases[16], *p, n, oks["w16"].data_ptr(), s),
                   "w23": lambda: ctx.eddsa_verify_signer_dev(bases[23], *p, n, oks["w23"].data_ptr(), s),
                   "generic": lambda: ctx.eddsa_verify_dev(d["pk"].data_ptr(), *p, n, oks["generic"].data_ptr(), s),
                   "poseidon": lambda: ctx.poseidon5_dev(hin.data_ptr(), n, hout.data_ptr(), s)}
        with torch.cuda.stream(st):
            t = measure(torch, fns, st, args.rounds, args.inner)
        torch.cuda.synchronize()
        assert bool(torch.equal(oks["w16"], oks["generic"])) and bool(torch.equal(oks["w23"], oks["generic"])), "verdicts disagree"
        good = int((oks["generic"] == 1).sum())
        stem = "bjj_schnorr_verify" if schnorr else "bjj_eddsa_verify"
        lines.append("# %s: %d of %d verdicts are 1" % ("Schnorr" if schnorr else "EdDSA", good, n))
        row(stem + "_signer_dev, signer W = 16", t["w16"])
        row(stem + "_signer_dev, signer W = 23", t["w23"])
        row(stem + "_dev, key replicated", t["generic"])
        if not schnorr:
            row("bjj_poseidon5_dev, same count (floor)", t["poseidon"])
        for b in bases.values():
            b.close()
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
