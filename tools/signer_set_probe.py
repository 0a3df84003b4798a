#!/usr/bin/env python3
"""Developer tool: bjj_eddsa_verify_set_dev / bjj_schnorr_verify_set_dev against the generic verifiers on the same inputs with the
keys gathered by index, against bjj_eddsa_verify_signer_dev (one key), and against the sort-free alternative -- the items grouped
by key beforehand and one bjj_eddsa_verify_signer_dev call per key.  n = 2^20, one process, device events, the default context.
The forms of a block alternate: after three warm-up calls of each, --rounds rounds time --inner back-to-back calls of every form
between one pair of events, in an order that rotates from round to round; a row gives the median over the rounds and the smallest
and largest round.  Every pair is checked for equal bytes before its times are reported.

  python tools/signer_set_probe.py [--out profiles/signer_set.txt] [--log2n 20] [--rounds 7] [--inner 10] [--skip-64k]

Workload: the cfg-4 one under k keys -- item i belongs to signer idx[i], uniform over the set; R = rho*B8,
S = rho + 8*hm*key[idx] mod l (Schnorr: rho + h*key[idx]), 1 item in 64 with one seeded bit flipped in S, msg or R.y."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bases_probe import measure  # noqa: E402

SEED_IDX = 0x5E7A11


def set_workload(ctx, n, k, schnorr, shared):
    """(keys (k, 64), idx (n,) uint32, pk (n, 64) gathered, R, S, msg) built with the library's own fixed-base and Poseidon kernels, as
    bench.py builds cfg 4.  `shared` carries what does not depend on k (the nonces and R) from one call to the next."""
    import numpy as np
    from babyjubjub_rs_amd import workload as w
    if "rho" not in shared:
        shared["rho"] = [v % w.L_ORDER for v in w.to_ints(w.random_u256(w.SEED_NONCES, n))]
        shared["R"] = ctx.mul_fixed_base(w.from_ints(shared["rho"]))
    rho, R = shared["rho"], shared["R"].copy()
    key = [v % w.L_ORDER for v in w.to_ints(w.random_u256(w.SEED_KEYS, k))]
    keys = ctx.mul_fixed_base(w.from_ints(key))
    idx = (w.splitmix64(SEED_IDX, n) % np.uint64(k)).astype(np.uint32)
    pk = np.ascontiguousarray(keys[idx])
    msg = w.random_u256(w.SEED_MSGS, n, top_bits_cleared=3)
    h = w.to_ints(ctx.poseidon5(np.concatenate([pk, R, msg] if schnorr else [R, pk, msg], axis=1)))
    ix = idx.tolist()
    S = w.from_ints([(rho[i] + (h[i] if schnorr else 8 * h[i]) * key[ix[i]]) % w.L_ORDER for i in range(n)])
    r = w.splitmix64(w.SEED_BAD, n)
    bad = np.nonzero((r & np.uint64(63)) == 0)[0]
    which = ((r[bad] >> np.uint64(6)) % np.uint64(3)).astype(np.int64)
    bit = ((r[bad] >> np.uint64(8)) % np.uint64(250)).astype(np.int64)
    for t, (arr, col0) in enumerate(((S, 0), (msg, 0), (R, 32))):
        sel = which == t
        arr[bad[sel], bit[sel] // 8 + col0] ^= (1 << (bit[sel] % 8)).astype(np.uint8)
    return keys, idx, pk, R, S, msg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--skip-64k", action="store_true", help="leave out the set of 65 536 signers (34.6 GB)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import babyjubjub_rs_amd as bjj
    n = 1 << args.log2n
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    s = st.cuda_stream
    ctx = bjj.Context(0, 0)
    lines = ["# verification against a set of signers' tables, by per-item index, and the generic verifier on the same inputs (keys",
             "# gathered by index), n = 2^%d items, indices uniform over the set, device events; the forms of a block alternate, %d rounds"
             % (args.log2n, args.rounds), "# of %d calls each after 3 warm-up calls; ms per call: median of the rounds [smallest .. largest round]; M/s"
             % args.inner, "# from the median; context: B8 table of %d-bit windows" % ctx.info().window_bits,
             "%-58s %-27s %8s" % ("form", "ms", "M/s")]

    def row(name, t):
        lines.append("%-58s %7.3f [%6.3f .. %6.3f] %8.1f" % (name, t[0], t[1], t[2], n / t[0] / 1e3))

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)

    shared = {}
    configs = [(1, 16, False), (256, 12, False), (4096, 8, False), (4096, 8, True)] + ([] if args.skip_64k else [(65536, 8, False)])
    for k, W, schnorr in configs:
        keys, idx, pk, R, S, msg = set_workload(ctx, n, k, schnorr, shared)
        stem = "bjj_schnorr_verify" if schnorr else "bjj_eddsa_verify"
        try:
            sset = ctx.signer_set(keys, W)
        except bjj.BjjError as e:
            lines.append("# %s_set_dev, k = %d, W = %d: not measured, the set could not be created (%s)" % (stem, k, W, e))
            continue
        d = {name: up(v) for name, v in (("idx", idx), ("pk", pk), ("R", R), ("S", S), ("msg", msg))}
        oks = {name: torch.full((n,), 0xEE, dtype=torch.uint8, device=dev) for name in ("set", "generic", "signer", "grouped")}
        p = [d[name].data_ptr() for name in ("R", "S", "msg")]
        set_fn = ctx.schnorr_verify_set_dev if schnorr else ctx.eddsa_verify_set_dev
        gen_fn = ctx.schnorr_verify_dev if schnorr else ctx.eddsa_verify_dev
        fns = {"set": lambda: set_fn(sset, d["idx"].data_ptr(), *p, n, oks["set"].data_ptr(), s),
               "generic": lambda: gen_fn(d["pk"].data_ptr(), *p, n, oks["generic"].data_ptr(), s)}
        bases = []
        if k == 1:                                          # the one-key path on the same items
            bases = [ctx.base(keys[0], 16)]
            fns["signer"] = lambda: ctx.eddsa_verify_signer_dev(bases[0], *p, n, oks["signer"].data_ptr(), s)
        if k == 256 and not schnorr:                        # the sort-free alternative: grouped by key beforehand, one call per key
            order = np.argsort(idx, kind="stable")
            g = {name: up(v[order]) for name, v in (("R", R), ("S", S), ("msg", msg))}
            start = np.searchsorted(idx[order], np.arange(k + 1))
            bases = [ctx.base(keys[j], 16) for j in range(k)]
            gp = [g[name].data_ptr() for name in ("R", "S", "msg")]
            okp = oks["grouped"].data_ptr()

            def grouped():
                for j in range(k):
                    a, cnt = int(start[j]), int(start[j + 1] - start[j])
                    ctx.eddsa_verify_signer_dev(bases[j], gp[0] + a * 64, gp[1] + a * 32, gp[2] + a * 32, cnt, okp + a, s)
            fns["grouped"] = grouped
        with torch.cuda.stream(st):
            t = measure(torch, fns, st, args.rounds, args.inner)
        torch.cuda.synchronize()
        assert bool(torch.equal(oks["set"], oks["generic"])), "verdicts disagree (set, k = %d)" % k
        if "signer" in fns:
            assert bool(torch.equal(oks["signer"], oks["generic"])), "verdicts disagree (signer)"
        if "grouped" in fns:
            assert bool(torch.equal(oks["grouped"].cpu(), oks["generic"].cpu()[torch.from_numpy(order)])), "verdicts disagree (grouped)"
        good = int((oks["generic"] == 1).sum())
        lines.append("# %s, k = %d: %d of %d verdicts are 1; the set's tables: %.1f MB" % ("Schnorr" if schnorr else "EdDSA", k, good, n,
                                                                                        sset.info()[3] / 1e6))
        row("%s_set_dev, k = %d, W = %d" % (stem, k, W), t["set"])
        row("%s_dev, keys gathered (baseline), k = %d" % (stem, k), t["generic"])
        if "signer" in fns:
            row("%s_signer_dev, the one key, W = 16" % stem, t["signer"])
        if "grouped" in fns:
            row("%d x %s_signer_dev, items grouped by key, W = 16" % (k, stem), t["grouped"])
        spread = max(t["set"][2] - t["set"][1], t["generic"][2] - t["generic"][1])
        lines.append("#   generic - set = %.3f ms (%.2fx); largest round-to-round spread of the two rows: %.3f ms"
                     % (t["generic"][0] - t["set"][0], t["generic"][0] / t["set"][0], spread))
        for b in bases:
            b.close()
        sset.close()
        del d, oks
        torch.cuda.empty_cache()
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
