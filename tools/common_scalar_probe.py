#!/usr/bin/env python3
"""Developer tool: the shared-scalar kernel (bjj_mul_common_dev, bjj_in_subgroup_dev, bjj_elgamal_decrypt_dev) at n = 2^20 points of
the prime-order subgroup beside the calls it replaces, with device events in one process on the same inputs.  Three contexts of
the one process differ only in BJJ_COMMON_FORM (read at bjj_init): table-free forced, table forced, and the rule's choice -- the
yardsticks run in the third.  Rows:
  1  full-width random k: both forced forms against bjj_mul_var_base_dev with k replicated
  2  the same with an addend and subtraction against bjj_mul_var_base_dev + bjj_point_add_dev
  3  k = 8, a 64-bit and a 128-bit k against the same K2 call
  4  bjj_in_subgroup_dev against bjj_mul_var_base_dev with l
  5  bjj_elgamal_decrypt_dev at the default table and 32 range bits, all found and none found, against the three device calls
No device call negates a point, so the compositions of rows 2 and 5 get their negation FOR FREE: they multiply a copy of the
points that was negated on the host, outside the timed region.  The forms of a row alternate as in dlog_probe.py: three warm-up
calls each, then --rounds rounds of --inner back-to-back calls between one pair of events; a row is the median of the rounds with
the smallest and the largest.  Every result is compared with its yardstick before its time is printed.

  python tools/common_scalar_probe.py [--out profiles/common_scalar.txt] [--log2n 20] [--rounds 7] [--inner 3] [--rows 1,2,3,4,5]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dlog_probe import measure  # noqa: E402

L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
FULL = 0x2A6D5E0F1B3C7A9948D1C0E2F3B4A59687766554433221100FFEEDDCCBBAA998
K64 = 0xD1B54A32D192ED03
K128 = 0x9E3779B97F4A7C15F39CC0605CEDC834
SK = 0x05A1B2C3D4E5F60718293A4B5C6D7E8F9A0B1C2D3E4F5061728394A5B6C7D8E9 % L


def context(bjj, form):
    old = os.environ.get("BJJ_COMMON_FORM")
    os.environ.pop("BJJ_COMMON_FORM", None)
    if form:
        os.environ["BJJ_COMMON_FORM"] = form
    try:
        return bjj.Context(0, 16)
    finally:
        os.environ.pop("BJJ_COMMON_FORM", None)
        if old is not None:
            os.environ["BJJ_COMMON_FORM"] = old


def counts(k):
    """(weight of the NAF, weight of the width-5 NAF, the two multiplication counts) as common_scalar.hpp counts them"""
    def weight(w):
        v, c = k % (8 * L), 0
        while v:
            if v & 1:
                d = v & ((1 << w) - 1)
                if d >= 1 << (w - 1):
                    d -= 1 << w
                v -= d
                c += 1
            v >>= 1
        return c
    a, b = weight(2), weight(5)
    return a, b, 7 * a, 73 + 8 * b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--rows", default="1,2,3,4,5")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import babyjubjub_rs_amd as bjj
    from babyjubjub_rs_amd import api, workload as w
    lg = args.log2n
    n = 1 << lg
    rows = set(args.rows.split(","))
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    s = st.cuda_stream
    ctxs = {"table-free": context(bjj, "naf"), "table": context(bjj, "table"), "rule": context(bjj, None)}
    ref = ctxs["rule"]
    lines = ["# one scalar, many points: n = 2^%d points of the prime-order subgroup, device events; ms per call: median of %d rounds of %d"
             % (lg, args.rounds, args.inner),
             "# calls after 3 warm-up calls [smallest .. largest round]; M items/s from the median.  table-free / table: BJJ_COMMON_FORM",
             "# forced; rule: the form the multiplication count picks.  K2: bjj_mul_var_base_dev with the scalar replicated n times.",
             "# The compositions of rows 2 and 5 get their negation for free (a copy of the points negated on the host, untimed): no",
             "# device call negates.  new / yardstick: largest round of the new call against the smallest round of the yardstick.",
             "%-72s %-29s %8s" % ("row / form", "ms", "M/s")]

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)

    def le(k):
        return np.frombuffer(int(k).to_bytes(32, "little"), np.uint8)

    def emit(name, t, new, yard):
        for f in t:
            lines.append("%-72s %8.3f [%7.3f .. %7.3f] %8.2f" % (name + ": " + f, t[f][0], t[f][1], t[f][2], n / t[f][0] / 1e3))
        for f in new:
            lines.append("%-72s %8.2fx (median / median; largest %s round against smallest %s round: %.2fx)"
                         % (name + ": " + yard + " / " + f, t[yard][0] / t[f][0], f, yard, t[yard][1] / t[f][2]))
        sys.stdout.write("\n".join(lines[-len(t) - len(new):]) + "\n")
        sys.stdout.flush()

    pts = ref.mul_fixed_base(w.scalars_254(n, 0xC5))           # points of the prime-order subgroup
    add = ref.mul_fixed_base(w.scalars_254(n, 0xC6))
    d_pts, d_neg, d_add = up(pts), up(api._negate_x(pts)), up(add)
    d_sc = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    d_tmp = torch.empty(n * 64, dtype=torch.uint8, device=dev)
    outs = {f: torch.empty(n * 64, dtype=torch.uint8, device=dev) for f in ("table-free", "table", "rule", "yard")}
    oks = {f: torch.empty(n, dtype=torch.uint8, device=dev) for f in outs}

    def replicate(k):
        d_sc.copy_(up(np.tile(le(k), n)))
        torch.cuda.synchronize()

    def mul_rows(name, k, forms, with_add):
        replicate(k)
        fns = {}
        for f in forms:
            fns[f] = (lambda f=f: ctxs[f].mul_common_dev(k, d_pts.data_ptr(), d_add.data_ptr() if with_add else None, n, outs[f].data_ptr(),
                                                         oks[f].data_ptr(), with_add, s))
        if with_add:
            def yard():
                ref.mul_var_base_dev(d_neg.data_ptr(), d_sc.data_ptr(), n, d_tmp.data_ptr(), s)
                ref.point_add_dev(d_add.data_ptr(), d_tmp.data_ptr(), n, outs["yard"].data_ptr(), s)
            fns["K2 + point_add"] = yard
        else:
            fns["K2"] = lambda: ref.mul_var_base_dev(d_pts.data_ptr(), d_sc.data_ptr(), n, outs["yard"].data_ptr(), s)
        for f in forms:
            outs[f].fill_(0xEE)
        with torch.cuda.stream(st):
            t = measure(torch, fns, st, args.rounds, args.inner)
        torch.cuda.synchronize()
        for f in forms:
            assert bool((oks[f] == 1).all()) and bool((outs[f] == outs["yard"]).all()), "%s: %s differs from its yardstick" % (name, f)
        a, b, ca, cb = counts(k)
        lines.append("# %s: NAF weight %d = %d multiplications, width-5 weight %d = %d multiplications (doublings apart)" % (name, a, ca, b, cb))
        emit(name, t, forms, "K2 + point_add" if with_add else "K2")

    if "1" in rows:
        mul_rows("1 full-width k", FULL, ["table-free", "table"], False)
    if "2" in rows:
        mul_rows("2 full-width k, A - k P", FULL, ["table-free", "table"], True)
    if "3" in rows:
        for nm, k in (("3 k = 8", 8), ("3 64-bit k", K64), ("3 128-bit k", K128)):
            mul_rows(nm, k, ["table-free", "table", "rule"], False)
    if "4" in rows:
        replicate(L)
        fns = {f: (lambda f=f: ctxs[f].in_subgroup_dev(d_pts.data_ptr(), n, oks[f].data_ptr(), s)) for f in ("table-free", "table", "rule")}
        fns["K2"] = lambda: ref.mul_var_base_dev(d_pts.data_ptr(), d_sc.data_ptr(), n, outs["yard"].data_ptr(), s)
        with torch.cuda.stream(st):
            t = measure(torch, fns, st, args.rounds, args.inner)
        torch.cuda.synchronize()
        ident = up(np.tile(np.concatenate([le(0), le(1)]), n))
        assert bool((outs["yard"] == ident).all()), "l * P is not the identity for a subgroup point"
        for f in ("table-free", "table", "rule"):
            assert bool((oks[f] == 1).all()), "bjj_in_subgroup_dev (%s) differs from K2 with l" % f
        a, b, ca, cb = counts(L)
        lines.append("# 4 k = l: NAF weight %d = %d multiplications, width-5 weight %d = %d multiplications" % (a, ca, b, cb))
        emit("4 in_subgroup", t, ["table-free", "table", "rule"], "K2")
    if "5" in rows:
        rb = 32
        ms = (w.splitmix64(0xE1, n) & np.uint64(0xFFFFFFFF)).astype(np.uint64)
        rs = w.scalars_254(n, 0xC7)
        pk = ref.mul_fixed_base(le(SK)).reshape(-1)
        base = ref.base((int.from_bytes(bytes(pk[:32]), "little"), int.from_bytes(bytes(pk[32:]), "little")), 0)
        mrec = np.zeros((n, 32), np.uint8)
        mrec[:, :8] = ms.view(np.uint8).reshape(n, 8)
        c1 = ref.mul_fixed_base(rs)
        c2 = ref.mul_bases([None, base], [mrec, rs])
        base.close()
        d_c1, d_c1n, d_c2 = up(c1), up(api._negate_x(c1)), up(c2)
        tables = {f: ctxs[f].dlog_table(None, 0) for f in ("table-free", "table", "rule")}
        d_m = {f: torch.empty(n, dtype=torch.int64, device=dev) for f in ("table-free", "table", "rule", "yard")}
        for label, key in (("all found", SK), ("none found", (SK + 1) % L)):
            replicate(key)
            fns = {f: (lambda f=f: ctxs[f].decrypt_dev(tables[f], key, d_c1.data_ptr(), d_c2.data_ptr(), n, rb, d_m[f].data_ptr(),
                                                       oks[f].data_ptr(), s)) for f in ("table-free", "table", "rule")}

            def yard():
                ref.mul_var_base_dev(d_c1n.data_ptr(), d_sc.data_ptr(), n, d_tmp.data_ptr(), s)
                ref.point_add_dev(d_c2.data_ptr(), d_tmp.data_ptr(), n, outs["yard"].data_ptr(), s)
                ref.dlog_dev(tables["rule"], outs["yard"].data_ptr(), n, rb, d_m["yard"].data_ptr(), oks["yard"].data_ptr(), s)
            fns["K2 + point_add + dlog"] = yard
            with torch.cuda.stream(st):
                t = measure(torch, fns, st, args.rounds, args.inner)
            torch.cuda.synchronize()
            found = key == SK
            assert bool((oks["yard"] == (1 if found else 0)).all()), "the composition: ok"
            if found:
                assert bool((d_m["yard"].cpu() == torch.from_numpy(ms.view(np.int64))).all()), "the composition: m"
            for f in ("table-free", "table", "rule"):
                assert bool((oks[f] == oks["yard"]).all()) and bool((d_m[f] == d_m["yard"]).all()), "decrypt (%s) differs from the composition" % f
            emit("5 decrypt, 24-bit table, 32 range bits, %s" % label, t, ["table-free", "table", "rule"], "K2 + point_add + dlog")
        for f, t_ in tables.items():
            t_.close()
    for c in ctxs.values():
        c.close()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
