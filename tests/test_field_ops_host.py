"""The additive, comparison, conversion, square-root and codec field code (csrc/fr.hpp, csrc/bjj_device.hpp:536-659, ref_on_curve)
on the CPU: the dispatcher of tests/devfuzz/field_ops.hpp built by g++ with the bound assertions live
(tests/emul/emul_field_ops.cpp), on the directed edge sets of tests/field_ref.py plus 2^14 seeded random items per op, against
plain integers.  The edge sets hold what random data never produces: subtrahends equal to the borrowed constants limb for
limb, the representatives k r and k r +- 1 of zero up to 16 r, top limbs at the multiples of fr_reduce_weak's divisor, single
bits at the limb and word boundaries, (r - 1) / 2 and (r + 1) / 2, r +- 2^(32 j), every digit of the square root's discrete log
on its own.  tests/test_gpu_field_ops.py runs the same sets on the device.

The library is built with BJJ_DEBUG_BOUNDS, so an operand outside a function's contract -- which is also what a borrowed constant
that is too small in the header makes of an in-contract operand -- fails one of the BJJ_ASSERTs of csrc/fr.hpp: the whole pytest
process aborts (exit status 134) with the assertion's file and line.  That abort is the expected form of failure for a contract
violation; every other error is an ordinary failing assertion of the op's test."""
import ctypes
import os
import random

import numpy as np
import pytest

import field_ref as fr
import hostbuild
from conftest import ROOT

N_RANDOM = 1 << 14


@pytest.fixture(scope="module")
def flib():
    """the dispatcher of tests/devfuzz/field_ops.hpp built for the CPU"""
    lib = ctypes.CDLL(hostbuild.shared("libbjj_emul_field_ops.so", os.path.join(ROOT, "tests", "emul", "emul_field_ops.cpp")))
    for op, code in fr.OPS.items():
        assert tuple(lib.emul_field_words(code, k) for k in range(3)) == fr.WIDTHS[op], op
    return lib


# ---- the model against itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", list(fr.OPS))
def test_model_sets_are_inside_the_domain(op):
    edges = fr.edge_set(op)
    assert edges and len(set(edges)) == len(edges)
    out = [it for it in edges if not fr.in_domain(op, it)]
    assert not out, (op, out[:2])
    rnd_items = fr.random_set(op, random.Random(0xD0 + fr.OPS[op]), 2048)
    assert len(rnd_items) == 2048                                          # nothing rejected, nothing left out
    out = [it for it in rnd_items if not fr.in_domain(op, it)]
    assert not out, (op, out[:2])
    a, b = fr.records(op, edges)                                           # records round trip
    wa, wb, _ = fr.WIDTHS[op]
    assert a.dtype == np.uint32 and a.shape == (len(edges), wa) and (b is None) == (wb == 0)
    assert fr.items_of(op, a, b) == edges
    vec = fr.vals_of_limbs if wa == 9 else fr.vals_of_words
    one = fr.lval if wa == 9 else fr.wval
    assert vec(a) == [one(it[0]) for it in edges]


def test_model_constants():
    r = fr.R_MOD
    assert fr.TOP_R == 3171406 and fr.TOP_DIV == 3171407 and fr.R1 * fr.RINV % r == 1
    for C, k in ((fr.C4, 4), (fr.C8, 8), (fr.K8, 8)):
        assert fr.lval(C) == k * r
    assert all(c >= fr.M29 for c in fr.C4[:8]) and all(c >= fr.M29 for c in fr.C8[:8]) and all(c >= fr.ONES30 for c in fr.K8[:8])
    assert pow(fr.TS_G, 1 << 27, r) == r - 1                                # G has order 2^28 exactly
    assert fr.on_curve(*fr.B8) and all(fr.on_curve(*p) for p in fr.golden_points("torsion_points"))
    assert len(fr.golden_points("torsion_points")) == 8
    assert not fr.on_curve(0, 0) and fr.on_curve(0, 1) and fr.on_curve(0, r - 1)
    base = set([(0, 1), (0, r - 1), fr.B8] + fr.golden_points("torsion_points"))
    assert len(base) == 9                                                    # the torsion points hold the identity and (0, -1)
    assert {p for p in fr.curve_edge_points() if fr.on_curve(*p)} == base    # a step of 1 in x or y always leaves the curve
    assert len(fr.curve_edge_points()) > 4 * len(base)
    assert all(fr.on_curve(*p) for p in fr.curve_pool()[::37])
    assert not fr.y_of_x(fr.HALF) and len(fr.y_of_x(fr.HALF - 1)) == 2


def test_model_edge_sets_hold_the_directed_edges():
    # the sub family: the largest top limb over all-ones limbs, the borrowed constant limb for limb, b = 0, a = 0, a all 2^30 - 1
    for op, C, ones in (("sub", fr.C4, fr.M29), ("sub_lazy", fr.C4, fr.M29), ("sub8", fr.C8, fr.M29), ("sub8_of_lazy", fr.K8, fr.ONES30)):
        edges = set(fr.edge_set(op))
        zero, full = (0,) * 9, (fr.ONES30,) * 9
        for b in ((ones,) * 8 + (C[8],), tuple(C), zero):
            assert (zero, b) in edges and (full, b) in edges, (op, b)
    assert {(tuple(fr.C4),), ((0,) * 9,), ((fr.M29,) * 8 + (fr.C4[8],),)} <= set(fr.edge_set("neg"))
    # reduce_weak: top limbs 3171407 k - 1, 3171407 k, 3171407 k + 1 over all-zero and all-ones limbs
    tops = {(it[0][8], it[0][0]) for it in fr.edge_set("reduce_weak")}
    for k in range(22):
        for d in (-1, 0, 1):
            t = 3171407 * k + d
            if 0 <= t < 1 << 26:
                assert (t, 0) in tops and (t, fr.M29) in tops, t
    # canon / is_zero: k r and k r +- 1 for k = 0 .. 15, and 16 r - 1
    v = {fr.lval(it[0]) for it in fr.edge_set("canon")}
    assert {k * fr.R_MOD + d for k in range(16) for d in (-1, 0, 1) if k or d >= 0} | {16 * fr.R_MOD - 1} <= v
    # eq: every k that keeps a = b + k r in [0, 12 r), with +- 1, b at its largest, a = 12 r - 1
    eq = {(fr.lval(a), fr.lval(b)) for a, b in fr.edge_set("eq")}
    bmax = fr.lval((fr.M29,) * 8 + (fr.C4[8],))
    for b in (0, fr.R_MOD, bmax):
        for k in range(-4, 13):
            for d in (-1, 0, 1):
                if 0 <= b + k * fr.R_MOD + d < 12 * fr.R_MOD:
                    assert (b + k * fr.R_MOD + d, b) in eq
        assert (12 * fr.R_MOD - 1, b) in eq
    # words: r +- 2^(32 j); gt_halfq: (r - 1) / 2 and (r + 1) / 2
    w = {fr.wval(it[0]) for it in fr.edge_set("words_ge_r")}
    assert {0, (1 << 256) - 1, fr.R_MOD - 1, fr.R_MOD, fr.R_MOD + 1} | {fr.R_MOD + s * (1 << (32 * j)) for j in range(1, 8) for s in (1, -1)} <= w
    assert {1 << (29 * i) for i in range(1, 9)} | {1 << (32 * j) for j in range(1, 8)} <= w
    assert {fr.HALF, fr.HALF + 1} <= {fr.lval(it[0]) for it in fr.edge_set("gt_halfq")}
    fm = {fr.lval(it[0]) for it in fr.edge_set("from_mont")}
    assert {0, fr.R_MOD, fr.R1, fr.R1 + fr.R_MOD, fr.mont(fr.R_MOD - 1), fr.mont(fr.R_MOD - 1) + fr.R_MOD} <= fm
    # compress: the sign threshold in both representatives crossed with the y edges
    c = {(fr.wval(x), fr.wval(y)) for x, y in fr.edge_set("compress")}
    assert {(x, y) for x in fr.COMPRESS_X for y in fr.COMPRESS_Y} <= c


def test_model_sqrt_edges_reach_every_digit_table_entry():
    """from the inputs alone: every discrete log with a single non-zero digit -- each entry of the four 7-bit digit tables on its
    own -- is the log of a^s for some sqrt edge item, in both representatives; so are a digit at 127 beside zero digits, the
    log 2^28 - 2, and the non-residues G a"""
    edges = fr.edge_set("sqrt")
    assert fr.sqrt_logs_present(edges) == set(fr.SQRT_SINGLE_DIGIT_LOGS)
    assert len(fr.SQRT_SINGLE_DIGIT_LOGS) == 448
    # and every digit at the positions 0 .. 2 under non-zero higher digits: what makes a wrong stripping-table entry show
    strip = fr.SQRT_STRIP_LOGS
    assert fr.sqrt_logs_present(edges, strip) == set(strip) and len(set(strip)) == 64 + 128 + 128
    digit = lambda e, k: (e >> (7 * k)) & 127                                  # noqa: E731
    assert {(d, digit(e, d)) for e in strip for d in range(3) if e & ((1 << (7 * d)) - 1) == 0 and all(digit(e, k) for k in range(d + 1, 4))
            } >= {(d, v) for d in range(3) for v in range(128) if d or v % 2 == 0}
    canon = [it for it in edges if fr.lval(it[0]) < fr.R_MOD]
    wide = [it for it in edges if fr.lval(it[0]) >= fr.R_MOD]
    assert fr.sqrt_logs_present(canon) == fr.sqrt_logs_present(wide) == set(fr.SQRT_SINGLE_DIGIT_LOGS)
    plain = {fr.lval(it[0]) * fr.RINV % fr.R_MOD for it in edges}
    for e in ((1 << 28) - 2, 127 << 7 | 127 << 21, 126 | 127 << 14):
        assert any(pow(a, fr.TS_S, fr.R_MOD) == pow(fr.TS_G, e, fr.R_MOD) for a in plain if a), e
    assert ((0,) * 9,) in edges and (fr.nform(fr.R_MOD),) in edges
    nres = sum(1 for a in plain if a and not fr.is_residue(a))
    assert nres >= 448 and {1, fr.R_MOD - 1, 4} <= plain


# ---- the shipped functions, built by g++, against the model --------------------------------------------------------------------
@pytest.mark.parametrize("op", list(fr.OPS))
def test_field_op_edges_and_random(flib, op):
    edges = fr.edge_set(op)
    a, b = fr.records(op, edges)
    bad = fr.check(op, edges, fr.cpu_run(flib, op, a, b))
    assert bad == [], (op, "edges", len(bad), [(edges[i], why) for i, why in bad[:3]])
    items = fr.random_set(op, random.Random(0xF1E1D000 + fr.OPS[op]), N_RANDOM)
    a, b = fr.records(op, items)
    bad = fr.check(op, items, fr.cpu_run(flib, op, a, b))
    assert bad == [], (op, "random", len(bad), [(items[i], why) for i, why in bad[:3]])


def test_check_rejects_wrong_outputs(flib):
    """the checker itself: one wrong bit, a non-canonical limb split of the right value, or a flipped verdict is reported"""
    for op in ("sub", "canon", "reduce_weak", "to_words", "is_zero", "eq", "sqrt", "decompress", "compress", "add_lazy"):
        items = fr.edge_set(op)[:64]
        a, b = fr.records(op, items)
        out = fr.cpu_run(flib, op, a, b)
        assert fr.check(op, items, out) == []
        wrong = out.copy()
        wrong[:, 0] ^= 1
        assert len(fr.check(op, items, wrong)) == len(items), op
    items = [it for it in fr.edge_set("sub") if it[0][0] < fr.M29][:32]          # same value, a limb of 30 bits: not N-form
    a, b = fr.records("sub", items)
    out = fr.cpu_run(flib, "sub", a, b)
    keep = out[:, 1] > 0
    out[keep, 0] += 1 << 29
    out[keep, 1] -= 1
    assert len(fr.check("sub", items, out)) == int(keep.sum()) > 0
