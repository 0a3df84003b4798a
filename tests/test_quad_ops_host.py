"""The model, the directed sets and the checker of the four-lane ("quad") point arithmetic (tests/quad_ref.py), judged without a
GPU.  The quad functions of csrc/k_small.hip cannot run on the CPU (DPP quad permutes, wave shuffles), so nothing here runs
them: tests/test_gpu_quad_ops.py does, on the device.  What is judged here is everything that test relies on:
  - every edge and random item is inside the domain stated at the top of quad_ref.py;
  - the exceptional cases are in the sets, asserted by property from the inputs alone;
  - the checker accepts outputs that are right by construction -- the one-item-per-lane functions of csrc/curve.hpp and
    csrc/bjj_device.hpp built by g++ (tests/emul/emul_curve_ops.cpp), run on the same records and laid out as the quad ops lay
    their outputs out -- and reports every item that a seeded mutant of the quad code would change."""
import random

import numpy as np
import pytest

import curve_ref as cr
import field_ref as fr
import quad_ref as qr
from test_curve_ops_host import clibs  # noqa: F401  (the fixture that builds the CPU library of the lane dispatcher)

R_MOD = cr.R_MOD
N_RANDOM = 512


def _rand(op, n=N_RANDOM):
    return qr.random_set(op, random.Random(0x40AD000 + qr.OPS[op]), n)


# ---- the sets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", list(qr.OPS))
def test_sets_are_inside_the_domain(op):
    edges = qr.edge_set(op)
    assert edges and len(set(edges)) == len(edges)
    out = [it for it in edges if not qr.in_domain(op, it)]
    assert not out, (op, out[:2])
    items = _rand(op)
    assert len(items) == N_RANDOM
    out = [it for it in items if not qr.in_domain(op, it)]
    assert not out, (op, out[:2])
    a, b = qr.records(op, edges)
    wa, wb, _ = qr.WIDTHS[op]
    assert a.dtype == np.uint32 and a.shape == (len(edges), wa) and (b is None) == (wb == 0)
    n = len(qr.padded(edges))
    assert n > 64 and n % 16 != 0                                            # more than one workgroup, a partly filled last one


def test_domain_rejects_what_the_producers_cannot_make():
    e = qr.edge_set("add")[0]
    big = cr.nform(6 * R_MOD)                                                # ymx at 6r: fr_sub of two coordinates stays below
    assert not qr.in_domain("add", (e[0], big + e[1][9:]))
    assert not qr.in_domain("add", (e[0], e[1][:36] + (9, 0)))
    assert not qr.in_domain("add", (cr.nform(2 * R_MOD) + e[0][9:], e[1]))
    w = qr.edge_set("walk")[0]
    assert not qr.in_domain("walk", (w[0], cr.words(1 << 254) + (64,))) and not qr.in_domain("walk", (w[0], cr.words(4) + (1,)))
    assert not qr.in_domain("fb_mul", (cr.words(cr.SUBORDER),))
    assert not qr.in_domain("affine", (cr.nform(1) * 2 + cr.nform(R_MOD) + cr.nform(0),))      # Z == 0


def _add_cases():
    """(P, Q as the loader hands it on, slot, sign) of every item of the `add` edge set, from the inputs alone"""
    out = []
    for a, b in qr.edge_set("add"):
        sg = bool(b[36] and b[37])
        X, Y, Z = cr.pniels_proj(b[:36], sg)
        zi = cr.inv(Z)
        out.append((cr.ext_affine(a), (X * zi % R_MOD, Y * zi % R_MOD), b[36], b[37]))
    return out


def test_add_set_holds_the_exceptional_pairs_in_every_slot_and_sign():
    cases = _add_cases()
    pairs = {(p, q, s) for p, q, _, s in cases}
    pts = cr.edge_points()
    for p in pts:
        for q in (cr.neg(p), p, (0, 1)):                                     # P + (-P), P + P, P + O (O + O for P = O)
            for sg in (0, 1):
                assert (p, q, sg) in pairs, (p, q, sg)
    tors = pts[:8]
    for p in tors:
        for q in tors:
            assert (p, q, 0) in pairs or (p, q, 1) in pairs
    assert {(k, s) for _, _, k, s in cases} == {(k, s) for k in range(9) for s in (0, 1)}      # every slot, both signs
    assert all(p in {c[0] for c in cases} for p in pts)
    # the lazily negated entry: a stored 2D'T of raw zero (4r - 0 is the borrowed limbs of 4r themselves) and of r, negated
    negated = [b for _, b in qr.edge_set("add") if b[36] and b[37]]
    assert any(b[18:27] == (0,) * 9 for b in negated) and any(cr.lval(b[18:27]) == R_MOD for b in negated)
    assert max(max(c - x for c, x in zip(fr.C4[:8], b[18:26])) for b in negated) >= 1 << 29       # limbs of 30 bits reach quad_add
    # entries as qfb_load hands them on, and as quad_entry makes them of an all-(+ r) point
    assert any(b[27:36] == cr.nform(qr.TWO_R1) for _, b in qr.edge_set("add"))
    ents = {b[:36] for _, b in qr.edge_set("add")}
    for q in pts:
        assert cr.to_pniels_model(sum((cr.reps(v)[1] for v in cr.ext_coords(q, 1)), ())) in ents


def test_sets_hold_the_extreme_representatives():
    for op in ("dbl", "entry", "add", "table", "walk", "affine"):
        seen = [set() for _ in range(4)]
        for it in qr.edge_set(op):
            for k, c in enumerate(cr.split(it[0], 4)):
                seen[k].add(cr.lval(c))
        for k in range(4):
            assert ({1, R_MOD - 1, R_MOD + 1, 2 * R_MOD - 1} if k == 2 else {0, 1, R_MOD - 1, R_MOD, 2 * R_MOD - 1}) <= seen[k], (op, k)
    for op in ("dbl", "entry"):                                              # all 16 combinations of canonical / + r
        exts = {it[0] for it in qr.edge_set(op)}
        for p in cr.edge_points():
            for z in cr.edge_zs(p):
                c = cr.ext_coords(p, z)
                assert all(sum((cr.reps(c[i])[(m >> i) & 1] for i in range(4)), ()) in exts for m in range(16))
    tab = {cr.ext_affine(it[0]) for it in qr.edge_set("table")}
    assert any(p[0] == 0 and p != (0, 1) for p in tab) and any(p[1] == 0 for p in tab) and (0, 1) in tab      # X = 0, Y = 0, T = 0
    xs = {cr.lval(it[0]) for it in qr.edge_set("from_ref")}
    assert 4 * R_MOD in xs and 0 in xs and R_MOD in xs and any(2 * R_MOD < x < 4 * R_MOD for x in xs)         # fr_neg's outputs


def test_ladder_sets_hold_the_carry_chains_and_the_mixed_waves():
    sc = {fr.wval(it[1][:8]) for it in qr.edge_set("walk")}
    nib = lambda d: cr.nibbles(d) % (1 << 254)                               # noqa: E731
    assert {0, 1, cr.ORDER - 1, (1 << 254) - 1, nib(8), nib(7), sum(8 << (8 * i) for i in range(32)) % (1 << 254)} <= sc
    assert cr.recode(nib(8)) == [-8] + [-7] * 62 + [1] and cr.recode(nib(7)) == [7] * 63 + [3]
    d = cr.recode(sum(8 << (8 * i) for i in range(32)) % (1 << 254))
    assert d[:4] == [-8, 1, -8, 1]                                           # a carry into every other window
    assert all(it[1][8] == 64 for it in qr.edge_set("walk"))                 # bjj_k_mul_var_base_quad's count
    pts = {cr.ext_affine(it[0]) for it in qr.edge_set("walk")}
    assert set(cr.edge_points()) <= pts
    bits = {(fr.wval(it[1][:8]).bit_length(), fr.wval(it[1][8:16]).bit_length()) for it in qr.edge_set("walk_joint")}
    assert {(a, b) for a in qr.PAIR_BITS for b in qr.PAIR_BITS} <= bits
    needs = {it[1][16] for it in qr.edge_set("walk_joint")}
    assert {1, 2, 32, 33, 34, 63} <= needs
    jw = qr.wave_jw(qr.padded(qr.edge_set("walk_joint")))
    shorter = sum(1 for it, w in zip(qr.padded(qr.edge_set("walk_joint")), jw) if it[1][16] < w)
    assert shorter > 100                                                     # items that lift the identity entry and double it
    # u P + u P and u P - u P
    same = [it for it in qr.edge_set("walk_joint") if it[1][:8] == it[1][8:16]]
    rel = {cr.ext_affine(it[0][:36]) == cr.ext_affine(it[0][36:]) for it in same} | {
        cr.ext_affine(it[0][:36]) == cr.neg(cr.ext_affine(it[0][36:])) for it in same}
    assert same and rel == {True, False}


def test_affine_identity_and_fixed_base_sets():
    quot = set()
    for (a,) in qr.edge_set("affine"):
        X, Y, Z, _ = (cr.plain(c) for c in cr.split(a, 4))
        zi = cr.inv(Z)
        quot.add((X * zi * cr.FINV % R_MOD, Y * zi % R_MOD, cr.lval(a[0:9]), cr.lval(a[9:18])))
    for v in (0, 1, R_MOD - 1):
        assert any(q[0] == v for q in quot) and any(q[1] == v for q in quot)
    assert any(q[0] == 0 and q[2] == R_MOD for q in quot)                    # a zero that fr_mul sees as r
    ids = qr.edge_set("is_identity")
    truth = [cr.plain(a[0:9]) == 0 and cr.plain(a[9:18]) == cr.plain(a[18:27]) for (a,) in ids]
    yes = [a for (a,), t in zip(ids, truth) if t]
    assert {cr.lval(a[0:9]) for a in yes} == {0, R_MOD}
    assert any(cr.lval(a[9:18]) != cr.lval(a[18:27]) for a in yes)           # Y and Z different representatives of one z
    no = [a for (a,), t in zip(ids, truth) if not t]
    assert any(cr.lval(a[0:9]) == 1 for a in no)
    assert any(cr.plain(a[0:9]) == 0 and (cr.lval(a[9:18]) - cr.lval(a[18:27])) % R_MOD in (1, R_MOD - 1) for a in no)
    assert any(cr.plain(a[0:9]) == 0 and (cr.plain(a[9:18]) + cr.plain(a[18:27])) % R_MOD == 0 for a in no)   # the order-2 point
    assert {it[0] for it in qr.edge_set("fb_load")} == {(s, g) for s in range(qr.FB_SLOTS) for g in (0, 1)}
    sc = [fr.wval(it[0]) for it in qr.edge_set("fb_mul")]
    assert {0, 1, cr.SUBORDER - 1} <= set(sc)
    digs = set()
    for s in sc:                                                             # the signed digits of digit_next, W = 8
        carry = 0
        for j in range(qr.FB_NWIN):
            u = ((s >> (8 * j)) & 255) + carry
            carry = int(u > 128)
            digs.add((256 - u) * -1 if carry else u)
    assert {0, 1, 127, 128, -127, -1} <= digs and -128 not in digs
    assert any(cr.peq(cr.padd(tuple(cr.plain(c) for c in cr.split(b, 4))[:3], cr.g0_mul(cr.LOG_B8 * fr.wval(a))), (0, 1, 1))
               for a, b in qr.edge_set("fb_add"))                            # acc = -s B8: the sum is the identity


# ---- the checker: right by construction, and the mutants -----------------------------------------------------------------------
def _lane(clibs, op, a, b=None):  # noqa: F811
    return cr.cpu_run(clibs[0], op, np.ascontiguousarray(a, dtype=np.uint32), None if b is None else np.ascontiguousarray(b, dtype=np.uint32))


def _jw_cols(items):
    return np.repeat(np.array(qr.wave_jw(items), dtype=np.uint32)[:, None], 4, axis=1)


def _mul(clibs, ext, sc):  # noqa: F811
    return _lane(clibs, "mulw64_t", ext, sc)


def _sum(clibs, acc, ext):  # noqa: F811
    """acc + ext by the lane functions: ext_to_pniels, ext_add_pn"""
    ent = _lane(clibs, "to_pniels", ext)
    return _lane(clibs, "addpn_t", acc, np.concatenate([ent, np.zeros((len(ent), 1), dtype=np.uint32)], axis=1))


def right_outputs(clibs, op, items):  # noqa: F811
    """the op's outputs by construction: the g++ lane functions on the same records (plain integers where no lane function
    gives the value), in the quad op's layout"""
    a, b = qr.records(op, items)
    if op == "dbl4":
        out = a
        for _ in range(4):
            out = _lane(clibs, "dbl_t", out)
        return out
    if op in qr.LANE_OP:
        la, lb = qr.lane_records(op, items)
        out = _lane(clibs, qr.LANE_OP[op], la, lb)
        return qr.table_from_lane(out) if op == "table" else out
    if op == "walk":
        assert all(it[1][8] == 64 for it in items)
        return np.concatenate([_mul(clibs, a, b[:, :8]), _jw_cols(items)], axis=1)
    if op == "walk_joint":
        return np.concatenate([_sum(clibs, _mul(clibs, a[:, :36], b[:, :8]), _mul(clibs, a[:, 36:], b[:, 8:16])), _jw_cols(items)], axis=1)
    if op in ("fb_mul", "fb_add"):
        b8 = np.tile(np.array(sum((cr.reps(v)[0] for v in cr.ext_coords(cr.B8M, 1)), ()), dtype=np.uint32), (len(items), 1))
        sb = _mul(clibs, b8, a)
        return sb if op == "fb_mul" else _sum(clibs, b, sb)
    if op == "affine":
        rows = []
        for (e,) in items:
            x, y = cr.ext_affine(e)
            rows.append(cr.words(x * cr.FINV % R_MOD) + cr.words(y))
        return np.array(rows, dtype=np.uint32)
    if op == "is_identity":
        return np.array([[int(cr.plain(e[0:9]) == 0 and cr.plain(e[9:18]) == cr.plain(e[18:27]))] for (e,) in items], dtype=np.uint32)
    if op == "fb_load":
        rows = []
        for ((slot, sg),) in items:
            n = sum((cr.nform(v) for v in qr.fb_entry(slot)), ()) + cr.nform(qr.TWO_R1)
            rows.append(n)
        rows = np.array(rows, dtype=np.uint32)
        neg = qr.negated_entries(rows)
        sgs = np.array([it[0][1] for it in items], dtype=bool)
        rows[sgs] = neg[sgs]
        return rows
    raise ValueError(op)


def _items(op, n=160):
    if op == "walk":
        return qr.padded(qr.edge_set(op)[::17][:n] + [it for it in _rand(op, 256) if it[1][8] == 64][:64])
    if op == "walk_joint":
        return qr.padded(qr.edge_set(op)[::29][:n] + _rand(op, 64))
    if op == "fb_load":
        return qr.padded(qr.edge_set(op)[::13])
    step = max(1, len(qr.edge_set(op)) // n)
    return qr.padded(qr.edge_set(op)[::step] + _rand(op, 64))


@pytest.mark.parametrize("op", list(qr.OPS))
def test_checker_accepts_the_lane_functions_outputs(clibs, op):  # noqa: F811
    items = _items(op)
    out = right_outputs(clibs, op, items)
    bad = qr.check(op, items, out)
    assert bad == [], (op, len(bad), [(items[i], why) for i, why in bad[:2]])
    if op not in ("is_identity",):                                           # one flipped bit per record
        wrong = out.copy()
        wrong[:, 0] ^= 1
        assert len(qr.check(op, items, wrong)) == len(items), op


def _flagged(op, items, out):
    return {i for i, _ in qr.check(op, items, out)}


def _changed(right, mutant):
    return set(np.nonzero((right != mutant).any(axis=1))[0].tolist())


def _negated_add_items():
    items = [it for it in _items("add", 400) if it[1][36] and it[1][37]]
    return qr.padded(items)


def test_mutant_ymx_ypx_not_swapped_on_a_negative_digit(clibs):  # noqa: F811
    items = _items("table")
    right = right_outputs(clibs, "table", items)
    mut = right.copy()
    for k in range(8):                                                       # d = -8 .. -1
        mut[:, 36 * k:36 * k + 9], mut[:, 36 * k + 9:36 * k + 18] = right[:, 36 * k + 9:36 * k + 18], right[:, 36 * k:36 * k + 9]
    ch = _changed(right, mut)
    assert len(ch) > len(items) // 2 and _flagged("table", items, mut) == ch
    # ... and inside an addition: the lane function negates the entry stored with ymx and ypx exchanged, which leaves the two as
    # they were stored and 2D'T negated
    items = _negated_add_items()
    a, b = qr.records("add", items)
    right = right_outputs(clibs, "add", items)
    ent = b[:, :36].copy()
    ent[:, 0:9], ent[:, 9:18] = b[:, 9:18], b[:, 0:9]
    mut = _lane(clibs, "addpn_t", a, np.concatenate([ent, np.ones((len(ent), 1), dtype=np.uint32)], axis=1))
    ch = _changed(right, mut)
    assert len(ch) > len(items) // 2 and _flagged("add", items, mut) == ch


def test_mutant_t2d_not_negated(clibs):  # noqa: F811
    items = _items("table")
    right = right_outputs(clibs, "table", items)
    mut = right.copy()
    for k in range(8):
        mut[:, 36 * k + 18:36 * k + 27] = right[:, 36 * (16 - k) + 18:36 * (16 - k) + 27]
    assert _flagged("table", items, mut) == set(range(len(items)))           # 4r - t is never t
    items = _negated_add_items()
    a, b = qr.records("add", items)
    right = right_outputs(clibs, "add", items)
    ent = b[:, :36].copy()
    ent[:, 0:9], ent[:, 9:18] = b[:, 9:18], b[:, 0:9]
    mut = _lane(clibs, "addpn_t", a, np.concatenate([ent, np.zeros((len(ent), 1), dtype=np.uint32)], axis=1))
    ch = _changed(right, mut)
    assert len(ch) > len(items) // 2 and _flagged("add", items, mut) == ch
    items = qr.padded([it for it in _items("lift_t", 400) if it[0][36] and it[0][37]])
    a, _ = qr.records("lift_t", items)
    right = right_outputs(clibs, "lift_t", items)
    ent = a[:, :36].copy()
    ent[:, 0:9], ent[:, 9:18] = a[:, 9:18], a[:, 0:9]
    mut = _lane(clibs, "pn2ext_t", np.concatenate([ent, np.zeros((len(ent), 1), dtype=np.uint32)], axis=1))
    ch = _changed(right, mut)
    assert len(ch) > len(items) // 2 and _flagged("lift_t", items, mut) == ch


@pytest.mark.parametrize("op", ["add", "walk", "walk_joint", "fb_mul", "fb_add"])
def test_mutant_t_of_the_wrong_sign(clibs, op):  # noqa: F811
    items = _items(op)
    right = right_outputs(clibs, op, items)
    mut = right.copy()
    ch = {i for i in range(len(items)) if cr.plain(tuple(right[i, 27:36].tolist())) != 0}      # -T == T only for T == 0
    for i in ch:
        mut[i, 27:36] = cr.nform(-cr.lval(right[i, 27:36].tolist()) % R_MOD)
    assert len(ch) > len(items) // 2 and _flagged(op, items, mut) == ch


def _log(e):
    return cr.log_of(cr.ext_affine(e))


def test_mutant_one_window_too_few(clibs):  # noqa: F811
    items = _items("walk")
    a, b = qr.records("walk", items)
    sc = [fr.wval(it[1][:8]) for it in items]
    hi = [(s + 8) >> 4 for s in sc]                                          # the value of the windows 63 .. 1: the walk stops before window 0
    mut = np.concatenate([_mul(clibs, a, np.array([cr.words(s) for s in hi], dtype=np.uint32)), _jw_cols(items)], axis=1)
    ch = {i for i, it in enumerate(items) if (sc[i] - hi[i]) * _log(it[0]) % cr.ORDER}
    assert len(ch) > len(items) // 2 and _flagged("walk", items, mut) == ch
    mut = right_outputs(clibs, "walk", items)                                # ... or reports one window fewer than the wave's
    mut[:, 36:40] -= 1
    assert _flagged("walk", items, mut) == set(range(len(items)))


def test_mutant_digit_off_by_one_after_a_carry(clibs):  # noqa: F811
    items = _items("walk")
    a, b = qr.records("walk", items)
    sc = [fr.wval(it[1][:8]) for it in items]
    carried = []                                                             # the lowest window a carry of s + 0x88..8 enters, or None
    for s in sc:
        w = [j for j in range(1, 63) if (s % (1 << (4 * j)) + cr.nibbles(8) % (1 << (4 * j))) >> (4 * j)]
        carried.append(w[0] if w else None)
    assert sum(c is not None for c in carried) > len(items) // 4
    wrong = [s if c is None else s - (1 << (4 * c)) for s, c in zip(sc, carried)]       # the carry dropped at that window
    keep = [i for i, s in enumerate(wrong) if 0 <= s < 1 << 254]
    mut = right_outputs(clibs, "walk", items)
    part = _mul(clibs, a[keep], np.array([cr.words(wrong[i]) for i in keep], dtype=np.uint32))
    mut[keep, :36] = part
    ch = {i for i in keep if (sc[i] - wrong[i]) * _log(items[i][0]) % cr.ORDER}
    assert len(ch) > len(items) // 8 and _flagged("walk", items, mut) == ch


def test_mutant_affine_output_plus_r(clibs):  # noqa: F811
    items = _items("affine")
    right = right_outputs(clibs, "affine", items)
    for col in (0, 8):                                                       # x, then y: the conditional subtraction left out
        mut = right.copy()
        vals = fr.vals_of_words(right[:, col:col + 8])
        mut[:, col:col + 8] = np.array([cr.words(v + R_MOD) for v in vals], dtype=np.uint32)
        assert _flagged("affine", items, mut) == set(range(len(items)))


def test_mutant_is_identity_true_for_the_order_two_point(clibs):  # noqa: F811
    items = qr.padded(qr.edge_set("is_identity"))
    right = right_outputs(clibs, "is_identity", items)
    two = {i for i, (e,) in enumerate(items) if cr.plain(e[0:9]) == 0 and (cr.plain(e[9:18]) + cr.plain(e[18:27])) % R_MOD == 0}
    assert len(two) > 16 and all(right[i, 0] == 0 for i in two)
    mut = right.copy()
    mut[sorted(two), 0] = 1                                                  # X == 0 alone, or Y == +-Z
    assert _flagged("is_identity", items, mut) == two
