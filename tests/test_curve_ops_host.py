"""The group law and the per-lane table, ladder and fixed-table code (csrc/curve.hpp; csrc/bjj_device.hpp: niels_cneg_lazy,
vb_build_table .. vb_mul_windowed, ref_mul_scalar, fixed_table_entry / _chain / _check_slot, var_base_item) on the CPU: the
dispatcher of tests/devfuzz/curve_ops.hpp built by g++ with the bound assertions live (tests/emul/emul_curve_ops.cpp), in both
per-lane table layouts, on the directed sets of tests/curve_ref.py plus 2^12 seeded random items per op, against plain integers.
The directed sets hold what a random walk over multiples of one generator never produces: P + (-P), P + P and P + O for the
eight torsion points, B8, -B8, 2 B8 and B8 + T for T of order 2, 4 and 8; every pair of torsion points; coordinates whose
Montgomery representative is 0, 1, r - 1 or 2r - 1; the carry-less negated entries of niels_cneg_lazy / pniels_cneg; ladder
scalars whose recoding carries through all 64 windows; operands of the reference's addition whose denominator vanishes.
tests/test_gpu_curve_ops.py runs the same sets on the device.

The libraries are built with BJJ_DEBUG_BOUNDS, so an operand outside a function's contract -- which is also what a wrong lazy-limb
bound in a formula makes of an in-contract input -- fails one of the BJJ_ASSERTs of csrc/fr.hpp: the whole pytest process aborts
(exit status 134) with the assertion's file and line.  That abort is the expected form of failure for a contract violation;
every other error is an ordinary failing assertion of the op's test."""
import ctypes
import os
import random

import numpy as np
import pytest

import curve_ref as cr
import hostbuild
from conftest import ROOT

R_MOD = cr.R_MOD
N_RANDOM = 1 << 12


def build_clib(layout):
    """the dispatcher of tests/devfuzz/curve_ops.hpp built for the CPU, per per-lane table layout"""
    lib = ctypes.CDLL(hostbuild.shared("libbjj_emul_curve_ops_l%d.so" % layout, os.path.join(ROOT, "tests", "emul", "emul_curve_ops.cpp"),
                                       defines=("BJJ_PNIELS_LAYOUT=%d" % layout,)))
    assert lib.emul_curve_layout() == layout
    for op, code in cr.OPS.items():
        assert tuple(lib.emul_curve_words(code, k) for k in range(4)) == cr.WIDTHS[op], op
    return lib


@pytest.fixture(scope="module")
def clibs():
    """the CPU libraries of the dispatcher: [raw per-lane tables, packed per-lane tables]"""
    return [build_clib(0), build_clib(1)]


LAYOUT_OPS = ("table", "table_affine", "var_base") + tuple(cr.MULW)        # the ops that go through a per-lane table


# ---- the model against itself ---------------------------------------------------------------------------------------------
def test_model_constants_and_edge_points(pyoracle):
    r = R_MOD
    assert cr.F * cr.F % r == -cr.A_REF % r and cr.F < r - cr.F and cr.DP * cr.A_REF % r == -cr.D_REF % r
    assert pow(cr.DP, (r - 1) // 2, r) == r - 1                               # D' a non-residue: the law is complete
    assert cr.SUBORDER == pyoracle.SUBORDER and cr.ORDER == pyoracle.ORDER
    assert cr.smul_m1(cr.G0, cr.LOG_B8) == cr.B8M and cr.smul_m1(cr.G0, cr.LOG_T8) == cr.T8
    assert cr.smul_m1(cr.G0, cr.ORDER) == (0, 1) and cr.smul_m1(cr.G0, cr.SUBORDER) != (0, 1) and cr.smul_m1(cr.G0, cr.ORDER // 2) != (0, 1)
    pts = cr.edge_points()
    assert len(pts) == len(set(pts)) == 19 and all(cr.on_m1(p) for p in pts) and all(cr.on_ref(p) for p in cr.ref_edge_points())
    tors = pts[:8]
    assert tors == [cr.to_m1(p) for p in cr.TORSION_REF] and len(set(tors)) == 8
    assert tors[0] == (0, 1) and tors[4] == (0, r - 1) and tors[2][1] == 0 and tors[6][1] == 0
    assert [cr.smul_m1(cr.T8, j) for j in range(8)] == tors
    b8 = cr.B8M
    assert pts[8:11] == [b8, cr.neg(b8), cr.add_m1(b8, b8)] and cr.smul_m1(b8, cr.SUBORDER - 1) == cr.neg(b8)
    assert pts[11:17] == [q for j in (4, 2, 1) for q in (cr.add_m1(b8, tors[j]), cr.neg(cr.add_m1(b8, tors[j])))]
    for p in pts[17:]:                                                       # the seeded points generate the whole group
        assert cr.smul_m1(p, cr.SUBORDER) != (0, 1) and cr.smul_m1(p, cr.ORDER // 2) != (0, 1) and cr.smul_m1(p, cr.ORDER) == (0, 1)
    # the table-driven multiple and the known logs against plain double-and-add
    rnd = random.Random(5)
    for p in pts + cr.pool()[:6]:
        s = rnd.randrange(1 << 254)
        assert cr.log_of(p) is not None and cr.peq(cr.smul_known(p, s), cr.smul_m1(p, s % cr.ORDER) + (1,))
    # the model's statement of the reference's projective code is the oracle's
    for p, q, _ in cr.vanishing_pairs():
        assert cr.proj_add(p, q) == pyoracle.proj_add(p, q) and pyoracle.proj_affine(pyoracle.proj_add(p, q)) == (0, 0)
    for p in cr.ref_edge_points()[:4]:
        assert cr.mul_scalar(p, 0x1234567) == pyoracle.mul_scalar(p, 0x1234567)
    # the a' = -1 law is the reference's law carried over by x' = F x
    for p in pts[8:12]:
        for q in pts[:12]:
            assert cr.from_m1(cr.add_m1(p, q)) == pyoracle.proj_affine(pyoracle.proj_add(cr.from_m1(p) + (1,), cr.from_m1(q) + (1,)))


def test_no_point_doubles_into_a_vanishing_denominator():
    """the first doubling of the reference's loop has f = 0 (g = 0) only if D x^2 y^2 == 1 (== -1): D is a non-residue and both 1
    and -1 are residues mod r, so no (x, y) does either -- the vanishing denominators exist in the PAIR form only
    (curve_ref.vanishing_pairs), and tests/test_gpu_curve_ops.py keeps to that form"""
    h = (R_MOD - 1) // 2
    assert pow(cr.D_REF, h, R_MOD) == R_MOD - 1 and pow(R_MOD - 1, h, R_MOD) == 1
    fs = [w for _, _, w in cr.vanishing_pairs()]
    assert fs.count("f") >= 3 and fs.count("g") >= 3
    for p, q, w in cr.vanishing_pairs():
        t = cr.D_REF * p[0] * q[0] * p[1] * q[1] % R_MOD
        zz = (p[2] * q[2]) ** 2 % R_MOD
        assert p[2] % R_MOD and q[2] % R_MOD and t == (zz if w == "f" else -zz % R_MOD)


@pytest.mark.parametrize("op", list(cr.OPS))
def test_model_sets_are_inside_the_domain(op):
    edges = cr.edge_set(op)
    assert edges and len(set(edges)) == len(edges)
    out = [it for it in edges if not cr.in_domain(op, it)]
    assert not out, (op, out[:2])
    nrand = 72 if op == "fixed_chain" else 1024
    rnd_items = cr.random_set(op, random.Random(0xD0 + cr.OPS[op]), 1024)
    assert len(rnd_items) == nrand                                           # nothing rejected, nothing left out
    out = [it for it in rnd_items if not cr.in_domain(op, it)]
    assert not out, (op, out[:2])
    a, b = cr.records(op, edges)                                             # records round trip
    wa, wb, _, _ = cr.WIDTHS[op]
    assert a.dtype == np.uint32 and a.shape == (len(edges), wa) and (b is None) == (wb == 0)
    assert cr.items_of(op, a, b) == edges


def _pairs_of(op):
    """(affine P, affine Q after the op's negation) of every item of an addition op's edge set, from the inputs alone"""
    pn = op not in ("madd_t", "madd")
    out = set()
    for a, b in cr.edge_set(op):
        p = cr.ext_affine(a)
        if pn:
            X, Y, Z = cr.pniels_proj(b[:36], bool(b[36]))
            zi = cr.inv(Z)
            q = (X * zi % R_MOD, Y * zi % R_MOD)
        else:
            q = cr.niels_point(b[:27])
            q = cr.neg(q) if b[27] else q
        out.add((p, q, b[36 if pn else 27]))
    return out


@pytest.mark.parametrize("op", ["madd_t", "madd", "addpn_t", "addpn", "window"])
def test_model_addition_sets_hold_the_exceptional_pairs(op):
    """from the inputs alone: P + (-P), P + P and P + O for every edge point, and every ordered pair of edge points (the 64
    torsion pairs among them), each with the entry negated by the op and not"""
    pairs = _pairs_of(op)
    pts = cr.edge_points()
    for p in pts:
        for q in (cr.neg(p), p, (0, 1)):
            for negate in (0, 1):
                assert (p, q, negate) in pairs, (op, p, q, negate)
    for p in pts:
        for q in pts:
            assert (p, q, 0) in pairs or (p, q, 1) in pairs
            assert (p, cr.neg(q), 1) in pairs or (p, cr.neg(q), 0) in pairs
    if op == "window":
        assert {b[37] for _, b in cr.edge_set(op)} == {0, 1}
    # the negated entries are carry-less: 4r - t2d limb by limb reaches limbs of 30 bits
    neg_t2d = [tuple(c - x for c, x in zip(cr.fr.C4, b[18:27])) for _, b in cr.edge_set(op) if b[36 if op not in ("madd_t", "madd") else 27]]
    assert neg_t2d and max(max(t[:8]) for t in neg_t2d) >= 1 << 29 and min(min(t) for t in neg_t2d) >= 0


def test_model_sets_hold_the_extreme_representatives():
    """a coordinate at Montgomery representative 0, 1, r - 1 and 2r - 1 (and r) for each of X, Y, Z, T; every edge point in all
    of z = 1, z = r - 1 and all four coordinates at + r"""
    for op in ("madd_t", "addpn", "dbl_t", "dbl", "window", "to_pniels", "table", "mulw64", "mulw64_t"):
        seen = [set() for _ in range(4)]
        for it in cr.edge_set(op):
            for k, c in enumerate(cr.split(it[0], 4)):
                seen[k].add(cr.lval(c))
        for k in range(4):                                                   # Z is never zero: its representatives 0 and r do not exist
            assert ({1, R_MOD - 1, R_MOD + 1, 2 * R_MOD - 1} if k == 2 else {0, 1, R_MOD - 1, R_MOD, 2 * R_MOD - 1}) <= seen[k], (op, k)
    exts = {it[0] for it in cr.edge_set("dbl")}
    for p in cr.edge_points():
        for z in (1, R_MOD - 1):
            c = cr.ext_coords(p, z)
            assert sum((cr.reps(v)[0] for v in c), ()) in exts and sum((cr.reps(v)[1] for v in c), ()) in exts
    # entries: canonical and + r in every component, and ext_to_pniels of an all-(+ r) representation
    ents = {b[:36] for _, b in cr.edge_set("addpn")}
    for q in cr.edge_points():
        assert cr.pniels_reps(q, 1)[0] in ents and cr.pniels_reps(q, 1)[15] in ents
        c = cr.ext_coords(q, 1)
        assert cr.to_pniels_model(sum((cr.reps(v)[1] for v in c), ())) in ents
    nents = {b[:27] for _, b in cr.edge_set("madd")}
    for q in cr.edge_points():
        assert cr.niels_reps(q)[0] in nents and cr.niels_reps(q)[7] in nents


def test_model_ladder_scalars_reach_the_recoding_edges():
    """the signed digits of vb_mul_windowed are nibble + carry - 8 in [-8, 7]: table entry 8 is reached by -8 alone (+8 does not
    occur in this recoding), 7 is the largest positive digit; the sets hold both, a carry that runs through every window into
    window 63, and a single non-zero digit in the first, a middle and the two top windows"""
    sc = cr.edge_scalars()
    assert {0, 1, 2, 7, 8, 9, 15, 16, cr.SUBORDER - 1, cr.SUBORDER, cr.SUBORDER + 1, cr.ORDER - 1, (1 << 254) - 1} <= set(sc)
    assert all(0 <= s < 1 << 254 for s in sc)
    digs = {s: cr.recode(s) for s in sc}
    for s, d in digs.items():
        assert sum(v << (4 * j) for j, v in enumerate(d)) == s and all(-8 <= v <= 7 for v in d), s
    assert any(min(d) == -8 for d in digs.values()) and any(max(d) == 7 for d in digs.values())
    assert digs[cr.nibbles(8) % (1 << 254)] == [-8] + [-7] * 62 + [1]            # every window carries, the last into window 63
    assert digs[cr.nibbles(9) % (1 << 254)] == [-7] + [-6] * 62 + [2]
    assert digs[cr.nibbles(7) % (1 << 254)] == [7] * 63 + [3]                    # no carry anywhere
    for w in (0, 31, 62, 63):
        assert any(s and s >> (4 * w) << (4 * w) == s and s >> (4 * w) < 16 for s in sc), w
    used = {cr.fr.wval(it[1]) for it in cr.edge_set("mulw64")}
    assert set(sc) <= used
    assert {cr.fr.wval(it[1]) for it in cr.edge_set("mulw2")} == set(range(64)) and {cr.fr.wval(it[1]) for it in cr.edge_set("mulw1")} == set(range(4))


# ---- the shipped functions, built by g++, against the model --------------------------------------------------------------------
def _run(clibs, op, items, ref):
    a, b = cr.records(op, items)
    outs = []
    for layout in ((0, 1) if op in LAYOUT_OPS else (0,)):
        out = cr.cpu_run(clibs[layout], op, a, b)
        bad = cr.check(op, items, out, ref=ref, layout=layout)
        assert bad == [], (op, "layout %d" % layout, len(bad), [(items[i], why) for i, why in bad[:3]])
        outs.append(out)
    if len(outs) == 2 and op not in ("table", "table_affine"):
        # the packed and the raw per-lane tables give the same point (the packed ymx is weakly reduced: other limbs, same point)
        O0, O1 = cr._Rows(outs[0], 4), cr._Rows(outs[1], 4)
        for i in range(len(items)):
            assert cr.peq(O0.plain(i)[:3], O1.plain(i)[:3]), (op, items[i])
    return outs[0]


@pytest.mark.parametrize("op", list(cr.OPS))
def test_curve_op_edges_and_random(clibs, pyoracle, op):
    _run(clibs, op, cr.edge_set(op), pyoracle)
    _run(clibs, op, cr.random_set(op, random.Random(0xC0DE000 + cr.OPS[op]), N_RANDOM), pyoracle)


def test_reference_code_vanishing_denominators(clibs, pyoracle):
    """ref_add on the f = 0 and g = 0 operands: z3 is zero in value (limbs of a multiple of r), x3 and y3 are the oracle's, and
    affine() of them is (0, 0)"""
    items = [it for it in cr.edge_set("ref_add")
             if pyoracle.proj_add(tuple(cr.plain(c) for c in cr.split(it[0], 3)), tuple(cr.plain(c) for c in cr.split(it[1], 3)))[2] == 0]
    vp = {(p, q) for p, q, _ in cr.vanishing_pairs()}
    got = {(tuple(cr.plain(c) for c in cr.split(it[0], 3)), tuple(cr.plain(c) for c in cr.split(it[1], 3))) for it in items}
    assert vp <= got
    a, b = cr.records("ref_add", items)
    out = cr.cpu_run(clibs[0], "ref_add", a, b)
    assert cr.check("ref_add", items, out, ref=pyoracle) == []
    for row in out:
        assert cr.plain(tuple(int(v) for v in row[18:27])) == 0
        assert pyoracle.proj_affine(tuple(cr.plain(tuple(int(v) for v in row[9 * k:9 * k + 9])) for k in range(3))) == (0, 0)


def test_fixed_table_chain_equals_the_entry_definition(clibs):
    """the chain-built table equals fixed_table_entry limb for limb, for every chain length; fixed_table_check_slot counts
    nothing on it, and something for every flipped bit tried"""
    slots = [((s % 9, s // 9, 1 if s < 9 else 0),) for s in range(cr.FT_SLOTS)]
    a, _ = cr.records("fixed_entry", slots)
    entries = cr.cpu_run(clibs[0], "fixed_entry", a, None)
    assert cr.check("fixed_entry", slots, entries) == []
    chains = cr.edge_set("fixed_chain")
    a, _ = cr.records("fixed_chain", chains)
    out = cr.cpu_run(clibs[0], "fixed_chain", a, None).reshape(len(chains), cr.FT_SLOTS, 28)
    assert (out[:, :, :27] == entries[None, :, :]).all() and (out[:, :, 27] == 0).all()
    flips = cr.edge_set("fixed_flip")
    assert {(it[0][1], it[0][2]) for it in flips} == {(9 * j + s, w) for j in range(3) for s in (0, 4, 8) for w in range(27)}
    a, _ = cr.records("fixed_flip", flips)
    out = cr.cpu_run(clibs[0], "fixed_flip", a, None)
    assert (out[:, 0] > 0).all()
    # the slot before a flipped one sees a flipped y - x' or y + x' too (its link T[k] + P_j = T[k + 1] no longer closes); the
    # third word of an entry is judged at its own slot alone
    seen = np.array([it[0][1] % 9 != 0 and it[0][2] < 18 for it in flips])
    assert seen.any() and (out[seen, 1] > 0).all() and (out[~seen, 1] == 0).all()


def test_check_rejects_wrong_outputs(clibs):
    """the checker itself: one wrong bit, a T that is kept where none is asked for, the negated point, a limb out of form"""
    for op in ("madd_t", "addpn", "dbl", "window", "to_pniels", "pn2ext_t", "lift", "eq_niels", "nfa", "from_ref", "ref_add", "ref_mul2",
               "var_base", "table", "mulw2_t", "mulw64", "fixed_entry", "fixed_chain"):
        items = cr.edge_set(op)[:48]
        a, b = cr.records(op, items)
        out = cr.cpu_run(clibs[0], op, a, b)
        assert cr.check(op, items, out) == []
        wrong = out.copy()
        wrong[:, 0] ^= 1
        if op == "table":
            wrong = out.copy()
            wrong[:, 36 * 5] ^= 1                                            # entry 5, ymx
        assert len(cr.check(op, items, wrong)) == len(items), op
    items = cr.edge_set("dbl")[:48]                                          # T left behind where it is not asked for
    a, b = cr.records("dbl", items)
    out = cr.cpu_run(clibs[0], "dbl", a, b)
    out[:, 27] = 1
    assert len(cr.check("dbl", items, out)) == len(items)
    items = [it for it in cr.edge_set("madd_t") if cr.ext_affine(it[0])[0] != 0][:48]      # the other sign of x: another point
    a, b = cr.records("madd_t", items)
    out = cr.cpu_run(clibs[0], "madd_t", a, b)
    a2 = a.copy()
    a2[:, :9] = np.array([cr.nform(-cr.lval(tuple(int(v) for v in r)) % R_MOD) for r in a[:, :9]], dtype=np.uint32)
    a2[:, 27:36] = np.array([cr.nform(-cr.lval(tuple(int(v) for v in r)) % R_MOD) for r in a[:, 27:36]], dtype=np.uint32)
    other = cr.cpu_run(clibs[0], "madd_t", a2, b)
    nbad = len(cr.check("madd_t", items, other))
    assert nbad == len(items)                                                # -P + Q == P + Q only for 2 P == O, that is x == 0
    keep = out[:, 1] > 0                                                     # same value, a limb of 30 bits: not N-form
    out[keep, 0] += 1 << 29
    out[keep, 1] -= 1
    assert len(cr.check("madd_t", items, out)) == int(keep.sum()) > 0
