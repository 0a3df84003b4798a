"""The Poseidon permutation as field elements on the CPU (csrc/poseidon.hpp: poseidon5_t with its partial rounds one at a time and in
pairs, poseidon_full_round; csrc/dleq.hpp: dleq_challenge in both forms): the dispatcher of tests/devfuzz/hash_ops.hpp built by g++
with the bound assertions live (tests/emul/emul_hash_ops.cpp), on the directed edge sets of tests/hash_ref.py plus 2^12 seeded
random items per op.  The edge sets hold what a valid signature or proof can never put into the hash: the representatives 0, r,
r +- 1, 2r - 2, 2r - 1, Montgomery one and minus one in both representatives, single bits at every limb boundary, all-ones limbs
under the top limbs 0, top(r) - 1, top(r) and the largest one below 2r, and the two representatives of the input that makes an
S-box input zero -- each in every position.  The edges are judged by the plain 68-round model, which this module first holds
against oracle/bjj_oracle.py; the random items by the threaded C oracle.  tests/test_gpu_hash_ops.py runs the same sets on the device.

The library is built with BJJ_DEBUG_BOUNDS (the `hlib` fixture asserts that BJJ_ASSERT is live in it), so a lazily growing state
element that leaves its bound fails fr_dot3's operand and sum check, fr_dot2_add's BJJ_ASSERT or an operand check of fr_mul: the
whole pytest process aborts (exit status 134) with the assertion's file and line.  That abort is the expected form of failure for a
broken bound; every other error is an ordinary failing assertion."""
import ctypes
import os
import random

import numpy as np
import pytest

import hash_ref as hr
import hostbuild
from conftest import ROOT
from field_ref import R1, R_MOD, mont

N_RANDOM = 1 << 12
P5_OPS = ("p5_plain", "p5_pairs")
CHALLENGE_OPS = ("challenge_plain", "challenge_pairs")


@pytest.fixture(scope="module")
def hlib():
    """the dispatcher of tests/devfuzz/hash_ops.hpp built for the CPU, bound assertions live"""
    lib = ctypes.CDLL(hostbuild.shared("libbjj_emul_hash_ops.so", os.path.join(ROOT, "tests", "emul", "emul_hash_ops.cpp")))
    for op, code in hr.OPS.items():
        assert tuple(lib.emul_hash_words(code, k) for k in range(2)) == hr.WIDTHS[op], op
    assert lib.emul_hash_bounds_live() == 1          # an assert inside BJJ_ASSERT ran: BJJ_DEBUG_BOUNDS is set and NDEBUG is not
    return lib


# the edges every set must contain, written out here (not taken from hash_ref.edge_values)
NAMED_EDGES = ([0, 1, R_MOD - 1, R_MOD, R_MOD + 1, 2 * R_MOD - 2, 2 * R_MOD - 1, R1, R1 + R_MOD, mont(R_MOD - 1), mont(R_MOD - 1) + R_MOD]
               + [1 << (29 * i) for i in range(9)]
               + [((t + 1) << 232) - 1 for t in (0, 3171405, 3171406, ((2 * R_MOD) >> 232) - 1)])


# ---- the model against the oracle and against itself ------------------------------------------------------------------------
def test_model_is_the_python_oracles_permutation(pyoracle):
    C, M, rp = pyoracle.poseidon_params(6)
    assert rp == 60 and hr.C_PLAIN == list(C) and hr.M_PLAIN == [list(row) for row in M]
    # the full rounds' constants as the kernels add them: the oracle's for the rounds 0-3 and 65-67 (round 64's are adjusted for
    # the sparse form before it; the whole-hash ops are what holds those against the oracle)
    for k, r in ((0, 0), (1, 1), (2, 2), (3, 3), (5, 65), (6, 66), (7, 67)):
        assert hr.PCF[6 * k:6 * k + 6] == [mont(c) for c in C[6 * r:6 * r + 6]], k
    rows = [tuple(hr.plain(v) for v in row) for row in hr.p5_edge_rows()[::3]]
    assert len(rows) > 40 and [hr.poseidon5(row) for row in rows] == [pyoracle.poseidon(list(row)) for row in rows]
    # a full round of the model is a round of the oracle's permutation: four of them from [0, in] give the state the hash continues from
    st = [0] + list(rows[7])
    for r in range(4):
        st = hr.full_round(st, r)
    want = [0] + list(rows[7])
    for r in range(4):
        want = [pow((s + c) % R_MOD, 5, R_MOD) for s, c in zip(want, C[6 * r:6 * r + 6])]
        want = [sum(M[i][j] * want[j] for j in range(6)) % R_MOD for i in range(6)]
    assert st == want


@pytest.mark.parametrize("op", list(hr.OPS))
def test_model_sets_are_inside_the_domain(op):
    edges = hr.edge_set(op)
    assert edges and len(set(edges)) == len(edges)
    out = [it for it in edges if not hr.in_domain(op, it)]
    assert not out, (op, out[:2])
    rnd_items = hr.random_set(op, random.Random(0xD0 + hr.OPS[op]), 2048)
    assert len(rnd_items) == 2048                                          # nothing rejected, nothing left out
    out = [it for it in rnd_items if not hr.in_domain(op, it)]
    assert not out, (op, out[:2])
    recs = hr.records(op, edges)                                           # records round trip, and every element in N-form
    assert recs.dtype == np.uint32 and recs.shape == (len(edges), hr.WIDTHS[op][0])
    assert hr.items_of(op, recs) == edges
    limbs = recs[:, :hr.NELEMS[op] * 9].reshape(-1, 9)
    assert (limbs[:, :8] < 1 << 29).all() and (limbs[:, 8] <= hr.TOP_2R).all()


def test_model_edge_sets_hold_the_directed_edges():
    assert len(set(NAMED_EDGES)) == 23 and all(0 <= v < 2 * R_MOD for v in NAMED_EDGES)       # 2^0 is the value 1: 24 names, 23 values
    assert set(hr.edge_values()) == set(NAMED_EDGES)
    # the hashes: every named edge in each of the five positions and in all five at once; the others random, half of them canonical
    rows = hr.p5_edge_rows()
    for v in NAMED_EDGES:
        assert (v,) * 5 in rows
        for p in range(5):
            assert any(row[p] == v and row != (v,) * 5 for row in rows), (v, p)
    others = [x for row in rows[:23 * 5] for x in row if x not in NAMED_EDGES]
    assert 0.4 < sum(1 for x in others if x < R_MOD) / len(others) < 0.6
    # ... and for position j both representatives of the input that makes S-box input j + 1 of the first round zero
    for j in range(5):
        lo, hi = R_MOD - hr.PCF[j + 1], 2 * R_MOD - hr.PCF[j + 1]
        assert 0 < lo < R_MOD < hi < 2 * R_MOD and (lo + hr.PCF[j + 1]) % R_MOD == 0
        assert any(row[j] == lo for row in rows) and any(row[j] == hi for row in rows), j
    assert tuple(R_MOD - hr.PCF[j + 1] for j in range(5)) in rows and tuple(2 * R_MOD - hr.PCF[j + 1] for j in range(5)) in rows
    # the full round: every round index with every named edge in each of the six positions and in all six, and the states that
    # make S-box input j a representative of zero in that round
    rows = hr.full_round_edge_rows()
    for r in range(8):
        mine = [row[:6] for row in rows if row[6] == r]
        at = [set(row[p] for row in mine) for p in range(6)]
        for v in NAMED_EDGES:
            assert (v,) * 6 in mine and all(v in at[p] for p in range(6)), (r, v)
        for j in range(6):
            assert {R_MOD - hr.PCF[6 * r + j], 2 * R_MOD - hr.PCF[6 * r + j]} <= at[j], (r, j)
        assert tuple(R_MOD - hr.PCF[6 * r + j] for j in range(6)) in mine and tuple(2 * R_MOD - hr.PCF[6 * r + j] for j in range(6)) in mine
    # the challenges: the tag at every named edge
    rows = hr.challenge_edge_rows()
    assert set(NAMED_EDGES) <= {row[0] for row in rows if len(set(row)) > 1}
    assert all((v,) * 9 in rows for v in NAMED_EDGES)


# ---- the shipped functions, built by g++, against the model and the C oracle ---------------------------------------------------
@pytest.mark.parametrize("op", list(hr.OPS))
def test_hash_op_edges_and_random(hlib, oracle, op):
    edges = hr.edge_set(op)
    want = hr.expected(op, edges)
    if op != "full_round":
        assert hr.expected_c(op, edges, oracle) == want                    # the model and the C oracle agree on the edges
    got_e = hr.cpu_run(hlib, op, hr.records(op, edges))
    bad = hr.check(op, edges, got_e, want)
    assert bad == [], (op, "edges", len(bad), [(edges[i], why) for i, why in bad[:3]])
    items = hr.random_set(op, random.Random(0x4A5E000 + hr.OPS[op]), N_RANDOM)
    got_r = hr.cpu_run(hlib, op, hr.records(op, items))
    bad = hr.check(op, items, got_r, None if op == "full_round" else hr.expected_c(op, items, oracle))
    assert bad == [], (op, "random", len(bad), [(items[i], why) for i, why in bad[:3]])
    if op not in CHALLENGE_OPS:
        k = 9 if op in P5_OPS else 54
        print("[hash ops, CPU] %-15s largest output %.4f r" % (op, hr.largest_over_r(np.concatenate([got_e[:, :k], got_r[:, :k]]))))


@pytest.mark.parametrize("ops", [P5_OPS, CHALLENGE_OPS])
def test_the_two_forms_give_the_same_canonical_words(hlib, ops):
    items = hr.edge_set(ops[0]) + hr.random_set(ops[0], random.Random(0x4A5E100), 1024)
    recs = hr.records(ops[0], items)
    a, b = hr.cpu_run(hlib, ops[0], recs), hr.cpu_run(hlib, ops[1], recs)
    assert (a[:, -8:] == b[:, -8:]).all()
    if ops is P5_OPS:
        print("[hash ops, CPU] representatives differ on %d of %d items" % (int((a[:, :9] != b[:, :9]).any(axis=1).sum()), len(items)))


def test_check_rejects_wrong_outputs(hlib):
    """the checker itself: one flipped output bit, wherever it is, and a canonical part that is off by r are reported for every item"""
    for op in hr.OPS:
        items = hr.edge_set(op)[:64]
        if op == "full_round":
            items = items[:56] + [it for it in hr.edge_set(op) if it[6] == 7][:8]
        out = hr.cpu_run(hlib, op, hr.records(op, items))
        want = hr.expected(op, items)
        assert hr.check(op, items, out, want) == []
        for word, bit in ((0, 0), (3, 28), (hr.WIDTHS[op][1] - 1, 0), (hr.WIDTHS[op][1] - 1, 20)):
            wrong = out.copy()
            wrong[:, word] ^= np.uint32(1 << bit)
            assert len(hr.check(op, items, wrong, want)) == len(items), (op, word, bit)
        if op in P5_OPS:
            wrong = out.copy()                                                # the right value plus r in the 8 canonical words
            wrong[:, 9:] = np.ascontiguousarray(hr._le32([w + R_MOD for w in want])).view("<u4").reshape(-1, 8)
            assert len(hr.check(op, items, wrong, want)) == len(items), op
            wrong = out.copy()                                                # the raw limbs of the value plus 2r: not below 2r
            wrong[:, :9] = hr.limbs_of_vals([v + 2 * R_MOD for v in hr.vals_of_limbs(out[:, :9])])
            assert len(hr.check(op, items, wrong, want)) == len(items), op
    # the six-lane record: eight identical lanes pass, one differing lane or a wrong value on all of them does not
    items = hr.edge_set("p5_plain")[:64]
    out = hr.cpu_run(hlib, "p5_plain", hr.records("p5_plain", items))
    want = hr.expected("p5_plain", items)
    six = np.tile(out[:, :9], (1, 8))
    assert hr.check_six_lane(items, six, want) == []
    for lane in range(8):
        wrong = six.copy()
        wrong[:, 9 * lane + 4] ^= 1
        assert len(hr.check_six_lane(items, wrong, want)) == len(items), lane
    wrong = np.tile(out[:, :9] ^ np.array([1] + [0] * 8, np.uint32), (1, 8))
    assert len(hr.check_six_lane(items, wrong, want)) == len(items)
    other = np.tile(hr.limbs_of_vals([v + R_MOD for v in hr.vals_of_limbs(out[:, :9])]), (1, 8))     # another representative is fine here
    assert hr.check_six_lane(items, other, want) == []
