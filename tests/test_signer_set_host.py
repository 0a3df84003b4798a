"""bjj_eddsa_verify_set / bjj_schnorr_verify_set without a GPU: the per-item body of csrc/signer_set.hpp -- what k_signer_set.hip
launches -- run on the CPU by the stand-alone program tests/signer_set_emul (bound assertions on, and a gather that refuses a slot
outside its table), over sets of k = 3 keys at W = 4 and W = 5 laid out in one allocation and built thread by thread with the
bodies of the set's build kernels, and a context's B8 table at W = 4.  Every verdict is the pure-Python oracle's verify /
verify_schnorr for the key the item's index names; an index that is not one of the set gives 3.  The same program runs once more
built with -fsanitize=address,undefined, directly (no preload)."""
import os

import numpy as np
import pytest

import hostbuild
import signer_cases as sc
from conftest import ROOT, ints, unpack

Q = sc.Q
SRC = os.path.join(ROOT, "tests", "signer_set_emul", "signer_set_emul.cpp")
K = 3
BAD_SIGNER = 3


@pytest.fixture(scope="module")
def inputs(oracle, pyoracle, golden):
    """the program's stdin and the expected verdicts -- computed once.  Keys: ordinary, of order 8l, ordinary with x + r in its
    record.  Items: the directed ones under keys 0 (both schemes) and 1 (EdDSA), a few signed ones under every key, four of them
    presented under another signer's index, and three whose index is not one of the set, one of these with msg > Q as well."""
    o = pyoracle
    tors = [ints(t) for t in golden["gpu_expected"]["torsion_points"]]
    scalars = [sc.KEY_SCALAR, sc.KEY_SCALAR + 12345, sc.KEY_SCALAR + 999]
    torsion = [None, tors[1], None]
    keys = [sc.key_point(oracle, scalars[j], torsion[j]) for j in range(K)]
    assert all(o.on_curve(A) for A in keys)
    records = [keys[0], keys[1], (keys[2][0] + Q, keys[2][1])]
    idx, parts = [], []

    def add(j, triple):
        parts.append(triple)
        idx.extend([j] * len(triple[1]))
    add(0, sc.directed(oracle, keys[0], scalars[0], 0x5E70, False, False))
    add(0, sc.directed(oracle, keys[0], scalars[0], 0x5E71, True, False))
    add(1, sc.directed(oracle, keys[1], scalars[1], 0x5E72, False, True))
    for j in range(K):
        for schnorr in (False, True):
            add(j, sc.bulk(oracle, keys[j], scalars[j], 4, 0x5E80 + 2 * j + schnorr, schnorr, torsion[j] is not None))
    R, S, M = (np.concatenate([p[c] for p in parts]) for c in range(3))
    n = len(idx)
    first_bulk = 3 * len(sc.DIRECTED)
    for i in range(first_bulk, n, 6):                      # a valid signature under the wrong key
        idx[i] = (idx[i] + 1) % K
    out_of_range = {first_bulk + 1: K, first_bulk + 8: K + 1, n - 1: (1 << 32) - 1}
    for i, v in out_of_range.items():
        idx[i] = v
    perm = np.random.default_rng(0x5E7).permutation(n)
    idx = [idx[i] for i in perm]
    Rv, Sv, Mv = ([unpack(a, w)[i] for i in perm] for a, w in ((R, 2), (S, 1), (M, 1)))
    assert {0, K - 1} <= set(idx) and sum(i >= K for i in idx) == 3
    both = idx.index(K + 1)                                # one of them also carries msg > Q: the index is looked at first
    Mv[both] = Q + 7
    assert o.verify_schnorr(keys[0], Mv[both], Rv[both], Sv[both]) is None and not o.verify(keys[0], Rv[both], Sv[both], Mv[both])
    text = "K %d\n%s\nI %d\n%s\n" % (K, "\n".join("%x %x" % p for p in records), n,
                                     "\n".join("%x %x %x %x %x" % (idx[i], Rv[i][0], Rv[i][1], Sv[i], Mv[i]) for i in range(n)))
    ed, sn = [], []
    for i in range(n):
        if idx[i] >= K:
            ed.append(BAD_SIGNER)
            sn.append(BAD_SIGNER)
            continue
        A = keys[idx[i]]                                   # the record reduced mod r
        ed.append(int(o.verify(A, Rv[i], Sv[i], Mv[i])))
        sn.append({None: 2, False: 0, True: 1}[o.verify_schnorr(A, Mv[i], Rv[i], Sv[i])])
    # the inputs are what they claim to be: both verdicts occur under every key, and the wrong-signer items are refused
    for j in range(K):
        assert {ed[i] for i in range(n) if idx[i] == j} == {0, 1}, j
    assert set(ed) == {0, 1, 3} and set(sn) == {0, 1, 2, 3}
    assert ed[both] == BAD_SIGNER and sn[both] == BAD_SIGNER
    return {"text": text, "n": n, "eddsa": ed, "schnorr": sn}


def _check_output(out, inp):
    facts = {"check": [], "tform": [], "e": {}, "s": {}}
    for line in out.split("\n"):
        f = line.split()
        if not f:
            continue
        if f[0] == "check":
            facts["check"].append((int(f[1]), int(f[2])))
        elif f[0] == "tform":
            facts["tform"].append((int(f[1]), int(f[2]), int(f[3])))
        elif f[0] in ("e", "s"):
            facts[f[0]].setdefault(int(f[1]), []).append((int(f[2]), int(f[3])))
    assert facts["check"] == [(0, 0), (1, 0), (2, 0)]
    assert facts["tform"] == [(W, s, 1) for W in (4, 5) for s in range(K)]      # window 0 of EVERY signer is in T form
    for W in (4, 5):
        for kind, want in (("e", inp["eddsa"]), ("s", inp["schnorr"])):
            got = facts[kind][W]
            assert [i for i, _ in got] == list(range(inp["n"]))
            bad = [(i, v, want[i]) for i, v in got if v != want[i]]
            assert not bad, (kind, W, bad)


def test_verdicts_match_the_python_oracle(inputs):
    _check_output(hostbuild.run(hostbuild.program("signer_set_emul", SRC), inputs["text"]), inputs)


def test_the_same_program_under_asan_and_ubsan(inputs):
    hostbuild.need_sanitizer_runtimes()          # BEFORE the build: a build that fails is a failure
    _check_output(hostbuild.run_sanitized(hostbuild.program("signer_set_emul_san", SRC, san=True), inputs["text"]), inputs)
