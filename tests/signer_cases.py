"""Inputs shared by the signer-verification tests (tests/test_signer_host.py on the CPU, tests/test_gpu_signer.py on the GPU); holds
no tests.  Everything is built with the C oracle's batch functions (an `Oracle` of conftest.py), as workload.make_signatures does,
but under ONE key:  A = k*B8 (+ a torsion point),  R_i = rho_i*B8,  S_i = rho_i + 8*hm_i*k mod l  (Schnorr: S_i = rho_i + h_i*k mod l).

A key with a torsion component has order 8l.  EdDSA multiplies the hash by 8, which kills the torsion, so every such signature is
valid.  Schnorr does not: s*B8 == R + h*A needs h*T8 == O, i.e. h = 0 (mod 8), so the nonces are searched (seeded, in rounds) until
every item's hash is a multiple of 8 -- valid signatures exist for such a key, they are just 8 times rarer."""
import numpy as np

from conftest import pack, unpack

Q = 21888242871839275222246405745257275088548364400416034343698204186575808495617
L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
B8 = (5299619240641551281634865583518297030282874472190772894086521144482721001553,
      16950150798460657717958625567821834550301663161624707787222815936182638968203)
KEY_SCALAR = 0x1d5a3c4b7e6f8091a2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f7081 % L


def rec(vals, width=32):
    """ints (or tuples of ints) -> (n, width) uint8 records"""
    return pack(vals).reshape(-1, width)


def key_point(oracle, k, torsion=None):
    """k*B8, plus `torsion` (a point) when given -> (x, y)"""
    a = oracle.mul_fixed_base(rec([k]))
    if torsion is not None:
        a = oracle.point_add(a, rec([tuple(torsion)], 64))
    return unpack(a, 2)[0]


def _rand_ints(rng, n, below):
    return [int.from_bytes(rng.integers(0, 256, 40, dtype=np.uint8).tobytes(), "little") % below for _ in range(n)]


def sign_items(oracle, A, k, msgs, seed, schnorr, need_h_mod8=False):
    """valid signatures of the key (A, k) over msgs (ints < Q): -> R (n, 64), S (n, 32) uint8"""
    rng = np.random.default_rng(seed)
    n = len(msgs)
    M = rec([m % Q for m in msgs])
    Arec = np.tile(rec([A], 64), (n, 1))
    rho, R, h = [0] * n, np.zeros((n, 64), np.uint8), [0] * n
    todo = list(range(n))
    for _ in range(400):
        if not todo:
            break
        cand = _rand_ints(rng, len(todo), L)
        Rc = oracle.mul_fixed_base(rec(cand))
        parts = [Arec[todo], Rc, M[todo]] if schnorr else [Rc, Arec[todo], M[todo]]
        hc = unpack(oracle.poseidon5(np.concatenate(parts, axis=1)))
        left = []
        for j, i in enumerate(todo):
            if need_h_mod8 and hc[j] % 8:
                left.append(i)
                continue
            rho[i], R[i], h[i] = cand[j], Rc[j], hc[j]
        todo = left
    assert not todo, "the nonce search did not finish"
    S = [(rho[i] + (h[i] if schnorr else 8 * h[i]) * k) % L for i in range(n)]
    return R, rec(S)


def bulk(oracle, A, k, n, seed, schnorr, torsion_key):
    """n signatures under one key, 1 in 8 with one seeded bit flipped in S, msg or R.y (an R.y flip puts R off the curve)
    -> R, S, msg"""
    rng = np.random.default_rng(seed ^ 0x51617)
    msgs = _rand_ints(rng, n, 1 << 253)
    R, S = sign_items(oracle, A, k, msgs, seed, schnorr, need_h_mod8=schnorr and torsion_key)
    M = rec(msgs)
    pick = rng.integers(0, 8, n)
    which = rng.integers(0, 3, n)
    bit = rng.integers(0, 250, n)
    for i in np.nonzero(pick == 0)[0]:
        arr, col0 = ((S, 0), (M, 0), (R, 32))[which[i]]
        arr[i, col0 + bit[i] // 8] ^= np.uint8(1 << (bit[i] % 8))
    return R, S, M


DIRECTED = ("valid", "valid2", "s+l", "s=2^256-1", "msg=Q", "msg=Q+1", "flip s", "flip msg", "flip R.x", "flip R.y",
            "R=identity", "R=(0,0)", "R=order 2", "R.x+r")


def directed(oracle, A, k, seed, schnorr, torsion_key):
    """the directed items, in the order of DIRECTED -> R (n, 64), S (n, 32), msg (n, 32)"""
    n = len(DIRECTED)
    rng = np.random.default_rng(seed ^ 0xD1EC7)
    msgs = _rand_ints(rng, n, 1 << 253)
    msgs[DIRECTED.index("msg=Q")] = 0                      # signed as 0, presented as Q: the reference wraps Q to 0
    R, S = sign_items(oracle, A, k, msgs, seed, schnorr, need_h_mod8=schnorr and torsion_key)
    Rv, Sv = [list(p) for p in unpack(R, 2)], unpack(S)
    i = DIRECTED.index
    Sv[i("s+l")] += L
    Sv[i("s=2^256-1")] = (1 << 256) - 1
    msgs[i("msg=Q")] = Q
    msgs[i("msg=Q+1")] = Q + 1
    Sv[i("flip s")] ^= 1 << 77
    msgs[i("flip msg")] ^= 1 << 5
    Rv[i("flip R.x")][0] ^= 1 << 100
    Rv[i("flip R.y")][1] ^= 1 << 3
    Rv[i("R=identity")] = [0, 1]
    Rv[i("R=(0,0)")] = [0, 0]
    Rv[i("R=order 2")] = [0, Q - 1]
    Rv[i("R.x+r")][0] += Q                                 # < 2^256: the record is reduced mod r, the signature stays valid
    return rec([tuple(p) for p in Rv], 64), rec(Sv), rec(msgs)
