"""The product's field arithmetic (babyjubjub-rs_amd/csrc/fr.hpp: 9 x 29-bit limbs, Montgomery
radix 2^261, lazy reduction, binary-GCD inversion) executed on the CPU by the debug harness
tests/emul/emul_fr.cpp with limb/column/value-bound assertions on, against Python integers."""
import ctypes
import os
import random

import pytest

import hostbuild
from conftest import ROOT, le32

Q = 21888242871839275222246405745257275088548364400416034343698204186575808495617


@pytest.fixture(scope="module")
def frlib():
    return ctypes.CDLL(hostbuild.shared("libbjj_emul_fr.so", os.path.join(ROOT, "tests", "emul", "emul_fr.cpp"), opt="-O1"))

def _vals(rnd, n):
    edge = [0, 1, 2, Q - 1, Q - 2, (1 << 256) - 1, Q, Q + 1, 1 << 255, (1 << 29) - 1, 1 << 29, (1 << 232) - 1]
    return edge + [rnd.randrange(1 << 256) for _ in range(n)]


def test_field_ops(frlib):
    rnd = random.Random(7)
    vals = _vals(rnd, 200)
    out = ctypes.create_string_buffer(32)
    g = lambda: int.from_bytes(out.raw, "little")  # noqa: E731
    for x in vals:
        frlib.emul_words_roundtrip(le32(x), out)
        assert g() == x
    for _ in range(1500):
        x, y, z = rnd.choice(vals), rnd.choice(vals), rnd.choice(vals)
        frlib.emul_fr_mul(le32(x), le32(y), out); assert g() == x * y % Q
        frlib.emul_fr_sqr(le32(x), out); assert g() == x * x % Q
        frlib.emul_fr_add(le32(x), le32(y), out); assert g() == (x + y) % Q
        frlib.emul_fr_sub(le32(x), le32(y), out); assert g() == (x - y) % Q
        frlib.emul_fr_sub8(le32(x), le32(y), out); assert g() == (x - y) % Q
        frlib.emul_fr_chain(le32(x), le32(y), le32(z), out); assert g() == ((x * y - z) - (x + y)) * x % Q
        assert frlib.emul_fr_eq(le32(x), le32(y)) == (x % Q == y % Q)


def test_inversions_agree(frlib):
    """binary-GCD inversion (used by the kernels) == Fermat == pow(x, -1, r); 0 -> 0"""
    rnd = random.Random(9)
    R = 1 << 261
    vals = [0, 1, 2, 3, Q - 1, (Q + 1) // 2] + [rnd.randrange(Q) for _ in range(1500)] + \
           [rnd.randrange(1 << k) for k in range(1, 254)] + \
           [pow(R, -1, Q) * t % Q for t in (1, 2, 3, 1 << 29, (1 << 58) - 1, 1 << 59, 1 << 60, (1 << 60) - 1, (1 << 61) + 5)]
    out = ctypes.create_string_buffer(32)
    for i, x in enumerate(vals):
        want = pow(x, Q - 2, Q)
        frlib.emul_fr_inv_gcd(le32(x), out)
        assert int.from_bytes(out.raw, "little") == want, hex(x)
        if i % 16 == 0:
            frlib.emul_fr_inv(le32(x), out)
            assert int.from_bytes(out.raw, "little") == want
            y = rnd.randrange(Q)
            frlib.emul_fr_inv_gcd_lazy(le32(x), le32(y), out)  # un-normalised (lazy) input
            assert int.from_bytes(out.raw, "little") == want
