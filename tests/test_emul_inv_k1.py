"""fr_inv_k1 (babyjubjub-rs_amd/csrc/fr.hpp: the division-step inversion of K1's epilogue) on the CPU, built by
tests/emul/emul_inv_k1.cpp with BJJ_DEBUG_BOUNDS -- the growth bound of (d, e), the exactness of every division by 2^29 and
g == 0 after the 21 batches are asserted on every call -- against fr_inv_fermat AND fr_inv_gcd, byte for byte after fr_canon,
and against Python integers.  Inputs are raw representatives below 2r, as K1's epilogue hands them over.
What this harness compiles is the portable `#else` branch of the limb products.  The branch the device build takes -- the
eight v_mad_i64_i32 of a limb as one inline-asm statement -- never runs here: it is covered on the GPU, on the same directed
set (tests/divstep_ref.py), by tests/test_gpu_devfuzz.py::test_k1_inversion_core_on_device and ::test_block_invert_directed_lanes."""
import ctypes
import os

import pytest

import divstep_ref as ds
import hostbuild
from conftest import ROOT, le32

Q = 21888242871839275222246405745257275088548364400416034343698204186575808495617   # r
R = 1 << 261


@pytest.fixture(scope="module")
def invlib():
    lib = ctypes.CDLL(hostbuild.shared("libbjj_emul_inv_k1.so", os.path.join(ROOT, "tests", "emul", "emul_inv_k1.cpp"), extra=("-pthread",)))
    lib.emul_inv_k1_splitmix.restype = ctypes.c_long
    lib.emul_inv_k1_splitmix.argtypes = [ctypes.c_ulonglong, ctypes.c_long, ctypes.c_char_p]
    return lib


def _check(lib, xs):
    out = ctypes.create_string_buffer(32)
    for x in xs:
        assert 0 <= x < 2 * Q
        assert lib.emul_inv_k1_one(le32(x), out) == 1, "the three cores disagree on %#x" % x
        # X = x R  ->  R / x = R^2 / X; 0 (and r) -> 0
        want = R * R * pow(x, Q - 2, Q) % Q
        assert int.from_bytes(out.raw, "little") == want, hex(x)


def test_edges(invlib):
    _check(invlib, [0, 1, 2, Q - 1, Q, Q + 1, 2 * Q - 1, R % Q, R * R % Q])


def test_powers_of_two(invlib):
    _check(invlib, [1 << k for k in range(255)] + [(1 << k) - 1 for k in range(255)])   # 2^254 < 2r < 2^255


def test_short_operands(invlib):
    """top limbs zero: 60, 90 and 120 significant bits"""
    xs = []
    for bits in (60, 90, 120):
        xs += [(1 << bits) - 1, 1 << (bits - 1), (1 << (bits - 1)) + 1,
               (0x9e3779b97f4a7c15f39cc0605cedc835 * (bits + 1)) % (1 << bits) | (1 << (bits - 1)),
               (0xc2b2ae3d27d4eb4f165667b19e3779f9 * (bits + 3)) % (1 << bits) | (1 << (bits - 1)) | 1]
    _check(invlib, xs)


def test_splitmix_values(invlib):
    """10^5 SplitMix64 values below 2r, compared inside the harness (8 streams on 8 threads)"""
    first_bad = ctypes.create_string_buffer(32)
    bad = invlib.emul_inv_k1_splitmix(0x6b315f696e76, 100000, first_bad)
    assert bad == 0, "first disagreement at %#x" % int.from_bytes(first_bad.raw, "little")


def test_division_step_model_on_the_directed_set():
    """the plain-integer model of the division steps (tests/divstep_ref.py) on the directed set the GPU tests use: g reaches 0
    within the 21 x 29 = 609 steps and sign(f) * d is R^2 / y.  The set's own coverage is asserted too, as a property of the
    inputs: at least 100 operands end with f = -1 (the two's-complement negation of d at the end of fr_inv_k1) and at least 100
    with f = +1."""
    ends = {1: 0, -1: 0}
    for y in ds.directed_operands():
        sign, zero_at, d = ds.divsteps(y)
        assert zero_at is not None and zero_at <= 609, hex(y)
        assert sign * d % Q == ds.want_inverse(y) == (0 if y % Q == 0 else R * R * pow(y, -1, Q) % Q), hex(y)
        ends[sign] += 1
    assert ends[1] >= 100 and ends[-1] >= 100, ends


def test_directed_set(invlib):
    """the directed set of the GPU tests through the portable branch, with the bound assertions on"""
    _check(invlib, ds.directed_operands())
