"""Plain-integer model of fr_inv_k1's division steps (babyjubjub-rs_amd/csrc/fr.hpp) and the directed operand set of its
tests.  Test infrastructure: used by tests/test_emul_inv_k1.py (CPU) and tests/test_gpu_devfuzz.py (GPU).  The model says which
end state an operand drives the function into (f = +1 or f = -1, the latter takes the two's-complement negation of d) and
how many steps it needs, so that a test can prove its own coverage from its inputs alone."""
import functools
import random

R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
RADIX = 1 << 261
K = RADIX * RADIX % R_MOD       # d*y == f*K, e*y == g*K (mod r)
HALF = (R_MOD + 1) // 2         # 1/2 mod r
BATCHES, STEPS = 21, 29


@functools.lru_cache(maxsize=None)
def divsteps(y):
    """21 batches x 29 steps of the half-delta divstep on (f, g) = (r, y mod r), zeta = -(delta + 1/2) starting at -1.
    Returns (sign of the final f, the number of steps after which g was 0 for the first time (None: never), d mod r).
    (d, e) are kept modulo r; the kernel keeps unreduced signed multiples and divides by 2^29 once per batch."""
    f, g, d, e, zeta, zero_at = R_MOD, y % R_MOD, 0, K, -1, None
    for step in range(BATCHES * STEPS):
        if g == 0 and zero_at is None:
            zero_at = step
        if g & 1:
            if zeta < 0:                                   # delta > 0: swap and subtract
                f, g, d, e, zeta = g, g - f, e, e - d, -zeta - 2
            else:
                g, e, zeta = g + f, e + d, zeta - 1
        else:
            zeta -= 1
        assert g & 1 == 0
        g, e = g >> 1, e * HALF % R_MOD
    if g == 0 and zero_at is None:
        zero_at = BATCHES * STEPS
    return (1 if f > 0 else -1), zero_at, d % R_MOD


def want_inverse(v):
    """what every inversion core returns for the raw operand v: R^2 / v mod r, canonical; 0 (and r) -> 0"""
    return 0 if v % R_MOD == 0 else K * pow(v, -1, R_MOD) % R_MOD


# operands the directed set keeps by name: none has failed so far
NAMED = {}


@functools.lru_cache(maxsize=None)
def directed_operands(seeded=3000):
    """raw values below 2r, as block_invert hands them to the inversion core.  Tuple, in a fixed order."""
    r = R_MOD
    base = [0, 1, 2, r - 1, r, r + 1, 2 * r - 1, RADIX % r, K]
    base += [1 << k for k in range(1, 255)] + [(1 << k) - 1 for k in range(1, 255)]
    ops = list(base) + [v + r for v in base if v < r]      # the [r, 2r) representative that fr_cond_sub_kr must fold
    rnd = random.Random(0x6b31646976)
    for bits in (29, 58, 60, 90, 120):                     # short operands (upper limbs zero): top bit set / low bit set too
        top = 1 << (bits - 1)
        ops += [top, top | 1, (1 << bits) - 1, top | rnd.getrandbits(bits - 1), top | rnd.getrandbits(bits - 1) | 1]
    for low in (29, 58):                                   # low limb(s) zero: 29 / 58 leading "g even" steps, a pure-shift batch
        ops += [r - (r % (1 << low))] + [(rnd.randrange(1 << low, 2 * r) >> low) << low for _ in range(8)]
    ops += [rnd.randrange(2 * r) for _ in range(seeded)]
    ops += list(NAMED.values())
    assert all(0 <= v < 2 * r for v in ops)
    return tuple(ops)
