"""Inputs shared by the bjj_mul_bases tests (tests/test_bases_host.py on the CPU, tests/test_gpu_bases.py on the GPU); holds no tests.

Directed scalars: the values around the two reductions (mod l for the context's B8 table, mod 8l for a caller's table) and,
per window width W, the two digit patterns that stress the signed recoding -- every window 2^(W-1), the largest non-negative
digit (no carry anywhere), and every window 2^(W-1) + 1, where every digit is negative and the carry runs through all windows
into the top one.  A pattern is cut at the top until it is below 8l, so that the reduction leaves its digits as they are."""
import numpy as np

L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
ORDER8 = 8 * L
FIXED = [0, 1, L - 1, L, L + 1, ORDER8 - 1, ORDER8, ORDER8 + 1, (1 << 254) - 1, (1 << 256) - 1]


def base_windows(W):
    return -(-255 // W)


def pattern(W, digit):
    nwin = base_windows(W)
    while True:
        v = sum(digit << (W * j) for j in range(nwin))
        if v < ORDER8:
            return v
        nwin -= 1


def directed(widths):
    out = list(FIXED)
    for W in widths:
        out += [pattern(W, 1 << (W - 1)), pattern(W, (1 << (W - 1)) + 1)]
    return out


def random_scalars(n, seed):
    """n x 32 bytes from a seeded generator (any 256-bit value)"""
    return np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)


def scalar_array(n, widths, seed):
    """(n, 32) uint8: the directed scalars first (as many as fit), seeded random ones behind them"""
    from conftest import pack
    d = pack(directed(widths)).reshape(-1, 32)[:n]
    return np.concatenate([d, random_scalars(n - len(d), seed)]) if len(d) < n else d
