"""scalar_mod_l_weak (babyjubjub-rs_amd/csrc/bjj_device.hpp): scalar_mod_l without its last conditional subtraction, which K1's
overlap form feeds its digit stream with.  Its contract -- congruent mod l, the input less q l for the quotient estimate q,
below 1.17 l -- and what the signed recoding needs of it for EVERY table width 4 .. 28 (every slot inside its window's
entries, the signed digits sum to the value, no carry leaves the top window) are checked on the CPU: the function runs in a
stand-alone program (tests/emul/weak_mod_l_main.cpp) built with AddressSanitizer and UndefinedBehaviorSanitizer, against plain
Python integers."""
import os
import random

import hostbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
ESTIMATES = sorted({(t * 10834) >> 16 for t in range(256)})      # every quotient the top byte can give


def _inputs():
    rnd = random.Random(0x4B31)
    plain = []
    for top in range(256):
        for low in [0, (1 << 248) - 1] + [rnd.getrandbits(248) for _ in range(64)]:
            plain.append((top << 248) | low)
    edges = []
    for q in ESTIMATES:
        for v in (q * L - 1, q * L, (q + 1) * L - 1, (q + 1) * L, (q + 1) * L + (1 << 232)):
            if 0 <= v < 1 << 256:
                edges.append(v)
    return plain, edges


def _digits(s, W):
    """the signed W-bit digits of s over fixed_nwin(W) windows as (slot, neg), and the carry left after the last one"""
    nwin, stride, half, carry, out = (252 + W - 1) // W, (1 << (W - 1)) + 1, 1 << (W - 1), 0, []
    for j in range(nwin):
        u = ((s >> (W * j)) & ((1 << W) - 1)) + carry
        neg = u > half
        carry = 1 if neg else 0
        out.append((j * stride + ((1 << W) - u if neg else u), neg))
    return out, carry


def test_weak_mod_l_contract_and_digits_for_every_width():
    exe = hostbuild.program("weak_mod_l_san", os.path.join(ROOT, "tests", "emul", "weak_mod_l_main.cpp"), san=True)
    plain, edges = _inputs()
    assert len(plain) == 256 * 66 and len(edges) >= 5 * (len(ESTIMATES) - 2)
    text = "".join("%064x\n" % v for v in plain) + "".join("D %064x\n" % v for v in edges)
    lines = hostbuild.run_sanitized(exe, text).split("\n")
    pos = 0
    worst = 0
    for k, v in enumerate(plain + edges):
        res, bad = lines[pos].split()
        pos += 1
        s = int(res, 16)
        q = ((v >> 248) * 10834) >> 16
        assert s == v - q * L, (hex(v), hex(s))                   # the plain-integer model: the estimate's remainder, untouched
        assert s % L == v % L and 0 <= s and 100 * s < 117 * L, (hex(v), hex(s))
        assert int(bad) == 0, (hex(v), hex(s), bad)               # slots, digit sum and last carry, every W, in the program
        worst = max(worst, s)
        if k >= len(plain):                                       # the digits themselves against the model
            for W in range(4, 29):
                f = lines[pos].split()
                pos += 1
                assert f[0] == "W" and int(f[1]) == W
                got = [(int(a), b == "1") for a, b in (t.split(":") for t in f[2:])]
                want, carry = _digits(s, W)
                assert got == want and carry == 0, (hex(v), W)
                stride = (1 << (W - 1)) + 1
                assert all(j * stride <= slot < (j + 1) * stride for j, (slot, _) in enumerate(want))
                assert sum((-1 if neg else 1) * (slot - j * stride) << (W * j) for j, (slot, neg) in enumerate(want)) == s
    assert worst >= L                                             # the inputs do reach the range the full reduction would fold
