"""The sign-carrying recurrence of K1's overlap form (babyjubjub-rs_amd/csrc/k_fixed.hip, BJJ_K1_SIGN_CARRY): the accumulator
holds R_j = eps_j S_j (eps_j the sign of window j's digit, S_j the partial sum), R_j = (eps_j eps_{j-1}) R_{j-1} + Q_j with the
table entry Q_j exactly as stored, and the negation is a select inside the addition that makes the accumulator.  The functions
the kernel runs (curve.hpp: niels_tform_state, ext_madd_state, ext_madd_forms) run here on the CPU in a stand-alone program
(tests/emul/k1_sign_carry_main.cpp) built with AddressSanitizer, UndefinedBehaviorSanitizer and BJJ_DEBUG_BOUNDS -- every
multiplication and lazy subtraction asserts its operands' limb bounds -- against fixed_base_mul on the same entries, for every
table width 4 .. 28.  Equal means: the same affine point.

Inputs per width: 0, 1, l - 1, l, l + 1, 2^254 - 1; digit strings that are all positive, all negative (below a positive top
digit: the value is positive) and alternating either way; a zero digit in each window position in turn, inside an alternating
string; every window all ones (digit -1, then the recoding carry runs through every window to the top); and 2^12 random
scalars dealt over the widths.  The digit strings are built and checked with plain integers here."""
import os
import random
import subprocess

import hostbuild
from test_k1_weak_mod_l_host import L, _digits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = list(range(4, 29))
RANDOM = 1 << 12
PROCESSES = 8


def _nwin(W):
    return (252 + W - 1) // W


def _value(digits, W):
    return sum(d << (W * j) for j, d in enumerate(digits))


def _signs(v, W):
    """the signs of the digits of v < l as the recoding gives them: +1, -1, 0"""
    out, carry = _digits(v, W)
    assert carry == 0
    stride = (1 << (W - 1)) + 1
    return [0 if slot == j * stride else (-1 if neg else 1) for j, (slot, neg) in enumerate(out)]


def _directed(W):
    nw = _nwin(W)
    top = [1]                                                   # the top digit of a positive number below l
    pos = [3] * (nw - 1) + top
    neg = [-3] * (nw - 1) + top
    alt0 = [3 if j % 2 == 0 else -3 for j in range(nw - 1)] + top
    alt1 = [-3 if j % 2 == 0 else 3 for j in range(nw - 1)] + top
    out = [0, 1, L - 1, L, L + 1, (1 << 254) - 1]
    for digits, want in ((pos, 1), (neg, -1)):
        v = _value(digits, W)
        assert 0 < v < L and all(s == want for s in _signs(v, W)[:-1]) and _signs(v, W)[-1] == 1
        out.append(v)
    for digits in (alt0, alt1):
        v = _value(digits, W)
        s = _signs(v, W)
        assert 0 < v < L and all(s[j] == -s[j + 1] for j in range(nw - 2)) and s[-1] == 1
        out.append(v)
    for p in range(nw):                                         # a zero digit in window p
        digits = list(alt1 if p % 2 else alt0)
        digits[p] = 0
        if p == nw - 1:
            digits[p - 1] = 3                                   # a positive number still
        v = _value(digits, W)
        assert 0 <= v < L and _signs(v, W)[p] == 0, (W, p)
        out.append(v)
    v = ((1 << (W * nw)) - 1) & ((1 << 250) - 1)               # all ones: -1, then the carry through every window
    s = _signs(v, W)
    assert s[0] == -1 and not any(s[1:-1]) and s[-1] == 1
    out.append(v)
    return out


def test_sign_carry_equals_fixed_base_mul_for_every_width(tmp_path):
    exe = hostbuild.program("k1_sign_carry_san", os.path.join(ROOT, "tests", "emul", "k1_sign_carry_main.cpp"), san=True, opt="-O2",
                            defines=("BJJ_DEBUG_BOUNDS",))
    rnd = random.Random(0x51C7)
    lines = {W: [(W, v) for v in _directed(W)] for W in WIDTHS}
    for i in range(RANDOM):
        W = WIDTHS[i % len(WIDTHS)]
        lines[W].append((W, rnd.getrandbits(256) if i % 3 else rnd.getrandbits(254)))
    # one process per share of the widths (the program keeps one width's entries at a time), the wide and narrow ones mixed
    shares = [[c for W in WIDTHS[k::PROCESSES] for c in lines[W]] for k in range(PROCESSES)]
    procs = []
    for k, share in enumerate(shares):                          # through files: no pipe can fill up
        (tmp_path / ("in%d" % k)).write_text("".join("%d %064x\n" % c for c in share))
        procs.append(subprocess.Popen([exe], stdin=open(str(tmp_path / ("in%d" % k))), stdout=open(str(tmp_path / ("out%d" % k)), "w"),
                                      stderr=open(str(tmp_path / ("err%d" % k)), "w")))
    total = 0
    codes = [p.wait() for p in procs]
    for k, share in enumerate(shares):
        err = (tmp_path / ("err%d" % k)).read_text()
        assert codes[k] == 0, (codes[k], err[-3000:])           # a failed bound or a sanitizer report ends the program
        rows = (tmp_path / ("out%d" % k)).read_text().split("\n")
        assert len(rows) == len(share) + 1
        for (W, v), row in zip(share, rows):
            f = row.split()
            assert int(f[0]) == W and int(f[1]) == 0, (W, hex(v), row)
            if v % L == 0:
                assert int(f[2], 16) == 0 and int(f[3], 16) == 1   # the identity
            total += 1
    assert total == RANDOM + sum(10 + _nwin(W) + 1 for W in WIDTHS)
