"""bjj_elgamal_encrypt without a GPU: the per-item body of bjj_k_elgamal_encrypt (csrc/elgamal.hpp) run on the CPU
(tests/elgamal_emul, bound assertions on) over tables built in host memory, against the Python oracle's mul_scalar / add / affine
(src/lib.rs:149-164, 88-131, 70-85); the short m-chain's recoding in plain integers; and the same harness as a stand-alone program
under AddressSanitizer and UndefinedBehaviorSanitizer."""
import ctypes
import os
import random

import pytest

import bases_cases
from bases_cases import L, ORDER8
import hostbuild
from conftest import ROOT

EMUL_DIR = os.path.join(ROOT, "tests", "elgamal_emul")
WIDTHS = (4, 5, 13, 16)
M64 = (1 << 64) - 1


def le(v, size=32):
    return int(v).to_bytes(size, "little")


def nwin_m(W):
    return -(-65 // W)


def m_pattern(W, digit):
    """every window = digit, cut at the top until the value is below 2^64"""
    n = nwin_m(W)
    while True:
        v = sum(digit << (W * j) for j in range(n))
        if v <= M64:
            return v
        n -= 1


def m_edges(W):
    h = 1 << (W - 1)
    return [0, 1, h, h + 1, 1 << 63, M64, m_pattern(W, h), m_pattern(W, h + 1)]


def recode(m, W, nwin):
    """signed W-bit digits, LSB first: a window above 2^(W-1) becomes negative and carries (bjj_device.hpp: digit_next)"""
    out, carry = [], 0
    for j in range(nwin):
        u = ((m >> (W * j)) & ((1 << W) - 1)) + carry
        carry = 1 if u > (1 << (W - 1)) else 0
        out.append(u - (1 << W) if carry else u)
    return out, carry


# ---- the m-chain's recoding, in plain integers ------------------------------------------------------------------------------------
def test_the_short_recoding_of_m_is_exact_and_its_top_digit_is_not_negative():
    for W in range(4, 29):
        n = nwin_m(W)
        assert n >= 3 and W * n >= 65 and W * (n - 1) < 65
        for m in m_edges(W) + [M64 - 1, (1 << 63) + 1]:
            d, carry = recode(m, W, n)
            assert carry == 0 and d[-1] >= 0, (W, hex(m))                  # nothing leaves the chain
            assert sum(x << (W * j) for j, x in enumerate(d)) == m, (W, hex(m))
            assert all(abs(x) <= 1 << (W - 1) for x in d)                   # every digit has a table entry
        neg = recode(m_pattern(W, (1 << (W - 1)) + 1), W, n)[0]
        assert neg[0] < 0 and sum(1 for x in neg if x < 0) >= min(n - 1, 64 // W)   # the all-negative pattern is what its name says


# ---- the harness --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(hostbuild.shared("libelgamal_emul.so", os.path.join(EMUL_DIR, "elgamal_emul.cpp")))
    lib.eg_emul_table.argtypes = [ctypes.c_char_p, ctypes.c_int]
    lib.eg_emul_digits.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)]
    lib.eg_emul_digits.restype = None
    lib.eg_emul_encrypt.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t,
                                    ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    lib.eg_emul_free_tables.restype = None
    yield lib
    lib.eg_emul_free_tables()


def test_the_device_digit_stream_gives_that_recoding(emul):
    rng = random.Random(0xE16A)
    for W in range(4, 29):
        n = nwin_m(W)
        assert emul.eg_emul_nwin_m(W) == n
        for m in m_edges(W) + [rng.getrandbits(64) for _ in range(20)]:
            d = (ctypes.c_longlong * n)()
            emul.eg_emul_digits(m, W, n, d)
            assert list(d) == recode(m, W, n)[0], (W, hex(m))


@pytest.fixture(scope="module")
def world(emul, pyoracle):
    """the points and their tables: g in {context B8 at W 4 / 13, a generator of the whole group at W 5 / 16}, pk of four kinds"""
    o = pyoracle
    rng = random.Random(0xE16B)
    sub = o.mul_scalar(o.B8, rng.randrange(1, L))                                   # in the prime-order subgroup
    full = tuple(o.proj_affine(o.proj_add((*o.B8, 1), (*o.T8, 1))))                 # order 8l
    gen = tuple(o.proj_affine(o.proj_add((*o.mul_scalar(o.B8, 0x1234567), 1), (*o.mul_scalar(o.T8, 3), 1))))   # another one of order 8l
    pts = {"sub": sub, "full": full, "torsion": tuple(o.T8), "identity": (0, 1), "gen": gen}

    def table(name, W):
        h = emul.eg_emul_table(None if name is None else le(pts[name][0]) + le(pts[name][1]), W)
        assert h >= 0, (name, W, h)
        return h

    g = {("b8", 4): table(None, 4), ("b8", 13): table(None, 13), ("gen", 5): table("gen", 5), ("gen", 16): table("gen", 16)}
    pk = {("sub", 16): table("sub", 16), ("full", 13): table("full", 13), ("torsion", 4): table("torsion", 4), ("identity", 5): table("identity", 5),
          ("sub", 4): table("sub", 4), ("full", 5): table("full", 5)}
    pts["b8"] = tuple(o.B8)
    return {"pts": pts, "g": g, "pk": pk}


# (g, pk): every width on either side, mixed, and every kind of key
COMBOS = [(("b8", 4), ("sub", 16)), (("b8", 13), ("full", 5)), (("gen", 5), ("full", 13)), (("gen", 16), ("sub", 4)),
          (("b8", 4), ("torsion", 4)), (("gen", 5), ("identity", 5))]


def padd(o, p, q):
    return tuple(o.proj_affine(o.proj_add((*p, 1), (*q, 1))))


def neg(o, p):
    return ((o.Q - p[0]) % o.Q, p[1])


def on_curve(o, p):
    x, y = p[0] % o.Q, p[1] % o.Q
    return (o.A * x * x + y * y - 1 - o.D * x * x * y * y) % o.Q == 0


def records(pts):
    return b"".join(le(x) + le(y) for x, y in pts)


def run(emul, g, pk, m, r, add, in_place=False, want_ok=True):
    n = len(r)
    c1, c2, ok = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)
    rc = emul.eg_emul_encrypt(g, pk, None if m is None else b"".join(le(x, 8) for x in m), b"".join(le(x) for x in r),
                              None if add is None else records(add[0]), None if add is None else records(add[1]), n, 1 if in_place else 0,
                              c1, c2, ok if want_ok else None)
    assert rc == 0, rc

    def pts(buf):
        b = buf.raw
        return [(int.from_bytes(b[64 * i:64 * i + 32], "little"), int.from_bytes(b[64 * i + 32:64 * i + 64], "little")) for i in range(n)]
    return pts(c1), pts(c2), list(ok.raw)


def scalars_for(gw, pw, n_random, seed):
    rng = random.Random(seed)
    rs = bases_cases.directed(sorted({gw, pw})) + [rng.getrandbits(256) for _ in range(n_random)]
    pool = m_edges(gw) + [rng.getrandbits(64) for _ in range(n_random)]
    return [pool[i % len(pool)] for i in range(len(rs))], rs


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "g_%s%d_pk_%s%d" % (c[0] + c[1]))
def test_items_against_the_oracle(emul, pyoracle, world, combo):
    o = pyoracle
    (gname, gw), (pname, pw) = combo
    G, PK = world["pts"][gname], world["pts"][pname]
    gmod = L if gname == "b8" else ORDER8                      # what the chain reduces r by; the point's order divides it
    ms, rs = scalars_for(gw, pw, 6, 0xE16C + gw * 32 + pw)
    n = len(rs)
    rG = [tuple(o.mul_scalar(G, r % gmod)) for r in rs]
    want1 = rG
    want2 = [padd(o, tuple(o.mul_scalar(G, m)), tuple(o.mul_scalar(PK, r % ORDER8))) for m, r in zip(ms, rs)]
    want2_m0 = [tuple(o.mul_scalar(PK, r % ORDER8)) for r in rs]
    hg, hp = world["g"][(gname, gw)], world["pk"][(pname, pw)]

    c1, c2, ok = run(emul, hg, hp, ms, rs, None)
    assert c1 == want1 and c2 == want2 and ok == [1] * n
    assert run(emul, hg, hp, ms, rs, None, want_ok=False)[:2] == (want1, want2)           # ok may be left out
    assert run(emul, hg, hp, None, rs, None)[:2] == (want1, want2_m0)                     # m = None: the m-chain is not run
    assert run(emul, hg, hp, [0] * n, rs, None)[:2] == (want1, want2_m0)

    # add arrays: the identity, -result (the sum is the identity), the term itself (a doubling), torsion, a coordinate >= r
    big = (world["pts"]["sub"][0] + o.Q, world["pts"]["sub"][1])
    assert big[0] < 1 << 256
    adds = {
        "identity": ([(0, 1)] * n, [(0, 1)] * n),
        "minus": ([neg(o, p) for p in want1], [neg(o, p) for p in want2]),
        "same": (list(want1), list(want2)),
        "mixed": ([world["pts"]["torsion"], big] * (n // 2) + [big] * (n % 2), [big, world["pts"]["full"]] * (n // 2) + [big] * (n % 2)),
    }
    for name, (a1, a2) in adds.items():
        e1 = [padd(o, (a[0] % o.Q, a[1]), p) for a, p in zip(a1, want1)]
        e2 = [padd(o, (a[0] % o.Q, a[1]), p) for a, p in zip(a2, want2)]
        for in_place in (False, True):
            assert run(emul, hg, hp, ms, rs, (a1, a2), in_place) == (e1, e2, [1] * n), (name, in_place)
        if name == "minus":
            assert e1 == [(0, 1)] * n and e2 == [(0, 1)] * n
    # re-randomisation: m = None with add arrays
    a1, a2 = adds["same"]
    assert run(emul, hg, hp, None, rs, (a1, a2)) == ([padd(o, a, p) for a, p in zip(a1, want1)], [padd(o, a, p) for a, p in zip(a2, want2_m0)],
                                                      [1] * n)

    # an off-curve A1 only, an off-curve A2 only, (0, 0) on either side: that item alone is refused
    off = (world["pts"]["sub"][0] ^ 1, world["pts"]["sub"][1])
    assert not on_curve(o, off) and not on_curve(o, (0, 0)) and on_curve(o, big)
    a1, a2 = list(want1), list(want2)
    a1[1] = off; a2[3] = off; a1[4] = (0, 0); a2[6] = (0, 0); a1[7] = off; a2[7] = (0, 0)
    bad = {1, 3, 4, 6, 7}
    e1 = [(0, 0) if i in bad else padd(o, a1[i], want1[i]) for i in range(n)]
    e2 = [(0, 0) if i in bad else padd(o, a2[i], want2[i]) for i in range(n)]
    eok = [2 if i in bad else 1 for i in range(n)]
    for in_place in (False, True):
        assert run(emul, hg, hp, ms, rs, (a1, a2), in_place) == (e1, e2, eok), in_place


def test_the_harness_rejects_what_the_library_rejects(emul, world):
    hg, hp = world["g"][("b8", 4)], world["pk"][("sub", 4)]
    z = ctypes.create_string_buffer(64)
    r = le(5)
    one = records([(0, 1)])
    assert emul.eg_emul_encrypt(hg, hp, None, r, one, None, 1, 0, z, z, z) == -1      # one add array alone
    assert emul.eg_emul_encrypt(hg, hg, None, r, None, None, 1, 0, z, z, z) == -1     # the context's table is no key
    assert emul.eg_emul_table(le(1) + le(1), 4) == -1                                 # off the curve


# ---- the same body under the sanitizers ---------------------------------------------------------------------------------------------
def test_the_mixed_case_under_asan_and_ubsan():
    """a stand-alone program: the harness and its driver compiled with -fsanitize=address,undefined, run directly"""
    out = hostbuild.run_sanitized(hostbuild.program("elgamal_emul_san", os.path.join(EMUL_DIR, "elgamal_emul_main.cpp"), san=True), timeout=600)
    assert "elgamal ok" in out, out[-3000:]
