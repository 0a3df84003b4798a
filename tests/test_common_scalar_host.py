"""One scalar, many points without a GPU: the host's recoding (both forms, both signs), the form rule, and the per-lane item of
bjj_k_mul_common in both forms with the point and the subgroup epilogue -- the bodies of csrc/common_scalar.hpp run on the CPU
(tests/common_scalar_emul, bound assertions on) -- against the Python oracle's mul_scalar / add / affine (src/lib.rs:149-164,
88-131, 70-85)."""
import ctypes
import os
import random

import pytest

import hostbuild
from conftest import ROOT
from test_msm_host import L, ORDER8, le

EMUL_DIR = os.path.join(ROOT, "tests", "common_scalar_emul")
NAF, TABLE = 0, 1
FORMS = (NAF, TABLE)
FIXED_SCALARS = [0, 1, 2, 8, L - 1, L, L + 1, ORDER8 - 1, ORDER8, ORDER8 + 1, 1 << 253, (1 << 254) - 1, (1 << 256) - 1,
                 int("AA" * 32, 16), int("55" * 32, 16), (1 << 255) - 1, 0xD1B54A32D192ED03, 0x9E3779B97F4A7C15F39CC0605CEDC834]


def all_scalars():
    rng = random.Random(0xC5CA)
    return FIXED_SCALARS + [rng.getrandbits(256) for _ in range(1000)]


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(hostbuild.shared("libcommon_scalar_emul.so", os.path.join(EMUL_DIR, "common_scalar_emul.cpp")))
    lib.cs_emul_recode.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_byte), ctypes.POINTER(ctypes.c_int)]
    lib.cs_emul_choose.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.cs_emul_mul.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p,
                                ctypes.c_char_p]
    lib.cs_emul_subgroup.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p]
    return lib


def recode(lib, k, negate, form):
    d = (ctypes.c_byte * (lib.cs_emul_max_digits() + 1))()
    top = ctypes.c_int(-7)
    weight = lib.cs_emul_recode(le(k), 1 if negate else 0, form, d, ctypes.byref(top))
    return list(d), top.value, weight


def records(pts):
    return b"".join(le(x) + le(y) for x, y in pts)


def emul_mul(lib, k, pts, add, subtract, form):
    n = len(pts)
    out = ctypes.create_string_buffer(64 * n)
    ok = ctypes.create_string_buffer(n)
    assert lib.cs_emul_mul(le(k), records(pts), None if add is None else records(add), 1 if subtract else 0, n, form, out, ok) == 0
    r = out.raw
    return [(int.from_bytes(r[64 * i:64 * i + 32], "little"), int.from_bytes(r[64 * i + 32:64 * i + 64], "little")) for i in range(n)], list(ok.raw)


# ---- the recoding -----------------------------------------------------------------------------------------------------------------
def test_both_recodings_and_their_negations(emul):
    assert emul.cs_emul_max_digits() == 255
    for k in all_scalars():
        for form in FORMS:
            gap, limit = (2, 1) if form == NAF else (5, 15)
            for negate in (False, True):
                d, top, weight = recode(emul, k, negate, form)
                assert len(d) == 256 and d[255] == 0                                        # at most 255 digits: it fits the array
                assert sum(x << i for i, x in enumerate(d)) % ORDER8 == (-k if negate else k) % ORDER8, (k, form, negate)
                nz = [i for i, x in enumerate(d) if x]
                assert top == (nz[-1] if nz else -1) and weight == len(nz)
                assert all(x % 2 == 1 and abs(x) <= limit for x in d if x), (k, form)     # odd digits of the form's set
                assert all(b - a >= gap for a, b in zip(nz, nz[1:])), (k, form)            # no two adjacent; five apart for width 5
            plus, minus = recode(emul, k, False, form)[0], recode(emul, k, True, form)[0]
            assert minus == [-x for x in plus]                                              # a subtraction is a sign flip
    assert recode(emul, 0, False, NAF)[1] == recode(emul, ORDER8, True, TABLE)[1] == -1     # k == 0 (mod 8l): no digit at all
    assert recode(emul, 8, False, NAF) == ([0, 0, 0, 1] + [0] * 252, 3, 1)                   # 8 P: three doublings


def test_the_form_rule_counts_multiplications(emul):
    a, b = ctypes.c_int(), ctypes.c_int()
    assert emul.cs_emul_choose(le(8), ctypes.byref(a), ctypes.byref(b)) == NAF
    assert (a.value, b.value) == (7, 73 + 8)             # one mixed addition against the table and one table addition
    print("k = 8: table-free %d multiplications, table %d" % (a.value, b.value))
    rng = random.Random(0xF0)
    for bits, want in ((16, NAF), (32, NAF), (254, TABLE)):
        for _ in range(20):
            k = rng.getrandbits(bits) | (1 << (bits - 1))
            form = emul.cs_emul_choose(le(k), ctypes.byref(a), ctypes.byref(b))
            wn, ww = recode(emul, k, False, NAF)[2], recode(emul, k, False, TABLE)[2]
            assert (a.value, b.value) == (7 * wn, 73 + 8 * ww) and form == (TABLE if b.value < a.value else NAF) == want, (bits, k)
    assert emul.cs_emul_choose(le(L), ctypes.byref(a), ctypes.byref(b)) == TABLE   # the subgroup check: full width
    print("k = l: table-free %d multiplications, table %d" % (a.value, b.value))


# ---- items ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def points(pyoracle):
    """name -> point: B8, the identity, orders 2, 4, 8, subgroup points, subgroup + torsion, a coordinate >= r, off-curve, (0, 0)"""
    o = pyoracle
    rng = random.Random(0xC5C0)
    tors = [o.mul_scalar(o.T8, j) for j in range(8)]
    assert tors[0] == (0, 1) and tors[4] == (0, o.Q - 1)          # orders 1 and 2; tors[2]: 4, tors[1]: 8
    sub = [o.mul_scalar(o.B8, rng.randrange(1, L)) for _ in range(4)]
    shifted = [tuple(o.proj_affine(o.proj_add((*sub[j], 1), (*tors[t], 1)))) for j, t in ((0, 1), (1, 4), (2, 2), (3, 7))]
    big = (sub[0][0] + o.Q, sub[0][1])                            # x >= r and < 2^256: reduced mod r
    assert big[0] < 1 << 256
    off = (sub[1][0] ^ 1, sub[1][1])
    pts = [o.B8, tors[0], tors[4], tors[2], tors[1]] + sub + shifted + [big, off, (0, 0)]
    return {"pts": pts, "tors": tors, "sub": sub, "n_on": len(pts) - 2}


def reduced(o, p):
    return (p[0] % o.Q, p[1] % o.Q)


def on_curve(o, p):
    x, y = reduced(o, p)
    return (o.A * x * x + y * y - 1 - o.D * x * x * y * y) % o.Q == 0


def want_item(o, k, p, a, subtract):
    if not on_curve(o, p) or (a is not None and not on_curve(o, a)):
        return (0, 0), 2
    kp = o.mul_scalar(reduced(o, p), k % ORDER8)
    if subtract:
        kp = ((o.Q - kp[0]) % o.Q, kp[1])
    if a is None:
        return tuple(kp), 1
    return tuple(o.proj_affine(o.proj_add((*reduced(o, a), 1), (*kp, 1)))), 1


ITEM_SCALARS = [0, 1, 2, 8, L - 1, L, ORDER8 - 1, ORDER8 + 1, (1 << 256) - 1, int("AA" * 32, 16), 0xD1B54A32D192ED03,
                0x9E3779B97F4A7C15F39CC0605CEDC834, 0x0B3C9F1E5D7A2C48E6F1093B5A7D2C4E8F6A1B3C5D7E9F0A1B2C3D4E5F60718]


@pytest.mark.parametrize("form", FORMS, ids=["table_free", "table"])
def test_items_against_the_oracle(emul, pyoracle, points, form):
    o = pyoracle
    pts = points["pts"]
    n = len(pts)
    for k in ITEM_SCALARS:
        prod = {s: [want_item(o, k, p, None, s)[0] for p in pts] for s in (False, True)}
        addends = {
            "absent": None,
            "identity": [(0, 1)] * n,
            "+kP": prod[False][:points["n_on"]] + [o.B8, o.B8],
            "-kP": prod[True][:points["n_on"]] + [o.B8, o.B8],
            "torsion": [points["tors"][(i % 7) + 1] for i in range(n)],
            "off_curve": [(pts[5][0], pts[5][1] ^ 1) if i % 2 else points["sub"][i % 4] for i in range(n)],
        }
        for name, add in addends.items():
            for subtract in (False, True):
                got, ok = emul_mul(emul, k, pts, add, subtract, form)
                want = [want_item(o, k, p, None if add is None else add[i], subtract) for i, p in enumerate(pts)]
                assert got == [w[0] for w in want] and ok == [w[1] for w in want], (hex(k), name, subtract)
                if name == ("-kP" if not subtract else "+kP"):   # A - kP with A = kP, and A + kP with A = -kP: the identity
                    assert all(g == (0, 1) for g in got[:points["n_on"]])
        assert ok[-2:] == [2, 2]


@pytest.mark.parametrize("form", FORMS, ids=["table_free", "table"])
def test_the_subgroup_epilogue(emul, pyoracle, points, form):
    o = pyoracle
    pts = points["pts"]
    want = [2 if not on_curve(o, p) else 1 if tuple(o.mul_scalar(reduced(o, p), L)) == (0, 1) else 0 for p in pts]
    assert want[:5] == [1, 1, 0, 0, 0] and want[5:9] == [1] * 4 and want[9:13] == [0] * 4 and want[13:] == [1, 2, 2]
    ok = ctypes.create_string_buffer(len(pts))
    assert emul.cs_emul_subgroup(records(pts), len(pts), form, ok) == 0
    assert list(ok.raw) == want


# ---- the same bodies under the sanitizers -----------------------------------------------------------------------------------------
def test_the_mixed_case_under_asan_and_ubsan():
    """a stand-alone program: the harness and its driver compiled with -fsanitize=address,undefined, run directly"""
    hostbuild.need_sanitizer_runtimes()
    out = hostbuild.run_sanitized(hostbuild.program("common_scalar_emul_san", os.path.join(EMUL_DIR, "common_scalar_emul_main.cpp"), san=True), timeout=600)
    assert "common_scalar ok" in out, out[-3000:]
