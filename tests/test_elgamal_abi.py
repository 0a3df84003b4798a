"""include/bjj_hip_elgamal.h without a GPU: it declares the two functions and the two constants, it is plain C11, the library exports
the two, the binding knows them, what is pinned to the older headers did not move, and with a NULL context every call is
BJJ_E_INVALID and writes nothing."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "bjj_hip_elgamal.h")
FUNCTIONS = sorted(["bjj_elgamal_encrypt", "bjj_elgamal_encrypt_dev"])


def declared(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(bjj_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_the_two_functions_and_the_two_constants():
    assert declared(HEADER) == FUNCTIONS
    raw = open(HEADER).read()
    h = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    h = re.sub(r"\s+([,)])", r"\1", " ".join(h.split()))
    assert '#include "bjj_hip.h"' in h and '#include "bjj_hip_bases.h"' in h
    assert "#define BJJ_ELGAMAL_OK 1" in h and "#define BJJ_ELGAMAL_OFF_CURVE 2" in h
    assert sorted(set(re.findall(r"#define (BJJ_ELGAMAL_[A-Z_]+)", h))) == ["BJJ_ELGAMAL_OFF_CURVE", "BJJ_ELGAMAL_OK"]
    assert ("int bjj_elgamal_encrypt(bjj_ctx* ctx, const bjj_base* g, const bjj_base* pk, const uint64_t* m, const uint8_t* r, "
            "const uint8_t* add_c1_xy, const uint8_t* add_c2_xy, size_t n, uint8_t* out_c1_xy, uint8_t* out_c2_xy, uint8_t* ok);") in h
    assert ("int bjj_elgamal_encrypt_dev(bjj_ctx* ctx, const bjj_base* g, const bjj_base* pk, const void* d_m, const void* d_r, "
            "const void* d_add_c1_xy, const void* d_add_c2_xy, size_t n, void* d_out_c1_xy, void* d_out_c2_xy, void* d_ok, void* stream);") in h
    # the words the contract asks for
    for words in ("NOT CONSTANT TIME", "bjj_set_signer_constant_time", "byte for byte", "mod l", "mod 8l", "Both or neither", "a missing key",
                  "n == 0 is BJJ_OK", "A rejected call writes nothing", "before any device is touched", "no chunked pipeline", "in-place",
                  "one scratch set per stream", "is undefined", "(0, 0)"):
        assert words in raw, words


def test_header_is_plain_c11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "bjj_hip_elgamal.h"\n'
                   "int use(bjj_ctx* c, const bjj_base* g, const bjj_base* pk, const uint64_t* m, const uint8_t* r, uint8_t* out, uint8_t* ok) {\n"
                   "  int rc = bjj_elgamal_encrypt(c, g, pk, m, r, 0, 0, 0, out, out, ok);\n"
                   "  rc += bjj_elgamal_encrypt_dev(c, 0, pk, m, r, out, out, 0, out, out, ok, 0);\n"
                   "  return rc + (ok[0] == BJJ_ELGAMAL_OK) + (ok[0] == BJJ_ELGAMAL_OFF_CURVE);\n}\n")
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "use.o")],
                   check=True)


def test_library_exports_and_binding():
    lib = os.path.join(ROOT, "babyjubjub-rs_amd", "csrc", "libbjj_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    for name in FUNCTIONS:
        assert name in syms, "libbjj_hip.so does not export %s" % name
    from babyjubjub_rs_amd import _lib
    assert sorted(_lib.ELGAMAL_SYMBOLS) == FUNCTIONS and len(_lib.ELGAMAL_SYMBOLS) == 2
    assert (_lib.BJJ_ELGAMAL_OK, _lib.BJJ_ELGAMAL_OFF_CURVE) == (1, 2)
    older = (_lib.EXPORTED_SYMBOLS, _lib.EXT_SYMBOLS, _lib.BASES_SYMBOLS, _lib.SIGNER_SYMBOLS, _lib.SIGNER_SET_SYMBOLS, _lib.DLOG_SYMBOLS,
             _lib.POINT_SUM_SYMBOLS, _lib.COMMON_SYMBOLS)
    for t in older:
        assert not set(_lib.ELGAMAL_SYMBOLS) & set(t)
    loaded = _lib.load()
    for name in _lib.ELGAMAL_SYMBOLS:
        assert getattr(loaded, name).argtypes is not None
    import babyjubjub_rs_amd as bjj
    assert all(hasattr(bjj.Context, m) for m in ("elgamal_encrypt", "elgamal_rerandomize", "elgamal_encrypt_dev"))
    assert hasattr(bjj.api.FixedBase, "encrypt")


def test_the_older_headers_did_not_move():
    from babyjubjub_rs_amd import _lib
    for header, names in (("bjj_hip.h", _lib.EXPORTED_SYMBOLS), ("bjj_hip_msm_batch.h", _lib.EXT_SYMBOLS), ("bjj_hip_bases.h", _lib.BASES_SYMBOLS),
                          ("bjj_hip_signer.h", _lib.SIGNER_SYMBOLS), ("bjj_hip_signer_set.h", _lib.SIGNER_SET_SYMBOLS),
                          ("bjj_hip_dlog.h", _lib.DLOG_SYMBOLS), ("bjj_hip_point_sum.h", _lib.POINT_SUM_SYMBOLS),
                          ("bjj_hip_common_scalar.h", _lib.COMMON_SYMBOLS)):
        assert set(declared(os.path.join(INCLUDE, header))) == set(names), header
    assert len(_lib.EXPORTED_SYMBOLS) == 71
    assert (len(_lib.EXT_SYMBOLS), len(_lib.BASES_SYMBOLS), len(_lib.SIGNER_SYMBOLS), len(_lib.SIGNER_SET_SYMBOLS), len(_lib.DLOG_SYMBOLS),
            len(_lib.POINT_SUM_SYMBOLS), len(_lib.COMMON_SYMBOLS)) == (2, 6, 4, 8, 8, 2, 6)


def test_a_null_context_is_rejected_and_nothing_is_written():
    """every call below returns before the library touches a device or dereferences a table"""
    from babyjubjub_rs_amd import _lib
    lib = _lib.load()
    r = (ctypes.c_uint8 * 64)(*([0x11] * 64))
    m = (ctypes.c_uint8 * 16)(*([0x22] * 16))
    pts = (ctypes.c_uint8 * 128)()
    c1 = (ctypes.c_uint8 * 128)(*([0xEE] * 128))
    c2 = (ctypes.c_uint8 * 128)(*([0xEE] * 128))
    ok = (ctypes.c_uint8 * 16)(*([0xEE] * 16))
    fake = ctypes.c_void_p(0x1230)
    for n in (0, 2):
        for g in (None, fake):
            for pk in (None, fake):
                for mm in (None, m):
                    for add in ((None, None), (pts, pts), (pts, None)):
                        assert lib.bjj_elgamal_encrypt(None, g, pk, mm, r, add[0], add[1], n, c1, c2, ok) == _lib.BJJ_E_INVALID
                        assert b"ctx is NULL" in lib.bjj_last_error()
                        assert lib.bjj_elgamal_encrypt_dev(None, g, pk, mm, r, add[0], add[1], n, c1, c2, ok, None) == _lib.BJJ_E_INVALID
                        assert b"ctx is NULL" in lib.bjj_last_error()
    assert bytes(c1) == b"\xee" * 128 and bytes(c2) == b"\xee" * 128 and bytes(ok) == b"\xee" * 16
    assert bytes(r) == b"\x11" * 64 and bytes(m) == b"\x22" * 16 and bytes(pts) == bytes(128)
