"""include/bjj_hip_common_scalar.h without a GPU: it declares the six functions and the two constants, it is plain C11, the library
exports the six, the binding knows them, what is pinned to the older headers did not move, and with a NULL context every call is
BJJ_E_INVALID and writes nothing."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "bjj_hip_common_scalar.h")
FUNCTIONS = sorted(["bjj_mul_common", "bjj_mul_common_dev", "bjj_in_subgroup", "bjj_in_subgroup_dev", "bjj_elgamal_decrypt",
                    "bjj_elgamal_decrypt_dev"])


def declared(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(bjj_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_the_six_functions_and_the_two_constants():
    assert declared(HEADER) == FUNCTIONS
    raw = open(HEADER).read()
    h = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    h = re.sub(r"\s+([,)])", r"\1", " ".join(h.split()))
    assert '#include "bjj_hip.h"' in h
    assert "#define BJJ_COMMON_OK 1" in h and "#define BJJ_COMMON_OFF_CURVE 2" in h
    assert sorted(set(re.findall(r"#define (BJJ_COMMON_[A-Z_]+)", h))) == ["BJJ_COMMON_OFF_CURVE", "BJJ_COMMON_OK"]
    assert ("int bjj_mul_common(bjj_ctx* ctx, const uint8_t* scalar, const uint8_t* pts_xy, const uint8_t* add_xy, int subtract, size_t n, "
            "uint8_t* out_xy, uint8_t* ok);") in h
    assert ("int bjj_mul_common_dev(bjj_ctx* ctx, const uint8_t* scalar, const void* d_pts_xy, const void* d_add_xy, int subtract, size_t n, "
            "void* d_out_xy, void* d_ok, void* stream);") in h
    assert "int bjj_in_subgroup(bjj_ctx* ctx, const uint8_t* pts_xy, size_t n, uint8_t* ok);" in h
    assert "int bjj_in_subgroup_dev(bjj_ctx* ctx, const void* d_pts_xy, size_t n, void* d_ok, void* stream);" in h
    assert ("int bjj_elgamal_decrypt(bjj_ctx* ctx, const bjj_dlog_table* table, const uint8_t* sk, const uint8_t* c1_xy, const uint8_t* c2_xy, "
            "size_t n, int range_bits, uint64_t* out_m, uint8_t* ok);") in h
    assert ("int bjj_elgamal_decrypt_dev(bjj_ctx* ctx, const bjj_dlog_table* table, const uint8_t* sk, const void* d_c1_xy, "
            "const void* d_c2_xy, size_t n, int range_bits, void* d_out_m, void* d_ok, void* stream);") in h
    # the words the contract asks for: not constant time, and the knob
    assert "NOT CONSTANT TIME" in raw and "BJJ_COMMON_FORM" in raw and "bjj_set_signer_constant_time" in raw


def test_header_is_plain_c11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "bjj_hip_common_scalar.h"\n'
                   "int use(bjj_ctx* c, const bjj_dlog_table* t, const uint8_t* k, const uint8_t* p, uint8_t* out, uint64_t* m, uint8_t* ok) {\n"
                   "  int rc = bjj_mul_common(c, k, p, 0, 0, 0, out, ok) + bjj_mul_common_dev(c, k, p, p, 1, 0, out, ok, 0);\n"
                   "  rc += bjj_in_subgroup(c, p, 0, ok) + bjj_in_subgroup_dev(c, p, 0, ok, 0);\n"
                   "  rc += bjj_elgamal_decrypt(c, t, k, p, p, 0, 32, m, ok) + bjj_elgamal_decrypt_dev(c, t, k, p, p, 0, 32, m, ok, 0);\n"
                   "  return rc + (ok[0] == BJJ_COMMON_OK) + (ok[0] == BJJ_COMMON_OFF_CURVE);\n}\n")
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "use.o")],
                   check=True)


def test_library_exports_and_binding():
    lib = os.path.join(ROOT, "babyjubjub-rs_amd", "csrc", "libbjj_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    for name in FUNCTIONS:
        assert name in syms, "libbjj_hip.so does not export %s" % name
    from babyjubjub_rs_amd import _lib
    assert sorted(_lib.COMMON_SYMBOLS) == FUNCTIONS and len(_lib.COMMON_SYMBOLS) == 6
    assert (_lib.BJJ_COMMON_OK, _lib.BJJ_COMMON_OFF_CURVE) == (1, 2)
    older = (_lib.EXPORTED_SYMBOLS, _lib.EXT_SYMBOLS, _lib.BASES_SYMBOLS, _lib.SIGNER_SYMBOLS, _lib.SIGNER_SET_SYMBOLS, _lib.DLOG_SYMBOLS,
             _lib.POINT_SUM_SYMBOLS)
    for t in older:
        assert not set(_lib.COMMON_SYMBOLS) & set(t)
    loaded = _lib.load()
    for name in _lib.COMMON_SYMBOLS:
        assert getattr(loaded, name).argtypes is not None
    import babyjubjub_rs_amd as bjj
    assert all(hasattr(bjj.Context, m) for m in ("mul_common", "mul_common_dev", "in_subgroup", "in_subgroup_dev", "decrypt", "decrypt_dev",
                                                 "elgamal_decrypt"))


def test_the_older_headers_did_not_move():
    from babyjubjub_rs_amd import _lib
    for header, names in (("bjj_hip.h", _lib.EXPORTED_SYMBOLS), ("bjj_hip_msm_batch.h", _lib.EXT_SYMBOLS), ("bjj_hip_bases.h", _lib.BASES_SYMBOLS),
                          ("bjj_hip_signer.h", _lib.SIGNER_SYMBOLS), ("bjj_hip_signer_set.h", _lib.SIGNER_SET_SYMBOLS),
                          ("bjj_hip_dlog.h", _lib.DLOG_SYMBOLS), ("bjj_hip_point_sum.h", _lib.POINT_SUM_SYMBOLS)):
        assert set(declared(os.path.join(INCLUDE, header))) == set(names), header
    assert len(_lib.EXPORTED_SYMBOLS) == 71
    assert (len(_lib.EXT_SYMBOLS), len(_lib.BASES_SYMBOLS), len(_lib.SIGNER_SYMBOLS), len(_lib.SIGNER_SET_SYMBOLS), len(_lib.DLOG_SYMBOLS),
            len(_lib.POINT_SUM_SYMBOLS)) == (2, 6, 4, 8, 8, 2)


def test_a_null_context_is_rejected_and_nothing_is_written():
    """every call below returns before the library touches a device or dereferences a table"""
    from babyjubjub_rs_amd import _lib
    lib = _lib.load()
    k = (ctypes.c_uint8 * 32)(*([0x11] * 32))
    pts = (ctypes.c_uint8 * 128)()
    out = (ctypes.c_uint8 * 128)(*([0xEE] * 128))
    m = (ctypes.c_uint8 * 16)(*([0xEE] * 16))
    ok = (ctypes.c_uint8 * 16)(*([0xEE] * 16))
    fake = ctypes.c_void_p(0x1230)
    for n in (0, 2):
        for sub in (0, 1):
            for add in (None, pts):
                assert lib.bjj_mul_common(None, k, pts, add, sub, n, out, ok) == _lib.BJJ_E_INVALID
                assert b"ctx is NULL" in lib.bjj_last_error()
                assert lib.bjj_mul_common_dev(None, k, pts, add, sub, n, out, ok, None) == _lib.BJJ_E_INVALID
                assert b"ctx is NULL" in lib.bjj_last_error()
        assert lib.bjj_mul_common(None, None, pts, None, 0, n, out, ok) == _lib.BJJ_E_INVALID
        assert lib.bjj_in_subgroup(None, pts, n, ok) == _lib.BJJ_E_INVALID and b"ctx is NULL" in lib.bjj_last_error()
        assert lib.bjj_in_subgroup_dev(None, pts, n, ok, None) == _lib.BJJ_E_INVALID and b"ctx is NULL" in lib.bjj_last_error()
        for t in (fake, None):
            for rb in (0, 16, 46):
                assert lib.bjj_elgamal_decrypt(None, t, k, pts, pts, n, rb, m, ok) == _lib.BJJ_E_INVALID
                assert b"ctx is NULL" in lib.bjj_last_error()
                assert lib.bjj_elgamal_decrypt_dev(None, t, k, pts, pts, n, rb, m, ok, None) == _lib.BJJ_E_INVALID
                assert b"ctx is NULL" in lib.bjj_last_error()
    assert bytes(out) == b"\xee" * 128 and bytes(m) == b"\xee" * 16 and bytes(ok) == b"\xee" * 16
    assert bytes(k) == b"\x11" * 32 and bytes(pts) == bytes(128)
