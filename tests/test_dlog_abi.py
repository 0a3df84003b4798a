"""include/bjj_hip_dlog.h without a GPU: it parses, it is plain C11, the library exports the eight functions it declares, the
binding knows them, what is pinned to the other headers did not move, and the argument checks that need no device answer
BJJ_E_INVALID and write nothing."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "bjj_hip_dlog.h")
FUNCTIONS = sorted(["bjj_dlog_table_create", "bjj_dlog_table_free", "bjj_dlog_table_info", "bjj_dlog_table_check", "bjj_dlog_table_base",
                    "bjj_dlog_max_range_bits", "bjj_dlog", "bjj_dlog_dev"])


def declared(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(bjj_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_the_eight_functions():
    assert declared(HEADER) == FUNCTIONS
    h = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    h = re.sub(r"\s+([,)])", r"\1", " ".join(h.split()))
    assert '#include "bjj_hip.h"' in h
    assert "typedef struct bjj_dlog_table bjj_dlog_table;" in h
    for name, value in (("NOT_IN_RANGE", 0), ("FOUND", 1), ("OFF_CURVE", 2), ("MAX_GIANT_BITS", 16)):
        assert "#define BJJ_DLOG_%s %d" % (name, value) in h
    assert "int bjj_dlog_table_create(bjj_ctx* ctx, const uint8_t* point_xy, int baby_bits, bjj_dlog_table** out);" in h
    assert "int bjj_dlog_table_free(bjj_ctx* ctx, bjj_dlog_table* table);" in h
    assert "int bjj_dlog_table_info(const bjj_dlog_table* table, int* baby_bits, uint64_t* entries, uint64_t* table_bytes);" in h
    assert "int bjj_dlog_table_check(bjj_ctx* ctx, const bjj_dlog_table* table, uint64_t* n_bad);" in h
    assert "int bjj_dlog_table_base(const bjj_dlog_table* table, uint8_t* out_xy);" in h
    assert "int bjj_dlog_max_range_bits(const bjj_dlog_table* table);" in h
    assert ("int bjj_dlog(bjj_ctx* ctx, const bjj_dlog_table* table, const uint8_t* pts_xy, size_t n, int range_bits, "
            "uint64_t* out_m, uint8_t* ok);") in h
    assert ("int bjj_dlog_dev(bjj_ctx* ctx, const bjj_dlog_table* table, const void* d_pts_xy, size_t n, int range_bits, "
            "void* d_out_m, void* d_ok, void* stream);") in h


def test_header_is_plain_c11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "bjj_hip_dlog.h"\n'
                   "int use(bjj_ctx* c, const uint8_t* p, uint64_t* m, uint8_t* ok) {\n"
                   "  bjj_dlog_table* t = 0;\n  uint64_t entries = 0, bytes = 0, bad = 0;\n  int b = 0;\n  uint8_t xy[64];\n"
                   "  int rc = bjj_dlog_table_create(c, p, 0, &t) + bjj_dlog_table_info(t, &b, &entries, &bytes)\n"
                   "         + bjj_dlog_table_check(c, t, &bad) + bjj_dlog_table_base(t, xy) + bjj_dlog_max_range_bits(t);\n"
                   "  rc += bjj_dlog(c, t, p, 0, 32, m, ok) + bjj_dlog_dev(c, t, p, 0, 32, m, ok, 0);\n"
                   "  return rc + bjj_dlog_table_free(c, t) + (ok[0] == BJJ_DLOG_FOUND) + (ok[0] == BJJ_DLOG_OFF_CURVE)\n"
                   "       + (ok[0] == BJJ_DLOG_NOT_IN_RANGE) + BJJ_DLOG_MAX_GIANT_BITS;\n}\n")
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "use.o")],
                   check=True)


def test_library_exports_and_binding():
    lib = os.path.join(ROOT, "babyjubjub-rs_amd", "csrc", "libbjj_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    for name in FUNCTIONS:
        assert name in syms, "libbjj_hip.so does not export %s" % name
    from babyjubjub_rs_amd import _lib
    assert sorted(_lib.DLOG_SYMBOLS) == FUNCTIONS
    assert (_lib.BJJ_DLOG_NOT_IN_RANGE, _lib.BJJ_DLOG_FOUND, _lib.BJJ_DLOG_OFF_CURVE, _lib.BJJ_DLOG_MAX_GIANT_BITS) == (0, 1, 2, 16)
    assert not set(_lib.DLOG_SYMBOLS) & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.EXT_SYMBOLS) | set(_lib.BASES_SYMBOLS) | set(_lib.SIGNER_SYMBOLS)
                                         | set(_lib.SIGNER_SET_SYMBOLS))
    loaded = _lib.load()
    for name in _lib.DLOG_SYMBOLS:
        assert getattr(loaded, name).argtypes is not None
    import babyjubjub_rs_amd as bjj
    assert all(hasattr(bjj.Context, m) for m in ("dlog_table", "dlog", "dlog_dev", "elgamal_decrypt"))
    assert all(hasattr(bjj.DlogTable, m) for m in ("dlog", "check", "info", "close", "base", "max_range_bits"))


def test_the_other_headers_did_not_move():
    from babyjubjub_rs_amd import _lib
    assert set(declared(os.path.join(INCLUDE, "bjj_hip.h"))) == set(_lib.EXPORTED_SYMBOLS)
    assert set(declared(os.path.join(INCLUDE, "bjj_hip_bases.h"))) == set(_lib.BASES_SYMBOLS)
    assert set(declared(os.path.join(INCLUDE, "bjj_hip_signer.h"))) == set(_lib.SIGNER_SYMBOLS)
    assert set(declared(os.path.join(INCLUDE, "bjj_hip_signer_set.h"))) == set(_lib.SIGNER_SET_SYMBOLS)
    older = _lib.EXPORTED_SYMBOLS + _lib.EXT_SYMBOLS + _lib.BASES_SYMBOLS + _lib.SIGNER_SYMBOLS + _lib.SIGNER_SET_SYMBOLS
    assert not any("dlog" in n for n in older)


def test_bad_arguments_are_rejected_without_a_device():
    """every check below returns before the library touches a device or dereferences a table: the context is NULL (the same
    calls with a live context, a NULL table and a bad range_bits are in tests/test_gpu_dlog.py)"""
    from babyjubjub_rs_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 64)()
    m = (ctypes.c_uint8 * 32)(*([0xEE] * 32))
    ok = (ctypes.c_uint8 * 16)(*([0xEE] * 16))
    fake = ctypes.c_void_p(0x1230)
    out = ctypes.c_void_p(0x77)
    bad = ctypes.c_uint64(7)
    assert lib.bjj_dlog_table_create(None, buf, 0, ctypes.byref(out)) == _lib.BJJ_E_INVALID
    assert b"ctx is NULL" in lib.bjj_last_error() and out.value == 0x77
    assert lib.bjj_dlog_table_create(None, None, 8, ctypes.byref(out)) == _lib.BJJ_E_INVALID and out.value == 0x77
    assert lib.bjj_dlog_table_free(None, fake) == _lib.BJJ_E_INVALID
    assert lib.bjj_dlog_table_check(None, fake, ctypes.byref(bad)) == _lib.BJJ_E_INVALID and bad.value == 7
    assert lib.bjj_dlog_table_info(None, None, None, None) == _lib.BJJ_E_INVALID
    assert lib.bjj_dlog_table_base(None, buf) == _lib.BJJ_E_INVALID and bytes(buf) == bytes(64)
    assert lib.bjj_dlog_max_range_bits(None) == -1
    for n in (0, 1):
        for rb in (0, 16, 46):
            assert lib.bjj_dlog(None, fake, buf, n, rb, m, ok) == _lib.BJJ_E_INVALID
            assert b"ctx is NULL" in lib.bjj_last_error()
            assert lib.bjj_dlog_dev(None, fake, buf, n, rb, m, ok, None) == _lib.BJJ_E_INVALID
            assert lib.bjj_dlog(None, None, buf, n, rb, m, ok) == _lib.BJJ_E_INVALID
            assert lib.bjj_dlog_dev(None, None, buf, n, rb, m, ok, None) == _lib.BJJ_E_INVALID
    assert bytes(ok) == b"\xee" * 16 and bytes(m) == b"\xee" * 32
