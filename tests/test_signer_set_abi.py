"""include/bjj_hip_signer_set.h without a GPU: it parses, it is plain C11, the library exports the eight functions it declares, the
binding knows them, what is pinned to the other headers did not move, and the argument checks that need no device answer
BJJ_E_INVALID."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "bjj_hip_signer_set.h")
FUNCTIONS = sorted(["bjj_signer_set_create", "bjj_signer_set_free", "bjj_signer_set_info", "bjj_signer_set_check",
                    "bjj_eddsa_verify_set", "bjj_eddsa_verify_set_dev", "bjj_schnorr_verify_set", "bjj_schnorr_verify_set_dev"])


def declared(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(bjj_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_the_eight_functions():
    assert declared(HEADER) == FUNCTIONS
    h = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    h = re.sub(r"\s+([,)])", r"\1", " ".join(h.split()))
    assert '#include "bjj_hip_signer.h"' in h
    assert "typedef struct bjj_signer_set bjj_signer_set;" in h and "#define BJJ_VERIFY_BAD_SIGNER 3" in h
    assert ("int bjj_signer_set_create(bjj_ctx* ctx, const uint8_t* pks_xy, size_t k, int window_bits, bjj_signer_set** out, "
            "int64_t* out_first_off_curve);") in h
    assert "int bjj_signer_set_free(bjj_ctx* ctx, bjj_signer_set* set);" in h
    assert ("int bjj_signer_set_info(const bjj_signer_set* set, uint64_t* n_signers, int* window_bits, int* n_windows, "
            "uint64_t* table_bytes);") in h
    assert "int bjj_signer_set_check(bjj_ctx* ctx, const bjj_signer_set* set, uint64_t* n_bad);" in h
    for scheme in ("eddsa", "schnorr"):
        assert ("int bjj_%s_verify_set(bjj_ctx* ctx, const bjj_signer_set* set, const uint32_t* signer_idx, const uint8_t* r_xy, "
                "const uint8_t* s, const uint8_t* msg, size_t n, uint8_t* ok);" % scheme) in h
        assert ("int bjj_%s_verify_set_dev(bjj_ctx* ctx, const bjj_signer_set* set, const void* d_signer_idx, const void* d_r_xy, "
                "const void* d_s, const void* d_msg, size_t n, void* d_ok, void* stream);" % scheme) in h


def test_header_is_plain_c11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "bjj_hip_signer_set.h"\n'
                   "int use(bjj_ctx* c, const uint8_t* p, const uint32_t* ix, uint8_t* ok) {\n"
                   "  bjj_signer_set* t = 0;\n  int64_t first = 0;\n  uint64_t k = 0, bytes = 0, bad = 0;\n  int w = 0, nw = 0;\n"
                   "  int rc = bjj_signer_set_create(c, p, 1, 0, &t, &first) + bjj_signer_set_info(t, &k, &w, &nw, &bytes)\n"
                   "         + bjj_signer_set_check(c, t, &bad);\n"
                   "  rc += bjj_eddsa_verify_set(c, t, ix, p, p, p, 0, ok) + bjj_eddsa_verify_set_dev(c, t, ix, p, p, p, 0, ok, 0)\n"
                   "      + bjj_schnorr_verify_set(c, t, ix, p, p, p, 0, ok) + bjj_schnorr_verify_set_dev(c, t, ix, p, p, p, 0, ok, 0);\n"
                   "  return rc + bjj_signer_set_free(c, t) + (ok[0] == BJJ_VERIFY_BAD_SIGNER);\n}\n")
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "use.o")],
                   check=True)


def test_library_exports_and_binding():
    lib = os.path.join(ROOT, "babyjubjub-rs_amd", "csrc", "libbjj_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    for name in FUNCTIONS:
        assert name in syms, "libbjj_hip.so does not export %s" % name
    from babyjubjub_rs_amd import _lib
    assert sorted(_lib.SIGNER_SET_SYMBOLS) == FUNCTIONS and _lib.BJJ_VERIFY_BAD_SIGNER == 3
    assert not set(_lib.SIGNER_SET_SYMBOLS) & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.EXT_SYMBOLS) | set(_lib.BASES_SYMBOLS) | set(_lib.SIGNER_SYMBOLS))
    loaded = _lib.load()
    for name in _lib.SIGNER_SET_SYMBOLS:
        assert getattr(loaded, name).argtypes is not None
    import babyjubjub_rs_amd as bjj
    assert all(hasattr(bjj.Context, m) for m in ("signer_set", "eddsa_verify_set_dev", "schnorr_verify_set_dev"))
    assert all(hasattr(bjj.SignerSet, m) for m in ("verify", "verify_schnorr", "check", "info", "close"))


def test_the_other_headers_did_not_move():
    from babyjubjub_rs_amd import _lib
    assert set(declared(os.path.join(INCLUDE, "bjj_hip.h"))) == set(_lib.EXPORTED_SYMBOLS)
    assert set(declared(os.path.join(INCLUDE, "bjj_hip_bases.h"))) == set(_lib.BASES_SYMBOLS)
    assert set(declared(os.path.join(INCLUDE, "bjj_hip_signer.h"))) == set(_lib.SIGNER_SYMBOLS)
    older = _lib.EXPORTED_SYMBOLS + _lib.EXT_SYMBOLS + _lib.BASES_SYMBOLS + _lib.SIGNER_SYMBOLS
    assert not any("signer_set" in n or "verify_set" in n for n in older)


def test_null_arguments_are_rejected_without_a_device():
    """every check below returns before the library touches a device or dereferences a context"""
    from babyjubjub_rs_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 64)()
    ok = (ctypes.c_uint8 * 16)(*([0xEE] * 16))
    fake = ctypes.c_void_p(0x1230)
    out, first = ctypes.c_void_p(0x77), ctypes.c_int64(42)
    bad = ctypes.c_uint64(7)
    assert lib.bjj_signer_set_create(None, buf, 1, 0, ctypes.byref(out), ctypes.byref(first)) == _lib.BJJ_E_INVALID
    assert b"ctx is NULL" in lib.bjj_last_error() and out.value == 0x77 and first.value == 42
    assert lib.bjj_signer_set_free(None, fake) == _lib.BJJ_E_INVALID
    assert lib.bjj_signer_set_check(None, fake, ctypes.byref(bad)) == _lib.BJJ_E_INVALID and bad.value == 7
    assert lib.bjj_signer_set_info(None, None, None, None, None) == _lib.BJJ_E_INVALID
    for scheme in ("eddsa", "schnorr"):
        host, dev = getattr(lib, "bjj_%s_verify_set" % scheme), getattr(lib, "bjj_%s_verify_set_dev" % scheme)
        for n in (0, 1):
            assert host(None, fake, buf, buf, buf, buf, n, ok) == _lib.BJJ_E_INVALID
            assert b"ctx is NULL" in lib.bjj_last_error()
            assert dev(None, fake, buf, buf, buf, buf, n, ok, None) == _lib.BJJ_E_INVALID
            assert host(None, None, buf, buf, buf, buf, n, ok) == _lib.BJJ_E_INVALID
            assert dev(None, None, buf, buf, buf, buf, n, ok, None) == _lib.BJJ_E_INVALID
    assert bytes(ok) == b"\xee" * 16
