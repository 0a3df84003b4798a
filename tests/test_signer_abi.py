"""include/bjj_hip_signer.h without a GPU: it parses, it is plain C11, the library exports the four functions it declares, the
binding knows them, what is pinned to bjj_hip.h and bjj_hip_bases.h did not move, and the argument checks that need no device
answer BJJ_E_INVALID."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "bjj_hip_signer.h")
FUNCTIONS = ["bjj_eddsa_verify_signer", "bjj_eddsa_verify_signer_dev", "bjj_schnorr_verify_signer", "bjj_schnorr_verify_signer_dev"]


def declared(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(bjj_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_the_four_functions():
    assert declared(HEADER) == FUNCTIONS
    h = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    h = re.sub(r"\s+([,)])", r"\1", " ".join(h.split()))
    assert '#include "bjj_hip_bases.h"' in h
    for scheme in ("eddsa", "schnorr"):
        assert ("int bjj_%s_verify_signer(bjj_ctx* ctx, const bjj_base* signer, const uint8_t* r_xy, const uint8_t* s, "
                "const uint8_t* msg, size_t n, uint8_t* ok);" % scheme) in h
        assert ("int bjj_%s_verify_signer_dev(bjj_ctx* ctx, const bjj_base* signer, const void* d_r_xy, const void* d_s, "
                "const void* d_msg, size_t n, void* d_ok, void* stream);" % scheme) in h


def test_header_is_plain_c11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "bjj_hip_signer.h"\n'
                   "int use(bjj_ctx* c, const bjj_base* b, const uint8_t* p, uint8_t* ok) {\n"
                   "  return bjj_eddsa_verify_signer(c, b, p, p, p, 0, ok) + bjj_eddsa_verify_signer_dev(c, b, p, p, p, 0, ok, 0)\n"
                   "       + bjj_schnorr_verify_signer(c, b, p, p, p, 0, ok) + bjj_schnorr_verify_signer_dev(c, b, p, p, p, 0, ok, 0);\n}\n")
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_library_exports_and_binding():
    lib = os.path.join(ROOT, "babyjubjub-rs_amd", "csrc", "libbjj_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    for name in FUNCTIONS:
        assert name in syms, "libbjj_hip.so does not export %s" % name
    from babyjubjub_rs_amd import _lib
    assert sorted(_lib.SIGNER_SYMBOLS) == FUNCTIONS
    assert not set(_lib.SIGNER_SYMBOLS) & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.EXT_SYMBOLS) | set(_lib.BASES_SYMBOLS))
    loaded = _lib.load()
    for name in _lib.SIGNER_SYMBOLS:
        assert getattr(loaded, name).argtypes is not None
    import babyjubjub_rs_amd as bjj
    assert all(hasattr(bjj.Context, m) for m in ("eddsa_verify_signer", "schnorr_verify_signer", "eddsa_verify_signer_dev",
                                                 "schnorr_verify_signer_dev"))
    assert all(hasattr(bjj.FixedBase, m) for m in ("verify", "verify_schnorr"))


def test_the_other_headers_did_not_move():
    from babyjubjub_rs_amd import _lib
    assert set(declared(os.path.join(ROOT, "include", "bjj_hip.h"))) == set(_lib.EXPORTED_SYMBOLS)
    assert set(declared(os.path.join(ROOT, "include", "bjj_hip_bases.h"))) == set(_lib.BASES_SYMBOLS)
    assert not any("verify_signer" in n for n in _lib.EXPORTED_SYMBOLS + _lib.EXT_SYMBOLS + _lib.BASES_SYMBOLS)


def test_null_arguments_are_rejected_without_a_device():
    """every check below returns before the library touches a device or dereferences a context"""
    from babyjubjub_rs_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 64)()
    ok = (ctypes.c_uint8 * 16)(*([0xEE] * 16))
    fake = ctypes.c_void_p(0x1230)
    for scheme in ("eddsa", "schnorr"):
        host, dev = getattr(lib, "bjj_%s_verify_signer" % scheme), getattr(lib, "bjj_%s_verify_signer_dev" % scheme)
        for n in (0, 1):
            assert host(None, fake, buf, buf, buf, n, ok) == _lib.BJJ_E_INVALID
            assert b"ctx is NULL" in lib.bjj_last_error()
            assert dev(None, fake, buf, buf, buf, n, ok, None) == _lib.BJJ_E_INVALID
            assert host(None, None, buf, buf, buf, n, ok) == _lib.BJJ_E_INVALID
            assert dev(None, None, buf, buf, buf, n, ok, None) == _lib.BJJ_E_INVALID
    assert bytes(ok) == b"\xee" * 16
