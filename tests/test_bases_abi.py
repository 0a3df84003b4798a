"""include/bjj_hip_bases.h without a GPU: it parses, it is plain C11, the library exports every function it declares, the binding
knows them, what is pinned to bjj_hip.h did not move, and the argument checks that need no device answer BJJ_E_INVALID."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "bjj_hip_bases.h")
FUNCTIONS = ["bjj_base_check", "bjj_base_create", "bjj_base_free", "bjj_base_info", "bjj_mul_bases", "bjj_mul_bases_dev"]


def header_functions():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(bjj_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_the_six_functions():
    assert header_functions() == FUNCTIONS
    h = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    h = re.sub(r"\s+([,)])", r"\1", " ".join(h.split()))
    assert "typedef struct bjj_base bjj_base;" in h and "#define BJJ_MAX_BASES 8" in h and '#include "bjj_hip.h"' in h
    assert "int bjj_base_create(bjj_ctx* ctx, const uint8_t* point_xy, int window_bits, bjj_base** out);" in h
    assert ("int bjj_mul_bases(bjj_ctx* ctx, const bjj_base* const* bases, int t, const uint8_t* const* scalars, size_t n, "
            "uint8_t* out_xy);") in h
    assert ("int bjj_mul_bases_dev(bjj_ctx* ctx, const bjj_base* const* bases, int t, const void* const* d_scalars, size_t n, "
            "void* d_out_xy, void* stream);") in h


def test_header_is_plain_c11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "bjj_hip_bases.h"\n'
                   "int use(bjj_ctx* c, const uint8_t* p, uint8_t* out) {\n"
                   "  bjj_base* b = 0; const bjj_base* bs[BJJ_MAX_BASES] = {0}; const uint8_t* sc[1] = {p}; const void* d[1] = {p};\n"
                   "  int w, nw; uint64_t tb, bad;\n"
                   "  return bjj_base_create(c, p, 0, &b) + bjj_base_info(b, &w, &nw, &tb) + bjj_base_check(c, b, &bad)\n"
                   "       + bjj_mul_bases(c, bs, 1, sc, 0, out) + bjj_mul_bases_dev(c, bs, 1, d, 0, out, 0) + bjj_base_free(c, b);\n}\n")
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_library_exports_and_binding():
    lib = os.path.join(ROOT, "babyjubjub-rs_amd", "csrc", "libbjj_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    for name in header_functions():
        assert name in syms, "libbjj_hip.so does not export %s" % name
    from babyjubjub_rs_amd import _lib
    assert sorted(_lib.BASES_SYMBOLS) == FUNCTIONS and _lib.BJJ_MAX_BASES == 8
    assert not set(_lib.BASES_SYMBOLS) & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.EXT_SYMBOLS))
    loaded = _lib.load()
    for name in _lib.BASES_SYMBOLS:
        assert getattr(loaded, name).argtypes is not None
    import babyjubjub_rs_amd as bjj
    assert all(hasattr(bjj.Context, m) for m in ("base", "mul_bases", "mul_bases_dev"))
    assert all(hasattr(bjj.FixedBase, m) for m in ("close", "info", "check", "mul"))


def test_bjj_hip_h_did_not_move():
    from babyjubjub_rs_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bjj_hip.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(bjj_[a-z0-9_]+)\s*\(", txt))
    assert names == set(_lib.EXPORTED_SYMBOLS) and not any(n.startswith("bjj_base_") or "mul_bases" in n for n in names)


def test_null_arguments_are_rejected_without_a_device():
    """every check below returns before the library touches a device or dereferences a context"""
    from babyjubjub_rs_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p(0x1234)
    pt = (ctypes.c_uint8 * 64)()
    assert lib.bjj_base_create(None, pt, 0, ctypes.byref(h)) == _lib.BJJ_E_INVALID and h.value == 0x1234
    assert b"ctx is NULL" in lib.bjj_last_error()
    assert lib.bjj_base_free(None, None) == _lib.BJJ_E_INVALID
    assert lib.bjj_base_info(None, None, None, None) == _lib.BJJ_E_INVALID
    bad = ctypes.c_uint64(7)
    assert lib.bjj_base_check(None, None, ctypes.byref(bad)) == _lib.BJJ_E_INVALID and bad.value == 7
    bases, arrs = (ctypes.c_void_p * 9)(), (ctypes.c_void_p * 9)()
    out = (ctypes.c_uint8 * 64)(*([0xEE] * 64))
    for t in (0, 1, 8, 9):
        assert lib.bjj_mul_bases(None, bases, t, arrs, 1, out) == _lib.BJJ_E_INVALID
        assert lib.bjj_mul_bases_dev(None, bases, t, arrs, 1, out, None) == _lib.BJJ_E_INVALID
    assert bytes(out) == b"\xee" * 64
