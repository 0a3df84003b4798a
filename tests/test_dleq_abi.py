"""include/bjj_hip_dleq.h without a GPU: it declares the six functions and the three constants, it is plain C11, the library exports
the six, the binding knows them and keeps them apart from every other symbol list, what is pinned to the older headers did not move,
and the argument-rejection table with a NULL context: every call is BJJ_E_INVALID before a device is touched, and writes nothing."""
import ctypes
import itertools
import os
import re
import subprocess

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "bjj_hip_dleq.h")
FUNCTIONS = sorted(["bjj_mul_pair", "bjj_mul_pair_dev", "bjj_dleq_verify", "bjj_dleq_verify_dev", "bjj_dleq_prove", "bjj_dleq_prove_dev"])


def declared(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(bjj_[a-z0-9_]+)\s*\(", txt)))


def test_header_declarations_equal_dleq_symbols():
    from babyjubjub_rs_amd import _lib
    assert declared(HEADER) == FUNCTIONS == sorted(_lib.DLEQ_SYMBOLS) and len(_lib.DLEQ_SYMBOLS) == 6
    raw = open(HEADER).read()
    h = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    h = re.sub(r"\s+([,)])", r"\1", " ".join(h.split()))
    assert '#include "bjj_hip.h"' in h and '#include "bjj_hip_bases.h"' in h
    assert "#define BJJ_DLEQ_REJECT 0" in h and "#define BJJ_DLEQ_OK 1" in h and "#define BJJ_DLEQ_OFF_CURVE 2" in h
    assert sorted(set(re.findall(r"#define (BJJ_DLEQ_[A-Z_]+)", h))) == ["BJJ_DLEQ_OFF_CURVE", "BJJ_DLEQ_OK", "BJJ_DLEQ_REJECT"]
    assert (_lib.BJJ_DLEQ_REJECT, _lib.BJJ_DLEQ_OK, _lib.BJJ_DLEQ_OFF_CURVE) == (0, 1, 2)
    assert ("int bjj_mul_pair(bjj_ctx* ctx, const uint8_t* p_xy, const uint8_t* a, const uint8_t* q_xy, const uint8_t* b, "
            "const uint8_t* add_xy, size_t n, uint8_t* out_xy, uint8_t* ok);") in h
    assert ("int bjj_mul_pair_dev(bjj_ctx* ctx, const void* d_p_xy, const void* d_a, const void* d_q_xy, const void* d_b, "
            "const void* d_add_xy, size_t n, void* d_out_xy, void* d_ok, void* stream);") in h
    assert ("int bjj_dleq_verify(bjj_ctx* ctx, const bjj_base* g, const bjj_base* pk, const uint8_t* tag, const uint8_t* c1_xy, "
            "const uint8_t* d_xy, const uint8_t* a_xy, const uint8_t* b_xy, const uint8_t* z, size_t n, uint8_t* ok);") in h
    assert ("int bjj_dleq_verify_dev(bjj_ctx* ctx, const bjj_base* g, const bjj_base* pk, const uint8_t* tag, const void* d_c1_xy, "
            "const void* d_d_xy, const void* d_a_xy, const void* d_b_xy, const void* d_z, size_t n, void* d_ok, void* stream);") in h
    assert ("int bjj_dleq_prove(bjj_ctx* ctx, const bjj_base* g, const uint8_t* sk, const uint8_t* tag, const uint8_t* c1_xy, "
            "const uint8_t* w, size_t n, uint8_t* d_xy, uint8_t* a_xy, uint8_t* b_xy, uint8_t* z, uint8_t* ok);") in h
    assert ("int bjj_dleq_prove_dev(bjj_ctx* ctx, const bjj_base* g, const uint8_t* sk, const uint8_t* tag, const void* d_c1_xy, "
            "const void* d_w, size_t n, void* d_d_xy, void* d_a_xy, void* d_b_xy, void* d_z, void* d_ok, void* stream);") in h
    # the words the contract asks for
    for words in ("NOT CONSTANT TIME", "bjj_mul_common", "bjj_set_signer_constant_time", "byte for byte", "mod 8l", "mod l", "a missing key",
                  "n == 0 is BJJ_OK", "A rejected call writes nothing", "before any device is touched", "no chunked pipeline",
                  "one scratch set per stream", "(0, 0)", "ONLY through tag", "bjj_in_subgroup", "order 2", "c is even", "must be canonical",
                  "16-byte aligned", "bjj_poseidon5"):
        assert words in raw, words


def test_header_is_plain_c11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "bjj_hip_dleq.h"\n'
                   "int use(bjj_ctx* c, const bjj_base* g, const bjj_base* pk, const uint8_t* in, uint8_t* out, uint8_t* ok) {\n"
                   "  int rc = bjj_mul_pair(c, in, in, in, in, 0, 0, out, ok);\n"
                   "  rc += bjj_mul_pair_dev(c, in, in, in, in, in, 0, out, ok, 0);\n"
                   "  rc += bjj_dleq_verify(c, g, pk, in, in, in, in, in, in, 0, ok);\n"
                   "  rc += bjj_dleq_verify_dev(c, 0, pk, in, in, in, in, in, in, 0, ok, 0);\n"
                   "  rc += bjj_dleq_prove(c, g, in, in, in, in, 0, out, out, out, out, ok);\n"
                   "  rc += bjj_dleq_prove_dev(c, 0, in, in, in, in, 0, out, out, out, out, ok, 0);\n"
                   "  return rc + (ok[0] == BJJ_DLEQ_OK) + (ok[0] == BJJ_DLEQ_OFF_CURVE) + (ok[0] == BJJ_DLEQ_REJECT);\n}\n")
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "use.o")],
                   check=True)


def test_library_exports_and_binding():
    lib = os.path.join(ROOT, "babyjubjub-rs_amd", "csrc", "libbjj_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    for name in FUNCTIONS:
        assert name in syms, "libbjj_hip.so does not export %s" % name
    from babyjubjub_rs_amd import _lib
    loaded = _lib.load()
    for name in _lib.DLEQ_SYMBOLS:
        assert getattr(loaded, name).argtypes is not None
    import babyjubjub_rs_amd as bjj
    assert all(hasattr(bjj.Context, m) for m in ("mul_pair", "mul_pair_dev", "dleq_verify", "dleq_verify_dev", "dleq_prove", "dleq_prove_dev",
                                                 "dleq_tag"))


def test_dleq_symbols_are_disjoint_from_every_other_list_and_the_older_headers_did_not_move():
    from babyjubjub_rs_amd import _lib
    lists = {k: v for k, v in vars(_lib).items() if k.endswith("_SYMBOLS") and k != "DLEQ_SYMBOLS"}
    assert sorted(lists) == sorted(["EXPORTED_SYMBOLS", "EXT_SYMBOLS", "BASES_SYMBOLS", "SIGNER_SYMBOLS", "SIGNER_SET_SYMBOLS", "DLOG_SYMBOLS",
                                    "POINT_SUM_SYMBOLS", "COMMON_SYMBOLS", "ELGAMAL_SYMBOLS"])
    for name, t in lists.items():
        assert not set(_lib.DLEQ_SYMBOLS) & set(t), name
    for header, names in (("bjj_hip.h", _lib.EXPORTED_SYMBOLS), ("bjj_hip_msm_batch.h", _lib.EXT_SYMBOLS), ("bjj_hip_bases.h", _lib.BASES_SYMBOLS),
                          ("bjj_hip_signer.h", _lib.SIGNER_SYMBOLS), ("bjj_hip_signer_set.h", _lib.SIGNER_SET_SYMBOLS),
                          ("bjj_hip_dlog.h", _lib.DLOG_SYMBOLS), ("bjj_hip_point_sum.h", _lib.POINT_SUM_SYMBOLS),
                          ("bjj_hip_common_scalar.h", _lib.COMMON_SYMBOLS), ("bjj_hip_elgamal.h", _lib.ELGAMAL_SYMBOLS)):
        assert set(declared(os.path.join(INCLUDE, header))) == set(names), header
    assert len(_lib.EXPORTED_SYMBOLS) == 71
    assert (len(_lib.EXT_SYMBOLS), len(_lib.BASES_SYMBOLS), len(_lib.SIGNER_SYMBOLS), len(_lib.SIGNER_SET_SYMBOLS), len(_lib.DLOG_SYMBOLS),
            len(_lib.POINT_SUM_SYMBOLS), len(_lib.COMMON_SYMBOLS), len(_lib.ELGAMAL_SYMBOLS)) == (2, 6, 4, 8, 8, 2, 6, 2)


def test_a_null_context_is_rejected_and_nothing_is_written():
    """the rejection table: every call below returns before the library touches a device or dereferences a handle or a buffer"""
    from babyjubjub_rs_amd import _lib
    lib = _lib.load()
    inp = (ctypes.c_uint8 * 128)(*([0x11] * 128))
    outs = [(ctypes.c_uint8 * 128)(*([0xEE] * 128)) for _ in range(5)]
    fake = ctypes.c_void_p(0x1230)
    calls = 0
    for n, g, pk, key, arr in itertools.product((0, 2), (None, fake), (None, fake), (None, inp), (None, inp)):
        o = [None if arr is None else x for x in outs]
        for rc in (lib.bjj_mul_pair(None, arr, arr, arr, arr, key, n, o[0], o[4]),
                   lib.bjj_mul_pair_dev(None, arr, arr, arr, arr, key, n, o[0], o[4], None),
                   lib.bjj_dleq_verify(None, g, pk, key, arr, arr, arr, arr, arr, n, o[4]),
                   lib.bjj_dleq_verify_dev(None, g, pk, key, arr, arr, arr, arr, arr, n, o[4], None),
                   lib.bjj_dleq_prove(None, g, key, key, arr, arr, n, o[0], o[1], o[2], o[3], o[4]),
                   lib.bjj_dleq_prove_dev(None, g, key, key, arr, arr, n, o[0], o[1], o[2], o[3], o[4], None)):
            assert rc == _lib.BJJ_E_INVALID
            assert b"ctx is NULL" in lib.bjj_last_error()
            calls += 1
    assert calls == 32 * 6
    assert all(bytes(x) == b"\xee" * 128 for x in outs) and bytes(inp) == b"\x11" * 128
