// DEBUG HARNESS (tests only): the dispatcher of tests/devfuzz/curve_ops.hpp -- the shipped group law, conversions, per-lane
// table, ladder and fixed-table items on raw limbs -- built by g++ with the bound assertions of csrc/fr.hpp live (the BJJ_ASSERTs
// of fr_sub, fr_sub8, fr_sub_lazy, fr_sub8_of_lazy and the operand checks of fr_mul), once per per-lane table layout
// (-DBJJ_PNIELS_LAYOUT=0 / 1).  tests/test_curve_ops_host.py checks it against plain integers; tests/test_gpu_curve_ops.py
// compares the device build with it bit for bit.  Not a fallback, not linked into libbjj_hip.so.
#define BJJ_DEBUG_BOUNDS 1
#include <stddef.h>
#include <stdint.h>
#include "../../babyjubjub-rs_amd/csrc/bjj_device.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
#include "../devfuzz/curve_ops.hpp"
using namespace bjj;
static const Consts K = BJJ_CONSTS_INIT;

// a: n records of curve_words(op, 0) words, b: n of curve_words(op, 1) (may be null when 0), out: n of curve_words(op, 2);
// the per-item scratch (curve_words(op, 3) words) is one 16-byte aligned block here, reused item after item
extern "C" int emul_curve_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  if (op < 0 || op >= CO_NOPS || (curve_words(op, 1) && !b) || !a || !out) return -1;
  const size_t wa = curve_words(op, 0), wb = curve_words(op, 1), wo = curve_words(op, 2);
  alignas(16) uint32_t scr[CO_FT_WORDS > VB_TABLE_WORDS_MAX ? CO_FT_WORDS : VB_TABLE_WORDS_MAX];
  for (size_t i = 0; i < n; i++) {
    for (size_t k = 0; k < sizeof(scr) / sizeof(scr[0]); k++) scr[k] = 0xEEEEEEEEu;
    curve_op(op, a + i * wa, b + i * wb, out + i * wo, scr, K);
  }
  return 0;
}
extern "C" int emul_curve_words(int op, int which) {
  return (op < 0 || op >= CO_NOPS || which < 0 || which > 3) ? -1 : curve_words(op, which);
}
extern "C" int emul_curve_layout() { return BJJ_PNIELS_LAYOUT; }
