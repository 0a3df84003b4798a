// DEBUG HARNESS (tests only): the dispatcher of tests/devfuzz/field_ops.hpp -- the shipped field layer, square root and codec
// items on raw limbs or words -- built by g++ with the bound assertions of csrc/fr.hpp live (the BJJ_ASSERTs of fr_sub,
// fr_sub8, fr_sub_lazy, fr_sub8_of_lazy and the operand checks of fr_mul).  tests/test_field_ops_host.py checks it against
// plain integers; tests/test_gpu_field_ops.py compares the device build with it bit for bit.  Not a fallback, not linked into
// libbjj_hip.so.
#define BJJ_DEBUG_BOUNDS 1
#include <stddef.h>
#include <stdint.h>
#include "../../babyjubjub-rs_amd/csrc/bjj_device.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
#include "../devfuzz/field_ops.hpp"
using namespace bjj;
static const Consts K = BJJ_CONSTS_INIT;

// a: n records of field_words(op, 0) words, b: n records of field_words(op, 1) (may be null when 0), out: n of field_words(op, 2)
extern "C" int emul_field_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  if (op < 0 || op >= FO_NOPS || (field_words(op, 1) && !b) || !a || !out) return -1;
  const size_t wa = field_words(op, 0), wb = field_words(op, 1), wo = field_words(op, 2);
  for (size_t i = 0; i < n; i++) field_op(op, a + i * wa, b + i * wb, out + i * wo, K);
  return 0;
}
extern "C" int emul_field_words(int op, int which) {
  return (op < 0 || op >= FO_NOPS || which < 0 || which > 2) ? -1 : field_words(op, which);
}
