// DEBUG HARNESS (tests only): the dispatcher of tests/devfuzz/hash_ops.hpp -- the shipped Poseidon permutation in both forms of
// its partial rounds, one full round, and the DLEQ challenge in both forms, on raw limbs -- built by g++ with the bound
// assertions live: the operand and sum check of fr_dot3, the BJJ_ASSERT of fr_dot2_add, the operand checks of fr_mul and the
// assertions of csrc/fr.hpp.  tests/test_hash_ops_host.py checks it against plain integers; tests/test_gpu_hash_ops.py compares
// the device build with it bit for bit.  Not a fallback, not linked into libbjj_hip.so.
#define BJJ_DEBUG_BOUNDS 1
#define BJJ_PNIELS_LAYOUT 0
#include <stddef.h>
#include <stdint.h>
#include "../../babyjubjub-rs_amd/csrc/dleq.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
#include "../devfuzz/hash_ops.hpp"
using namespace bjj;
static const Consts K = BJJ_CONSTS_INIT;

// in: n records of hash_words(op, 0) words, out: n records of hash_words(op, 1)
extern "C" int emul_hash_op(int op, const uint32_t* in, uint32_t* out, size_t n) {
  if (op < 0 || op >= HO_NOPS || !in || !out) return -1;
  const size_t wi = hash_words(op, 0), wo = hash_words(op, 1);
  for (size_t i = 0; i < n; i++) hash_op(op, in + i * wi, out + i * wo, K);
  return 0;
}
extern "C" int emul_hash_words(int op, int which) {
  return (op < 0 || op >= HO_NOPS || which < 0 || which > 1) ? -1 : hash_words(op, which);
}
// 1: BJJ_ASSERT is assert and assert is live in this build (what makes a broken lazy bound abort the process)
extern "C" int emul_hash_bounds_live(void) {
#if defined(BJJ_DEBUG_BOUNDS) && !defined(NDEBUG)
  int live = 0;
  BJJ_ASSERT((live = 1) != 0);
  return live;
#else
  return 0;
#endif
}
