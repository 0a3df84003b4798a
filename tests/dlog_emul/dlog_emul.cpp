// DEBUG HARNESS (tests only): the per-lane bodies of the discrete-logarithm kernels (csrc/dlog.hpp, what k_dlog.hip launches) on the
// CPU with limb / value-bound assertions and a slot policy that refuses a slot outside the table -- a stand-alone program, so that
// it also runs under AddressSanitizer and UndefinedBehaviorSanitizer as it is (tests/test_dlog_host.py builds it twice).  Not linked
// into libbjj_hip.so.  Where the kernels take 1 / Z from the workgroup inversion, this program takes it from fr_inv.  A launch that
// takes more rounds than a lane can need -- every step refused at every slot -- aborts: on the device such a lane would spin.
//
// stdin:  "G <x> <y>"                      the base point (hex, on the curve; coordinates >= r are reduced)
//         "T <baby_bits> <chain>"          the table: built thread by thread, `chain` consecutive j per thread
//         "R <count>" and <count> values   the range_bits to search with
//         "I <count>" and <count> lines "<x> <y>" (hex): the items
// Everything runs twice: with the kernels' 32-bit tags and with 3-bit tags, which force false tag hits.
// stdout: "small <0|1>"                    8 G = identity
//         "base <x> <y>"                   the canonical record dlog_setup leaves
//         "check <tag_bits> <bad> <occupied>"            the check bodies over the untouched table
//         "flip <tag_bits> <tag|j> <bad>"                the same with one bit of one occupied slot flipped
//         "slots <tag_bits> <slot>:<j + 1> ..."          the occupied slots of the table as built
//         "r <tag_bits> <range_bits> <i> <ok> <m> <refused>"   item i searched in one go (m in hex), and the tag hits of this item
//                                                        that confirmation refused
//         "s <tag_bits> <range_bits> <i> <ok> <m> <launches> <refused>"  the same search cut into launches of 3 giant steps, how
//                                                        many of them walked the item (a decided item is passed by), and the
//                                                        refused hits over all of them
//         "rejected <tag_bits> <count>"                  tag hits that confirmation refused, over all "r" searches
#define BJJ_DEBUG_BOUNDS 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../babyjubjub-rs_amd/csrc/dlog.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
#include "../emul_support.hpp"

static void print_hex_short(const u32 w[8]) {   // without leading zeros
  int top = 7;
  while (top > 0 && w[top] == 0) top--;
  printf("%x", w[top]);
  for (int i = top - 1; i >= 0; i--) printf("%08x", w[i]);
}

// the table as the kernels see it, with every index checked
struct SlotsBounded {
  u64* p;
  size_t n;
  u64 load(u32 i) const {
    if (i >= n) { fprintf(stderr, "slot out of bounds: %u of %zu\n", i, n); abort(); }
    return p[i];
  }
  bool cas(u32 i, u64 v) const {
    if (i >= n) { fprintf(stderr, "slot out of bounds: %u of %zu\n", i, n); abort(); }
    if (p[i] != 0) return false;
    p[i] = v;
    return true;
  }
};

static int g_b;
alignas(16) static u32 g_params[DLOG_PARAM_WORDS];

template <int TB>
static void build(std::vector<u64>& tv, u32 chain) {
  tv.assign((size_t)dlog_slots(g_b), 0);
  const SlotsBounded S = {tv.data(), tv.size()};
  const u32 mask = (u32)(tv.size() - 1);
  const Niels g = load_niels(g_params + DLOG_P_G);
  const u64 entries = dlog_entries(g_b), threads = (entries + chain - 1) / chain;
  for (u64 t = 0; t < threads + 2; t++) {   // two threads past the end, as a launch rounded up to the workgroup has
    const u64 j0 = t * chain;
    Ext acc = dlog_mul_small(g, j0 < entries ? j0 : 0, g_b + 1);
    for (u32 k = 0; k < chain; k++) {
      if (j0 + k < entries && !dlog_insert<TB>(S, mask, (u32)(j0 + k), acc, fr_inv(acc.Z))) { fprintf(stderr, "table full\n"); abort(); }
      acc = ext_madd(acc, g);
    }
  }
}
template <int TB>
static unsigned long long check(std::vector<u64>& tv, unsigned long long* occupied) {
  const SlotsBounded S = {tv.data(), tv.size()};
  const u32 mask = (u32)(tv.size() - 1);
  unsigned long long bad = 0, occ = 0;
  for (u64 j = 0; j < dlog_entries(g_b); j++) bad += (unsigned long long)dlog_check_entry<TB>(S, mask, g_params, (u32)j, g_b, K);
  for (size_t i = 0; i < tv.size(); i++) {
    u32 o;
    bad += (unsigned long long)dlog_check_slot(tv[i], g_b, o);
    occ += o;
  }
  if (occupied) *occupied = occ;
  return bad + (occ != dlog_entries(g_b) ? 1 : 0);
}
// one launch of bjj_k_dlog_search for one lane: giant steps s0 .. s1 - 1; ok is the lane's byte of the ok array
template <int TB>
static void launch(std::vector<u64>& tv, const Words* rec, int range_bits, u32 s0, u32 s1, bool last, u64& m, int& ok,
                   unsigned long long& rejected, unsigned long long* walked = nullptr) {
  if (!dlog_resumes(s0, s0 ? (u32)ok : 0u)) return;
  if (walked) (*walked)++;
  const SlotsBounded S = {tv.data(), tv.size()};
  const u32 mask = (u32)(tv.size() - 1);
  const Niels ns = load_niels(g_params + DLOG_P_NEG_STRIDE);
  alignas(16) u32 r[16];
  memcpy(r, rec[0].w, 32); memcpy(r + 8, rec[1].w, 32);
  DlogLane L;
  dlog_start(L, r, g_params, s0, K);
  const unsigned long long cap = ((unsigned long long)(s1 - s0) + 1) * (tv.size() + 1);
  unsigned long long rounds = 0;
  for (;;) {
    while (L.st == DL_SEARCH) {
      if (++rounds > cap) { fprintf(stderr, "step count cap: a lane that does not advance\n"); abort(); }
      dlog_step<TB>(L, fr_inv(L.Q.Z), ns, S, mask, s1);
    }
    if (L.st != DL_PENDING) break;
    rejected += dlog_confirm(L, load_niels(g_params + DLOG_P_G), g_b, range_bits) ? 1 : 0;
  }
  ok = (int)dlog_ok_byte(L, last); m = L.m;
}
template <int TB>
static void run(u32 chain, const std::vector<int>& ranges, const std::vector<Words>& items) {
  std::vector<u64> tv;
  build<TB>(tv, chain);
  unsigned long long occ = 0;
  const unsigned long long bad = check<TB>(tv, &occ);
  printf("check %d %llu %llu\n", TB, bad, occ);
  printf("slots %d", TB);
  for (size_t i = 0; i < tv.size(); i++)
    if (tv[i] != 0) printf(" %zu:%u", i, (u32)tv[i]);
  printf("\n");
  size_t victim = 0;
  while (victim < tv.size() && tv[victim] == 0) victim++;
  if (victim == tv.size()) abort();
  tv[victim] ^= (u64)1 << 32; printf("flip %d tag %llu\n", TB, check<TB>(tv, nullptr)); tv[victim] ^= (u64)1 << 32;
  tv[victim] ^= (u64)1;       printf("flip %d j %llu\n", TB, check<TB>(tv, nullptr));   tv[victim] ^= (u64)1;
  unsigned long long rejected = 0, unused = 0;
  const size_t ni = items.size() / 2;
  for (int range_bits : ranges) {
    const u32 nsteps = dlog_steps(g_b, range_bits);
    for (size_t i = 0; i < ni; i++) {
      u64 m = 0; int ok = 0;
      const unsigned long long before = rejected;
      launch<TB>(tv, &items[2 * i], range_bits, 0, nsteps, true, m, ok, rejected);
      printf("r %d %d %zu %d %llx %llu\n", TB, range_bits, i, ok, (unsigned long long)m, rejected - before);
      unsigned long long walked = 0;
      unused = 0;
      for (u32 s0 = 0; s0 < nsteps; s0 += 3)
        launch<TB>(tv, &items[2 * i], range_bits, s0, s0 + 3 < nsteps ? s0 + 3 : nsteps, s0 + 3 >= nsteps, m, ok, unused, &walked);
      printf("s %d %d %zu %d %llx %llu %llu\n", TB, range_bits, i, ok, (unsigned long long)m, walked, unused);
    }
  }
  printf("rejected %d %llu\n", TB, rejected);
}

int main() {
  Words gxy[2];
  unsigned chain = 0;
  size_t nr = 0, ni = 0;
  if (!read_tag("G") || !read_words(gxy, 2)) { fprintf(stderr, "bad G line\n"); return 2; }
  if (!read_tag("T") || scanf("%d %u", &g_b, &chain) != 2 || g_b < BJJ_DLOG_MIN_BABY_BITS || g_b > 12 || chain < 1) { fprintf(stderr, "bad T line\n"); return 2; }
  if (!read_header("R", nr) || nr > 16) { fprintf(stderr, "bad R line\n"); return 2; }
  std::vector<int> ranges(nr);
  for (size_t i = 0; i < nr; i++)
    if (scanf("%d", &ranges[i]) != 1 || ranges[i] < 1 || ranges[i] > dlog_max_range_bits(g_b)) { fprintf(stderr, "bad range\n"); return 2; }
  if (!read_header("I", ni)) { fprintf(stderr, "bad I line\n"); return 2; }
  std::vector<Words> items(2 * ni + 1);
  if (!read_words(items.data(), 2 * ni)) { fprintf(stderr, "bad item\n"); return 2; }
  items.resize(2 * ni);

  const Fr bx = fr_to_mont_words(gxy[0].w), by = fr_to_mont_words(gxy[1].w);
  if (!ref_on_curve(bx, by, K)) { fprintf(stderr, "the base is not on the curve\n"); return 2; }
  dlog_setup(g_params, bx, by, g_b, K);
  printf("small %u\n", g_params[DLOG_P_SMALL]);
  printf("base "); print_hex_short(g_params + DLOG_P_XY); printf(" "); print_hex_short(g_params + DLOG_P_XY + 8); printf("\n");
  if (g_params[DLOG_P_SMALL]) return 0;
  run<32>(chain, ranges, items);
  run<3>(chain, ranges, items);
  return 0;
}
