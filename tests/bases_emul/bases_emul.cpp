// DEBUG HARNESS (tests only): the table code and the per-item body of bjj_mul_bases (csrc/bases.hpp, what k_bases.hip launches)
// on the CPU with limb / value-bound assertions -- a stand-alone program, so that it also runs under AddressSanitizer and
// UndefinedBehaviorSanitizer as it is (tests/test_bases_host.py builds it twice).  Not linked into libbjj_hip.so.
//
// stdin:  "P <x> <y>" (a generator of the whole group, hex), then "S <count>" and <count> scalars (hex, < 2^256).
// Tables: 0..2 = P at W = 4, 5, 12;  3 = the order-2 point (0, -1) at W = 4;  4 = B8 at W = 4 as a CONTEXT's table (fixed_nwin
// windows, scalar mod l: what a NULL entry of `bases` selects).
// stdout: "check <table> <bad>"      the induction check over every slot (0 expected)
//         "corrupt <table> <bad>"    the same with one bit of one entry flipped (> 0 expected)
//         "anchor <table> <bad>"     the same against the WRONG base point (> 0 expected)
//         "entry <table> <mismatches>"  chain-built entries against the per-entry ladder base_table_entry (sampled; 0 expected)
//         "r <case> <i> <x> <y>"     result i of a case; the cases are listed in CASES below, scalar of base j = S[(i + 7 j) % count]
#define BJJ_DEBUG_BOUNDS 1
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../babyjubjub-rs_amd/csrc/bases.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
#include "../emul_support.hpp"

static void ext_out(const Ext& p, u32 x[8], u32 y[8]) {  // single-item affine epilogue
  Fr zi = fr_inv(p.Z);
  Fr c1 = fr_mul(zi, fr_one_plain()), c2 = fr_mul(zi, K.FINV_PLAIN);
  constexpr u32 R1[NL] = {BJJ_N0, BJJ_N1, BJJ_N2, BJJ_N3, BJJ_N4, BJJ_N5, BJJ_N6, BJJ_N7, BJJ_N8};
  fr_to_words(fr_cond_sub_kr(fr_mul(p.X, c2), R1), x);
  fr_to_words(fr_cond_sub_kr(fr_mul(p.Y, c1), R1), y);
}

struct Case { const char* name; int t; int tbl[3]; };
static const Case CASES[] = {
    {"p4", 1, {0}}, {"p5", 1, {1}}, {"p12", 1, {2}}, {"two4", 1, {3}}, {"b8", 1, {4}},
    {"p4+p12", 2, {0, 2}}, {"b8+p5", 2, {4, 1}}, {"two4+p4", 2, {3, 0}}, {"p12+b8", 2, {2, 4}},
    {"p12+b8+two4", 3, {2, 4, 3}}, {"p4+p4+p5", 3, {0, 0, 1}},
};

int main() {
  Words pxy[2];
  if (!read_tag("P") || !read_words(pxy, 2)) { fprintf(stderr, "bad P line\n"); return 2; }
  size_t count = 0;
  if (!read_header("S", count) || count == 0) { fprintf(stderr, "bad S line\n"); return 2; }
  std::vector<Words> S(count);
  if (!read_words(S.data(), count)) { fprintf(stderr, "bad scalar\n"); return 2; }

  const Fr Px = fr_to_mont_words(pxy[0].w), Py = fr_to_mont_words(pxy[1].w);
  if (!ref_on_curve(Px, Py, K)) { fprintf(stderr, "P is not on the curve\n"); return 2; }
  Words m1;   // r - 1: the y of the order-2 point (0, -1), through the conversion the kernels use (coordinates < 2r)
  parse_hex("30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000000", m1);
  const Fr zero = fr_zero(), minus_one = fr_to_mont_words(m1.w);
  HostTable T[5];
  T[0].build(Px, Py, 4, false, 3);
  T[1].build(Px, Py, 5, false, 8);
  T[2].build(Px, Py, 12, false, 64);
  T[3].build(zero, minus_one, 4, false, 4);
  T[4].build(K.B8X, K.B8Y, 4, true, 8);
  for (int i = 0; i < 5; i++) {
    printf("check %d %llu\n", i, T[i].check());
    // the chain builder against the independent per-entry definition (every entry of the small tables, a sample of W = 12)
    printf("entry %d %llu\n", i, T[i].entry_mismatches(T[i].W >= 12 ? 97 : 1));
  }
  printf("anchor 0 %llu\n", T[0].check(K.B8X, K.B8Y));
  printf("anchor 3 %llu\n", T[3].check(Px, Py));
  {
    HostTable& c = T[1];
    u32* word = c.t() + (fixed_stride(c.W) * 3 + 5) * NIELS_WORDS + 11;
    *word ^= 4u;
    printf("corrupt 1 %llu\n", c.check());
    *word ^= 4u;
    printf("check 1 %llu\n", c.check());
  }

  for (const Case& c : CASES) {
    BasesArgs A;
    memset(&A, 0, sizeof(A));
    A.t = c.t;
    for (int j = 0; j < c.t; j++) A.b[j] = T[c.tbl[j]].desc();
    for (size_t i = 0; i < count; i++) {
      const Ext p = mul_bases_item(A, GatherPerLane{A.b[0].table},
                                   [&](int j, u32 raw[8]) { memcpy(raw, S[(i + 7 * (size_t)j) % count].w, 32); }, K);
      Words x, y;
      ext_out(p, x.w, y.w);
      printf("r %s %zu ", c.name, i);
      print_hex(x.w); printf(" "); print_hex(y.w); printf("\n");
    }
  }
  return 0;
}
