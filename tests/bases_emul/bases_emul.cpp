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
#include <string>
#include <vector>
#include "../../babyjubjub-rs_amd/csrc/bases.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
using namespace bjj;
static const Consts K = {
    BJJ_K_A, BJJ_K_D, BJJ_K_F, BJJ_K_FINV_PLAIN, BJJ_K_FINV, BJJ_K_L_R1, BJJ_K_L_R2, BJJ_K_DP, BJJ_K_D2P, BJJ_K_DPINV, BJJ_K_B8X, BJJ_K_B8Y, BJJ_K_TS_G, BJJ_K_HALFQ,
    BJJ_K_ORDER, BJJ_K_ORDER2, BJJ_K_ORDER4, BJJ_K_L, BJJ_K_L2, BJJ_K_L4,
    BJJ_K_POSEIDON_CF, BJJ_K_POSEIDON_KP, BJJ_K_POSEIDON_SP, BJJ_K_POSEIDON_AL, BJJ_K_POSEIDON_M, BJJ_K_POSEIDON_CAB,
    BJJ_K_TS_NEG, BJJ_K_TS_HALF, BJJ_K_TS_HASH};

struct Words { alignas(16) u32 w[8]; };
static bool parse_hex(const char* s, Words& out) {
  const size_t len = strlen(s);
  if (len == 0 || len > 64) return false;
  memset(out.w, 0, sizeof(out.w));
  for (size_t i = 0; i < len; i++) {
    const char c = s[len - 1 - i];
    const int v = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
    if (v < 0) return false;
    out.w[i / 8] |= (u32)v << (4 * (i % 8));
  }
  return true;
}
static void print_hex(const u32 w[8]) {
  for (int i = 7; i >= 0; i--) printf("%08x", w[i]);
}
static void ext_out(const Ext& p, u32 x[8], u32 y[8]) {  // single-item affine epilogue
  Fr zi = fr_inv(p.Z);
  Fr c1 = fr_mul(zi, fr_one_plain()), c2 = fr_mul(zi, K.FINV_PLAIN);
  constexpr u32 R1[NL] = {BJJ_N0, BJJ_N1, BJJ_N2, BJJ_N3, BJJ_N4, BJJ_N5, BJJ_N6, BJJ_N7, BJJ_N8};
  fr_to_words(fr_cond_sub_kr(fr_mul(p.X, c2), R1), x);
  fr_to_words(fr_cond_sub_kr(fr_mul(p.Y, c1), R1), y);
}

struct Table {
  int W = 0, nwin = 0;
  bool ctx_b8 = false;   // the context's B8 table: fixed_nwin windows, scalars mod l
  Fr bx, by;
  std::vector<u32> tv, bv;
  u32* t() { return (u32*)(((uintptr_t)tv.data() + 15) & ~(uintptr_t)15); }
  u32* b() { return (u32*)(((uintptr_t)bv.data() + 15) & ~(uintptr_t)15); }
  size_t slots() const { return fixed_stride(W) * (size_t)nwin; }
  void build(const Fr& x, const Fr& y, int W_, bool ctx_b8_, u32 chain) {
    W = W_; ctx_b8 = ctx_b8_; bx = x; by = y;
    nwin = ctx_b8 ? fixed_nwin(W) : base_nwin(W);
    const size_t stride = fixed_stride(W);
    tv.assign(slots() * NIELS_WORDS + 4, 0);
    bv.assign((size_t)nwin * NIELS_WORDS + 4, 0);
    for (int j = 0; j < nwin; j++) store_niels(b() + (size_t)j * NIELS_WORDS, base_table_entry(bx, by, 1u, j, W, K));
    for (int j = 0; j < nwin; j++)
      for (size_t k0 = 0; k0 < stride; k0 += chain) {
        const u32 cnt = (u32)(stride - k0 < chain ? stride - k0 : chain);
        fixed_table_chain(t(), load_niels(b() + (size_t)j * NIELS_WORDS), (size_t)j * stride + k0, (u32)k0, cnt, W, K);
      }
  }
  unsigned long long check(const Fr& ax, const Fr& ay) {
    unsigned long long bad = 0;
    const size_t stride = fixed_stride(W);
    for (int j = 0; j < nwin; j++)
      for (size_t k = 0; k < stride; k++) bad += (unsigned long long)base_table_check_slot(t(), b(), j, (u32)k, W, nwin, ax, ay, K);
    return bad;
  }
};

struct Case { const char* name; int t; int tbl[3]; };
static const Case CASES[] = {
    {"p4", 1, {0}}, {"p5", 1, {1}}, {"p12", 1, {2}}, {"two4", 1, {3}}, {"b8", 1, {4}},
    {"p4+p12", 2, {0, 2}}, {"b8+p5", 2, {4, 1}}, {"two4+p4", 2, {3, 0}}, {"p12+b8", 2, {2, 4}},
    {"p12+b8+two4", 3, {2, 4, 3}}, {"p4+p4+p5", 3, {0, 0, 1}},
};

int main() {
  char tok[80], sx[80], sy[80];
  Words px, py;
  if (scanf("%79s %79s %79s", tok, sx, sy) != 3 || strcmp(tok, "P") || !parse_hex(sx, px) || !parse_hex(sy, py)) { fprintf(stderr, "bad P line\n"); return 2; }
  size_t count = 0;
  if (scanf("%79s %zu", tok, &count) != 2 || strcmp(tok, "S") || count == 0 || count > 100000) { fprintf(stderr, "bad S line\n"); return 2; }
  std::vector<Words> S(count);
  for (size_t i = 0; i < count; i++)
    if (scanf("%79s", sx) != 1 || !parse_hex(sx, S[i])) { fprintf(stderr, "bad scalar %zu\n", i); return 2; }

  const Fr Px = fr_to_mont_words(px.w), Py = fr_to_mont_words(py.w);
  if (!ref_on_curve(Px, Py, K)) { fprintf(stderr, "P is not on the curve\n"); return 2; }
  Words m1;   // r - 1: the y of the order-2 point (0, -1), through the conversion the kernels use (coordinates < 2r)
  parse_hex("30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000000", m1);
  const Fr zero = fr_zero(), minus_one = fr_to_mont_words(m1.w);
  Table T[5];
  T[0].build(Px, Py, 4, false, 3);
  T[1].build(Px, Py, 5, false, 8);
  T[2].build(Px, Py, 12, false, 64);
  T[3].build(zero, minus_one, 4, false, 4);
  T[4].build(K.B8X, K.B8Y, 4, true, 8);
  for (int i = 0; i < 5; i++) {
    printf("check %d %llu\n", i, T[i].check(T[i].bx, T[i].by));
    // the chain builder against the independent per-entry definition (every entry of the small tables, a sample of W = 12)
    unsigned long long mism = 0;
    const size_t stride = fixed_stride(T[i].W), step = T[i].W >= 12 ? 97 : 1;
    for (size_t s = 0; s < T[i].slots(); s += step) {
      const int j = (int)(s / stride);
      mism += !niels_limbs_equal(load_niels(T[i].t() + s * NIELS_WORDS), base_table_entry(T[i].bx, T[i].by, (u32)(s % stride), j, T[i].W, K, j == 0));
    }
    printf("entry %d %llu\n", i, mism);
  }
  printf("anchor 0 %llu\n", T[0].check(K.B8X, K.B8Y));
  printf("anchor 3 %llu\n", T[3].check(Px, Py));
  {
    Table& c = T[1];
    u32* word = c.t() + (fixed_stride(c.W) * 3 + 5) * NIELS_WORDS + 11;
    *word ^= 4u;
    printf("corrupt 1 %llu\n", c.check(c.bx, c.by));
    *word ^= 4u;
    printf("check 1 %llu\n", c.check(c.bx, c.by));
  }

  for (const Case& c : CASES) {
    BasesArgs A;
    memset(&A, 0, sizeof(A));
    A.t = c.t;
    for (int j = 0; j < c.t; j++) {
      Table& tb = T[c.tbl[j]];
      A.b[j].table = tb.t(); A.b[j].W = tb.W; A.b[j].nwin = tb.nwin; A.b[j].mod_l = tb.ctx_b8 ? 1 : 0;
    }
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
