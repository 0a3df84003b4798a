// DEBUG HARNESS (tests only): the per-item body and the verdict step of bjj_k_verify_signer (csrc/signer.hpp, what k_signer.hip
// launches) on the CPU with limb / value-bound assertions -- a stand-alone program, so that it also runs under AddressSanitizer
// and UndefinedBehaviorSanitizer as it is (tests/test_signer_host.py builds it twice).  Not linked into libbjj_hip.so.
//
// stdin:  "P <x> <y>"                the signer's point (hex, on the curve)
//         "I <count>" and <count> lines "<rx> <ry> <s> <msg>" (hex, any 256-bit values): the items
//         "Z <count>" and <count> non-zero field elements: the projective scalings of the verdict cases
//         "V <count>" and <count> lines "<lx> <ly> <tx> <ty> <rx> <ry>": curve points l, t (reference curve, affine) and any R
// Tables: the signer's at W = 4 and W = 5 (mod 8l, base_nwin windows), B8 at W = 4 as a CONTEXT's table (mod l, fixed_nwin windows).
// stdout: "check <table> <bad>"      the induction check of the three tables (0 expected)
//         "e <W> <i> <verdict>"      EdDSA verdict of item i over the signer's table of width W
//         "s <W> <i> <verdict>"      Schnorr verdict
//         "v <i> <k> <verdict>"      signer_verdict of case i with T scaled by Z[k] and L by Z[(k + 1) % count]; k = count: unscaled
#define BJJ_DEBUG_BOUNDS 1
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../babyjubjub-rs_amd/csrc/signer.hpp"
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
static bool read_words(Words* out, int count) {
  char tok[80];
  for (int i = 0; i < count; i++)
    if (scanf("%79s", tok) != 1 || !parse_hex(tok, out[i])) return false;
  return true;
}
static bool read_header(const char* name, size_t& count) {
  char tok[80];
  return scanf("%79s %zu", tok, &count) == 2 && !strcmp(tok, name) && count <= 100000;
}

struct Table {
  int W = 0, nwin = 0;
  bool ctx_b8 = false;   // the context's B8 table: fixed_nwin windows, scalars mod l
  Fr bx, by;
  std::vector<u32> tv, bv;
  u32* t() { return (u32*)(((uintptr_t)tv.data() + 15) & ~(uintptr_t)15); }
  u32* b() { return (u32*)(((uintptr_t)bv.data() + 15) & ~(uintptr_t)15); }
  void build(const Fr& x, const Fr& y, int W_, bool ctx_b8_, u32 chain) {
    W = W_; ctx_b8 = ctx_b8_; bx = x; by = y;
    nwin = ctx_b8 ? fixed_nwin(W) : base_nwin(W);
    const size_t stride = fixed_stride(W);
    tv.assign(stride * (size_t)nwin * NIELS_WORDS + 4, 0);
    bv.assign((size_t)nwin * NIELS_WORDS + 4, 0);
    for (int j = 0; j < nwin; j++) store_niels(b() + (size_t)j * NIELS_WORDS, base_table_entry(bx, by, 1u, j, W, K));
    for (int j = 0; j < nwin; j++)
      for (size_t k0 = 0; k0 < stride; k0 += chain) {
        const u32 cnt = (u32)(stride - k0 < chain ? stride - k0 : chain);
        fixed_table_chain(t(), load_niels(b() + (size_t)j * NIELS_WORDS), (size_t)j * stride + k0, (u32)k0, cnt, W, K);
      }
  }
  unsigned long long check() {
    unsigned long long bad = 0;
    for (int j = 0; j < nwin; j++)
      for (size_t k = 0; k < fixed_stride(W); k++) bad += (unsigned long long)base_table_check_slot(t(), b(), j, (u32)k, W, nwin, bx, by, K);
    return bad;
  }
  BaseDesc desc() {
    BaseDesc d;
    memset(&d, 0, sizeof(d));
    d.table = t(); d.W = W; d.nwin = nwin; d.mod_l = ctx_b8 ? 1 : 0;
    return d;
  }
};

// (x, y) affine on the reference curve -> the internal curve's projective form scaled by z: what a table chain hands to the verdict
static Ext scaled(const Words& x, const Words& y, const Fr* z) {
  Ext e = ext_from_ref_affine(fr_to_mont_words(x.w), fr_to_mont_words(y.w), K);
  e.T = fr_zero();
  if (z) { e.X = fr_mul(e.X, *z); e.Y = fr_mul(e.Y, *z); e.Z = *z; }
  return e;
}

int main() {
  char tok[80];
  Words pxy[2];
  if (scanf("%79s", tok) != 1 || strcmp(tok, "P") || !read_words(pxy, 2)) { fprintf(stderr, "bad P line\n"); return 2; }
  size_t ni = 0, nz = 0, nv = 0;
  if (!read_header("I", ni)) { fprintf(stderr, "bad I line\n"); return 2; }
  std::vector<Words> items(4 * ni + 1);
  if (!read_words(items.data(), (int)(4 * ni))) { fprintf(stderr, "bad item\n"); return 2; }
  if (!read_header("Z", nz) || nz == 0) { fprintf(stderr, "bad Z line\n"); return 2; }
  std::vector<Words> zs(nz);
  if (!read_words(zs.data(), (int)nz)) { fprintf(stderr, "bad scaling\n"); return 2; }
  if (!read_header("V", nv)) { fprintf(stderr, "bad V line\n"); return 2; }
  std::vector<Words> vc(6 * nv + 1);
  if (!read_words(vc.data(), (int)(6 * nv))) { fprintf(stderr, "bad verdict case\n"); return 2; }

  u32 xy[16];
  memcpy(xy, pxy[0].w, 32); memcpy(xy + 8, pxy[1].w, 32);
  const SignerPoint pk = signer_point(xy);
  if (!ref_on_curve(pk.x, pk.y, K)) { fprintf(stderr, "P is not on the curve\n"); return 2; }
  Table T[3];
  T[0].build(pk.x, pk.y, 4, false, 3);
  T[1].build(pk.x, pk.y, 5, false, 8);
  T[2].build(K.B8X, K.B8Y, 4, true, 8);
  for (int i = 0; i < 3; i++) printf("check %d %llu\n", i, T[i].check());

  for (int t = 0; t < 2; t++) {
    SignerArgs A;
    A.T = T[t].desc(); A.L = T[2].desc(); A.pk = pk;
    for (size_t i = 0; i < ni; i++) {
      const Words* it = &items[4 * i];   // rx, ry are read as ONE 64-byte record
      alignas(16) u32 r[16];
      memcpy(r, it[0].w, 32); memcpy(r + 8, it[1].w, 32);
      printf("e %d %zu %d\n", T[t].W, i, verify_signer_item<false>(A, GatherPerLane{A.T.table}, r, it[2].w, it[3].w, K));
      printf("s %d %zu %d\n", T[t].W, i, verify_signer_item<true>(A, GatherPerLane{A.T.table}, r, it[2].w, it[3].w, K));
    }
  }

  std::vector<Fr> z(nz);
  for (size_t k = 0; k < nz; k++) z[k] = fr_to_mont_words(zs[k].w);
  for (size_t i = 0; i < nv; i++) {
    const Words* c = &vc[6 * i];
    const Fr rx = fr_to_mont_words(c[4].w), ry = fr_to_mont_words(c[5].w);
    for (size_t k = 0; k <= nz; k++) {
      const Ext L = scaled(c[0], c[1], k < nz ? &z[(k + 1) % nz] : nullptr);
      const Ext Tp = scaled(c[2], c[3], k < nz ? &z[k] : nullptr);
      printf("v %zu %zu %d\n", i, k, signer_verdict(L, Tp, rx, ry, K));
    }
  }
  return 0;
}
