// DEBUG HARNESS (tests only): runs the per-item body of bjj_k_elgamal_encrypt (csrc/elgamal.hpp) on the CPU with limb / value-bound
// assertions, one "lane" after the other, over fixed-base tables built in host memory: the window bases by base_table_entry, the
// entries between them by fixed_table_chain, a sample of them compared with base_table_entry again.  The affine epilogue is the
// plain one (fr_inv per point) in place of the workgroup-wide inversion; an output record is written the moment the body hands
// its point over, so a call whose outputs ARE its add arrays behaves as the kernel does.  Not linked into libbjj_hip.so.
#define BJJ_DEBUG_BOUNDS 1
#include <string.h>
#include <memory>
#include <vector>
#include "../../babyjubjub-rs_amd/csrc/elgamal.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
#include "../emul_support.hpp"

static std::vector<std::unique_ptr<HostTable>> g_tables;

extern "C" {
int eg_emul_nwin_m(int W) { return elgamal_nwin_m(W); }
// The table of the point xy (64 bytes; any curve point) at width W, or with xy == NULL the table of B8 as a CONTEXT holds it.  Returns
// its handle, -1 for a point off the curve, -2 when a sampled entry differs from base_table_entry.
int eg_emul_table(const uint8_t* xy, int W) {
  Fr bx = K.B8X, by = K.B8Y;
  if (xy) {
    alignas(16) u32 w[16];
    memcpy(w, xy, 64);
    bx = fr_to_mont_words(w); by = fr_to_mont_words(w + 8);
    if (!ref_on_curve(bx, by, K)) return -1;
  }
  std::unique_ptr<HostTable> t(new HostTable);
  t->build(bx, by, W, !xy, 1024);
  if (t->entry_mismatches(t->slots() > 400 ? t->slots() / 97 : 1)) return -2;
  g_tables.push_back(std::move(t));
  return (int)g_tables.size() - 1;
}
void eg_emul_free_tables() { g_tables.clear(); }
// the signed digits digit_stream / digit_next give for the first nwin windows of m at width W (what the m-chain walks)
void eg_emul_digits(uint64_t m, int W, int nwin, long long* digits) {
  const u32 sc[8] = {(u32)m, (u32)(m >> 32), 0u, 0u, 0u, 0u, 0u, 0u};
  DigitStream ds = digit_stream(sc, W);
  for (int j = 0; j < nwin; j++) {
    bool neg;
    const size_t slot = digit_next(ds, neg);
    const long long d = (long long)(slot - (size_t)j * fixed_stride(W));
    digits[j] = neg ? -d : d;
  }
}
// out_c1 / out_c2 / ok as bjj_elgamal_encrypt writes them.  m, add_c1 / add_c2 (both or neither) and ok may be NULL; in_place: the
// add records are copied into the output arrays and read from there.  Returns 0, -1 for bad arguments, -3 for a zero Z.
int eg_emul_encrypt(int g, int pk, const uint64_t* m, const uint8_t* r, const uint8_t* add_c1, const uint8_t* add_c2, size_t n, int in_place,
                    uint8_t* out_c1, uint8_t* out_c2, uint8_t* ok) {
  if (g < 0 || pk < 0 || (size_t)g >= g_tables.size() || (size_t)pk >= g_tables.size() || !add_c1 != !add_c2 || g_tables[pk]->ctx_b8) return -1;
  if (in_place && !add_c1) return -1;
  HostTable& tg = *g_tables[g];
  HostTable& tp = *g_tables[pk];
  Aligned<uint8_t> in_r(n * 32 + 1), a1(n * 64 + 1), a2(n * 64 + 1), o1(n * 64 + 1), o2(n * 64 + 1);
  Aligned<uint64_t> in_m(n + 1);
  if (n) memcpy(in_r.p(), r, n * 32);
  if (n && m) memcpy(in_m.p(), m, n * 8);
  uint8_t* const s1 = in_place ? o1.p() : a1.p();
  uint8_t* const s2 = in_place ? o2.p() : a2.p();
  if (n && add_c1) { memcpy(s1, add_c1, n * 64); memcpy(s2, add_c2, n * 64); }
  ElgamalArgs A;
  memset(&A, 0, sizeof(A));
  A.b[0] = EgChain{tg.t(), tg.W, tg.nwin, tg.ctx_b8 ? EG_R_MOD_L : EG_R_MOD_ORDER};
  A.b[1] = EgChain{A.b[0].table, tg.W, elgamal_nwin_m(tg.W), EG_M};
  A.b[2] = EgChain{tp.t(), tp.W, tp.nwin, EG_R_MOD_ORDER};
  A.m = m ? in_m.p() : nullptr; A.r = in_r.p();
  A.add_c1 = add_c1 ? s1 : nullptr; A.add_c2 = add_c1 ? s2 : nullptr;
  int bad = 0;
  for (size_t i = 0; i < n; i++) {
    const auto sink = [&](int which, const Ext& p, bool on) {
      uint8_t* const o = (which ? o2.p() : o1.p()) + i * 64;
      if (!on) { memset(o, 0, 64); return; }
      if (fr_is_zero(p.Z)) { bad = -3; return; }   // the Z of a sum of curve points is never 0
      store_affine(o, p);
    };
    const bool on = add_c1 ? elgamal_item<true>(A, GatherPerLane{A.b[0].table}, i, sink, K)
                           : elgamal_item<false>(A, GatherPerLane{A.b[0].table}, i, sink, K);
    if (ok) ok[i] = on ? 1 : 2;
    if (bad) return bad;
  }
  if (n) { memcpy(out_c1, o1.p(), n * 64); memcpy(out_c2, o2.p(), n * 64); }
  return 0;
}
}
