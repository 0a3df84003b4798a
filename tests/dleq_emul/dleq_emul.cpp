// DEBUG HARNESS (tests only): runs the per-item bodies of csrc/dleq.hpp on the CPU with limb / value-bound assertions, one "lane"
// after the other: pair_item (bjj_k_mul_pair), dleq_verify_item (bjj_k_dleq_verify) over fixed-base tables built in host memory
// with a gather that knows their extents, and the prover's chain as bjj_dleq_prove launches it -- dleq_nonce_item, then the bodies of
// the launchers it borrows (cs_item over the recoded sk', mul_bases_item, var_base_fast), then dleq_respond_item.  The affine epilogue
// is the plain one (fr_inv per point) in place of the workgroup-wide inversion.  The per-lane tables use this unit's layout (raw).
// Not linked into libbjj_hip.so.
#define BJJ_DEBUG_BOUNDS 1
#define BJJ_PNIELS_LAYOUT 0
#include <string.h>
#include <memory>
#include <vector>
#include "../../babyjubjub-rs_amd/csrc/dleq.hpp"
#include "../../babyjubjub-rs_amd/csrc/common_scalar.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
#include "../emul_support.hpp"

static std::vector<std::unique_ptr<HostTable>> g_tables;

static void copy_in(Aligned<uint8_t>& dst, const uint8_t* src, size_t bytes) {
  dst = Aligned<uint8_t>(bytes + 1);
  if (bytes && src) memcpy(dst.p(), src, bytes);
}
static Fr tag_of(const uint8_t* tag) {
  alignas(16) u32 w[8];
  memcpy(w, tag, 32);
  return fr_to_mont_words(w);
}

extern "C" {
// The table of the point xy (64 bytes; any curve point) at width W, or with xy == NULL the table of B8 as a CONTEXT holds it.  Returns
// its handle, -1 for a point off the curve, -2 when a sampled entry differs from base_table_entry.
int dq_emul_table(const uint8_t* xy, int W) {
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
void dq_emul_free_tables() { g_tables.clear(); }

// out / ok as bjj_mul_pair writes them; add may be NULL.  Returns 0, -3 for a zero Z.
int dq_emul_pair(const uint8_t* p, const uint8_t* a, const uint8_t* q, const uint8_t* b, const uint8_t* add, size_t n, uint8_t* out, uint8_t* ok) {
  Aligned<uint8_t> ip, ia, iq, ib, iadd;
  copy_in(ip, p, n * 64); copy_in(ia, a, n * 32); copy_in(iq, q, n * 64); copy_in(ib, b, n * 32); copy_in(iadd, add, n * 64);
  Aligned<u32> tbl(2 * VB_TABLE_WORDS);
  const PairArgs A = {ip.p(), iq.p(), ia.p(), ib.p(), add ? iadd.p() : nullptr};
  for (size_t i = 0; i < n; i++) {
    Ext e;
    if (pair_item(A, i, tbl.p(), e, K)) {
      if (fr_is_zero(e.Z)) return -3;   // the Z of a sum of curve points is never 0
      store_affine(out + i * 64, e);
      ok[i] = 1;
    } else {
      memset(out + i * 64, 0, 64);
      ok[i] = 2;
    }
  }
  return 0;
}

// ok as bjj_dleq_verify writes it.  g: a table handle (the context's B8 table or a caller's), pk: a caller's table.  Returns 0, -1 for
// bad arguments.
int dq_emul_verify(int g, int pk, const uint8_t* tag, const uint8_t* c1, const uint8_t* d, const uint8_t* a, const uint8_t* b, const uint8_t* z,
                   size_t n, uint8_t* ok) {
  if (g < 0 || pk < 0 || (size_t)g >= g_tables.size() || (size_t)pk >= g_tables.size() || g_tables[pk]->ctx_b8 || !tag) return -1;
  HostTable& tg = *g_tables[g];
  HostTable& tp = *g_tables[pk];
  Aligned<uint8_t> ic1, id, ia, ib, iz;
  copy_in(ic1, c1, n * 64); copy_in(id, d, n * 64); copy_in(ia, a, n * 64); copy_in(ib, b, n * 64); copy_in(iz, z, n * 32);
  Aligned<u32> tbl(2 * VB_TABLE_WORDS);
  DleqVerifyArgs A;
  memset(&A, 0, sizeof(A));
  A.b[0] = tg.desc(); A.b[1] = tp.desc();
  A.tag = tag_of(tag);
  A.c1 = ic1.p(); A.d = id.p(); A.a = ia.p(); A.b_xy = ib.p(); A.z = iz.p();
  const GatherBounded<2> gather = {tg.t(), {{tg.t(), tg.slots()}, {tp.t(), tp.slots()}}};
  for (size_t i = 0; i < n; i++) ok[i] = (uint8_t)dleq_verify_item(A, gather, i, tbl.p(), K);
  return 0;
}

// d / a / b / z / ok as bjj_dleq_prove writes them: the chain of bjj_dleq.inc, item by item.  Returns 0, -1 for bad arguments, -3 for a zero Z.
int dq_emul_prove(int g, const uint8_t* sk, const uint8_t* tag, const uint8_t* c1, const uint8_t* w, size_t n, uint8_t* d, uint8_t* a, uint8_t* b,
                  uint8_t* z, uint8_t* ok) {
  if (g < 0 || (size_t)g >= g_tables.size() || !sk || !tag) return -1;
  HostTable& tg = *g_tables[g];
  Aligned<uint8_t> ic1, iw, od(n * 64 + 1, 0xEE), oa(n * 64 + 1, 0xEE), ob(n * 64 + 1, 0xEE), oz(n * 32 + 1, 0xEE);
  copy_in(ic1, c1, n * 64); copy_in(iw, w, n * 32);
  DleqRespondArgs R;
  memset(&R, 0, sizeof(R));
  alignas(16) u32 raw[8];
  memcpy(raw, sk, 32);
  scalar_mod_l(raw, R.sk, K);                                   // dleq_prove_check
  CsDigits D;
  if (cs_recode(R.sk, false, CS_FORM_NAF, &D, K) < 0) return -1;
  R.tag = tag_of(tag);
  R.c1 = ic1.p(); R.d = od.p(); R.a = oa.p(); R.b_xy = ob.p(); R.z = oz.p();
  BasesArgs B;
  memset(&B, 0, sizeof(B));
  B.t = 1; B.b[0] = tg.desc();
  Aligned<u32> tbl(2 * VB_TABLE_WORDS);
  const GatherBounded<1> gather = {tg.t(), {{tg.t(), tg.slots()}}};
  for (size_t i = 0; i < n; i++) {
    dleq_nonce_item(iw.p(), i, oz.p(), K);                      // launch 1: w' where z will stand
    Ext e;
    const bool on = cs_item<false, false>(ic1.p(), nullptr, i, D, nullptr, e, K);   // launch 2: D = sk' C1 (bjj_k_mul_common)
    ok[i] = on ? 1 : 2;
    if (on) { if (fr_is_zero(e.Z)) return -3; store_affine(od.p() + i * 64, e); } else memset(od.p() + i * 64, 0, 64);
    e = mul_bases_item(B, gather, [&](int, u32 sc[8]) { load_w8(oz.p() + i * 32, sc); }, K);   // launch 3: A = w' G (bjj_k_mul_bases)
    if (fr_is_zero(e.Z)) return -3;
    store_affine(oa.p() + i * 64, e);
    if (on) {                                                   // launch 4: B = w' C1 (K2 skips an off-curve point)
      Fr x, y;
      dleq_load_xy(ic1.p(), i, x, y);
      u32 sc[8];
      load_w8(oz.p() + i * 32, sc);
      e = var_base_fast(x, y, sc, tbl.p(), K);
      if (fr_is_zero(e.Z)) return -3;
      store_affine(ob.p() + i * 64, e);
    }
    dleq_respond_item(R, i, on, K);                             // launch 5
  }
  if (n) { memcpy(d, od.p(), n * 64); memcpy(a, oa.p(), n * 64); memcpy(b, ob.p(), n * 64); memcpy(z, oz.p(), n * 32); }
  return 0;
}
}
