// DEBUG HARNESS (tests only): runs the bodies of csrc/common_scalar.hpp -- the host's recoding, the form rule, and the per-lane item
// of bjj_k_mul_common in both forms with its three epilogues -- on the CPU with limb / value-bound assertions, one "lane" after the
// other.  The lane's table lies between guard words that are checked after every item.  The affine epilogue is the plain one
// (fr_inv per item) in place of the workgroup-wide inversion.  Not linked into libbjj_hip.so.
#define BJJ_DEBUG_BOUNDS 1
#define BJJ_PNIELS_LAYOUT 1   // K2's packed per-lane table, as k_common_scalar.hip
#include <string.h>
#include <vector>
#include "../../babyjubjub-rs_amd/csrc/common_scalar.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
#include "../emul_support.hpp"

constexpr u32 GUARD = 0xdeadbeefu;
constexpr int GUARD_WORDS = 8;

static void plan(const uint8_t scalar[32], bool negate, int form, CsDigits* D) {
  u32 raw[8];
  memcpy(raw, scalar, 32);
  cs_recode(raw, negate, form, D, K);
}
// the item of lane i; returns the ok byte of the point epilogue (1 / 2), out = 64 bytes
template <bool TABLE, bool ADD>
static int item_point(const uint8_t* pts, const uint8_t* add, size_t i, const CsDigits& D, u32* tbl, uint8_t* out) {
  Ext p;
  if (!cs_item<TABLE, ADD>(pts, add, i, D, tbl, p, K)) { memset(out, 0, 64); return 2; }
  if (fr_is_zero(p.Z)) return -3;   // the Z of a sum of curve points is never 0
  store_affine(out, p);
  return 1;
}
template <bool TABLE>
static int item_subgroup(const uint8_t* pts, size_t i, const CsDigits& D, u32* tbl) {
  Ext p;
  if (!cs_item<TABLE, false>(pts, nullptr, i, D, tbl, p, K)) return 2;
  return cs_is_identity(p) ? 1 : 0;
}

extern "C" {
int cs_emul_max_digits() { return CS_MAX_DIGITS; }
// digits: CS_MAX_DIGITS + 1 signed bytes (the whole array as the kernel could index it); *top as the kernel gets it.  Returns the weight.
int cs_emul_recode(const uint8_t scalar[32], int negate, int form, signed char* digits, int* top) {
  CsDigits D;
  u32 raw[8];
  memcpy(raw, scalar, 32);
  const int weight = cs_recode(raw, negate != 0, form, &D, K);
  for (int i = 0; i <= CS_MAX_DIGITS; i++) digits[i] = (signed char)cs_digit(D, i);
  *top = D.top;
  return weight;
}
// the form the rule picks, and the two multiplication counts it compared
int cs_emul_choose(const uint8_t scalar[32], int* cost_naf, int* cost_table) {
  CsDigits D;
  u32 raw[8];
  memcpy(raw, scalar, 32);
  const int wn = cs_recode(raw, false, CS_FORM_NAF, &D, K), ww = cs_recode(raw, false, CS_FORM_TABLE, &D, K);
  *cost_naf = cs_cost_naf(wn);
  *cost_table = cs_cost_table(ww);
  return cs_choose_form(wn, ww);
}
// out[i] = add[i] +- scalar * pts[i] as bjj_mul_common writes it (add may be NULL); ok: n bytes.  Returns 0, -1 for a bad form, -2 when a
// lane wrote outside its table, -3 for a zero Z.
int cs_emul_mul(const uint8_t scalar[32], const uint8_t* pts, const uint8_t* add, int subtract, size_t n, int form, uint8_t* out, uint8_t* ok) {
  if (form != CS_FORM_NAF && form != CS_FORM_TABLE) return -1;
  CsDigits D;
  plan(scalar, subtract != 0, form, &D);
  Aligned<uint8_t> in_p(n * 64 + 1), in_a(n * 64 + 1);
  if (n) memcpy(in_p.p(), pts, n * 64);
  if (n && add) memcpy(in_a.p(), add, n * 64);
  Aligned<u32> table(VB_TABLE_WORDS + 2 * GUARD_WORDS);
  for (size_t i = 0; i < n; i++) {
    u32* t = table.p();
    for (int k = 0; k < VB_TABLE_WORDS + 2 * GUARD_WORDS; k++) t[k] = GUARD;
    u32* tbl = t + GUARD_WORDS;
    int r;
    if (form == CS_FORM_TABLE) r = add ? item_point<true, true>(in_p.p(), in_a.p(), i, D, tbl, out + i * 64) : item_point<true, false>(in_p.p(), nullptr, i, D, tbl, out + i * 64);
    else r = add ? item_point<false, true>(in_p.p(), in_a.p(), i, D, tbl, out + i * 64) : item_point<false, false>(in_p.p(), nullptr, i, D, tbl, out + i * 64);
    if (r < 0) return r;
    ok[i] = (uint8_t)r;
    for (int k = 0; k < GUARD_WORDS; k++) if (t[k] != GUARD || t[GUARD_WORDS + VB_TABLE_WORDS + k] != GUARD) return -2;
    if (form == CS_FORM_NAF) for (int k = 0; k < VB_TABLE_WORDS; k++) if (tbl[k] != GUARD) return -2;   // the table-free form has no table
  }
  return 0;
}
// ok[i] as bjj_in_subgroup writes it: the same item with the scalar l and the projective comparison
int cs_emul_subgroup(const uint8_t* pts, size_t n, int form, uint8_t* ok) {
  if (form != CS_FORM_NAF && form != CS_FORM_TABLE) return -1;
  u32 w[8];
  uint8_t l[32];
  fr_to_words(K.L, w);
  memcpy(l, w, 32);
  CsDigits D;
  plan(l, false, form, &D);
  Aligned<uint8_t> in_p(n * 64 + 1);
  if (n) memcpy(in_p.p(), pts, n * 64);
  Aligned<u32> table(VB_TABLE_WORDS);
  for (size_t i = 0; i < n; i++) ok[i] = (uint8_t)(form == CS_FORM_TABLE ? item_subgroup<true>(in_p.p(), i, D, table.p()) : item_subgroup<false>(in_p.p(), i, D, table.p()));
  return 0;
}
}
