// One scalar, many points (bjj_mul_common / bjj_in_subgroup / bjj_elgamal_decrypt, k_common_scalar.hip): out_i = A_i +- k * P_i with
// ONE k for the whole launch.  The per-lane bodies and the host's recoding; __host__ __device__ like point_sum.hpp, so that
// tests/common_scalar_emul runs exactly this code on the CPU with bound assertions.
//
// Reference semantics: Point::mul_scalar (src/lib.rs:149-164) followed by PointProjective::add / affine (src/lib.rs:88-131, 70-85).
// The addition law is complete on the curve and canonical affine coordinates are unique, so for every ON-CURVE input -- points of
// order 1, 2, 4, 8 and points outside the prime-order subgroup included -- any correct evaluation gives the reference's bytes.
//
// The scalar never reaches the device as a number.  The host reduces it mod 8l (the group order), negates the digits for a
// subtraction and recodes it once (cs_recode) into a string of signed digits that travels BY VALUE in the kernel arguments; the
// kernel indexes it with a wave-uniform loop counter, so a zero digit is a doubling under a uniform branch, leading zeros do not exist
// (the loop starts at the top digit) and the sign of a digit is a scalar select.  Two forms of the same loop:
//   table-free   plain NAF, digits in {0, +-1}: P stays in registers as an affine Niels triple, one mixed addition per non-zero digit
//   table        width-5 NAF, odd digits |d| <= 15: {P, 3P, .., 15P} in the lane's variable-base table (K2's packed layout, entries
//                1 .. 8), built with one doubling and seven additions, one projective-Niels addition per non-zero digit
// and the host picks per call by counting field multiplications (cs_choose_form).
#pragma once
#include "bjj_device.hpp"

namespace bjj {

// ---- the digit string -------------------------------------------------------------------------------------------------------------
// k mod 8l < 2^254, so either recoding has at most 255 digits (indices 0 .. 254).  Digit i is the signed byte i & 3 of w[i >> 2];
// top = index of the highest non-zero digit, -1 for k == 0 (mod 8l).  260 bytes of kernel arguments.
constexpr int CS_MAX_DIGITS = 255;
constexpr int CS_DIGIT_WORDS = 64;
struct CsDigits { int32_t top; u32 w[CS_DIGIT_WORDS]; };
enum : int { CS_FORM_NAF = 0, CS_FORM_TABLE = 1 };

BJJ_HD int cs_digit(const CsDigits& D, int i) { return (int)(int8_t)(uint8_t)(D.w[i >> 2] >> (8 * (i & 3))); }

// Field multiplications (squarings count as one) behind the form rule, from the formulas of curve.hpp:
//   a non-zero NAF digit      ext_madd without T = 6, and the doubling in front of it computes a T it otherwise would not = 1
//   a non-zero width-5 digit  ext_add_pn without T = 7, and the same T of the doubling in front = 1
//   the table                 2P = ext_dbl with T = 8; seven ext_add_pn with T = 56; 2D'T of the nine projective-Niels forms (P, 2P and
//                             3P .. 15P) = 9
// The doublings are the same in both forms and do not enter.
constexpr int CS_NAF_DIGIT_MULS = 7;
constexpr int CS_TABLE_DIGIT_MULS = 8;
constexpr int CS_TABLE_BUILD_MULS = 73;
BJJ_HD int cs_cost_naf(int weight_naf) { return CS_NAF_DIGIT_MULS * weight_naf; }
BJJ_HD int cs_cost_table(int weight_w5) { return CS_TABLE_BUILD_MULS + CS_TABLE_DIGIT_MULS * weight_w5; }
BJJ_HD int cs_choose_form(int weight_naf, int weight_w5) { return cs_cost_table(weight_w5) < cs_cost_naf(weight_naf) ? CS_FORM_TABLE : CS_FORM_NAF; }

// Host side (CPU-testable): raw = any 256-bit integer, 8 little-endian words.  k = raw mod 8l (scalar_mod_order); the digits of k in
// width-w non-adjacent form, w = 2 (CS_FORM_NAF) or 5 (CS_FORM_TABLE): every non-zero digit is odd, |d| < 2^(w-1), and the w - 1 digits
// above it are zero.  negate: every digit with its sign flipped, so that the string sums to -k.  Returns the number of non-zero digits.
inline int cs_recode(const u32 raw[8], bool negate, int form, CsDigits* out, const Consts& K) {
  const int w = form == CS_FORM_TABLE ? 5 : 2;
  u32 v[9];
  scalar_mod_order(raw, v, K);
  v[8] = 0;
  out->top = -1;
  for (int i = 0; i < CS_DIGIT_WORDS; i++) out->w[i] = 0;
  int weight = 0;
  for (int i = 0; i <= CS_MAX_DIGITS; i++) {
    u32 any = 0;
    for (int j = 0; j < 9; j++) any |= v[j];
    if (!any) break;
    if (i == CS_MAX_DIGITS) return -1;   // cannot happen for k < 2^254
    if (v[0] & 1u) {
      int d = (int)(v[0] & ((1u << w) - 1u));
      if (d >= (1 << (w - 1))) d -= 1 << w;
      // v -= d
      if (d > 0) {
        u64 borrow = (u64)d;
        for (int j = 0; j < 9 && borrow; j++) { const u64 t = (u64)v[j] - borrow; v[j] = (u32)t; borrow = (t >> 63) & 1u; }
      } else {
        u64 carry = (u64)(-d);
        for (int j = 0; j < 9 && carry; j++) { const u64 t = (u64)v[j] + carry; v[j] = (u32)t; carry = t >> 32; }
      }
      const int s = negate ? -d : d;
      out->w[i >> 2] |= (u32)(uint8_t)(int8_t)s << (8 * (i & 3));
      out->top = i;
      weight++;
    }
    for (int j = 0; j < 8; j++) v[j] = (v[j] >> 1) | (v[j + 1] << 31);
    v[8] >>= 1;
  }
  return weight;
}

// ---- the table of the table form: entry e = 1 .. 8 holds (2e - 1) * P ---------------------------------------------------------------
BJJ_HD void cs_build_table(const Ext& P, const PNiels& p1, u32* tbl, const Consts& K) {
  vb_table_store(tbl, 1, p1);
  const PNiels p2 = ext_to_pniels(ext_dbl<true>(P), K);
  Ext cur = P;
#pragma unroll 1
  for (u32 e = 2; e <= 8; e++) {
    cur = ext_add_pn(cur, p2);
    vb_table_store(tbl, e, ext_to_pniels(cur, K));
  }
}

// ---- (sum of the digits) * P for an on-curve P = (x, y) (Montgomery, reference curve) -----------------------------------------------
// Most significant digit first.  Every branch on a digit is wave-uniform.  A doubling computes its T only in front of an addition,
// an addition only when nothing but the caller's own addition follows (WANT_T: the last operation of the loop, whichever it is).
template <bool TABLE, bool WANT_T>
BJJ_HD Ext cs_mul(const Fr& x, const Fr& y, const CsDigits& D, u32* tbl, const Consts& K) {
  const int top = D.top;
  if (top < 0) return ext_identity();
  const Ext P = ext_from_ref_affine(x, y, K);
  const PNiels p1 = ext_to_pniels(P, K);
  const Niels pa = {p1.ymx, p1.ypx, p1.t2d};   // Z == 1: the projective-Niels form of P is its affine one (as vb_build_table uses it)
  const int dt = cs_digit(D, top);
  Ext acc;
  if (TABLE) {
    cs_build_table(P, p1, tbl, K);
    const PNiels e = vb_table_load(tbl, (u32)(((dt < 0 ? -dt : dt) + 1) >> 1));
    acc = pniels_to_ext(pniels_cneg(e, dt < 0), K, WANT_T && top == 0);
  } else {
    acc = dt < 0 ? ext_from_ref_affine(fr_neg(x), y, K) : P;
  }
#pragma unroll 1
  for (int i = top - 1; i >= 0; i--) {
    const int d = cs_digit(D, i);
    const bool last_t = WANT_T && i == 0;
    if (d != 0) {
      acc = ext_dbl<true>(acc);
      const bool neg = d < 0;
      if (TABLE) {
        const PNiels e = vb_table_load(tbl, (u32)(((neg ? -d : d) + 1) >> 1));
        acc = ext_add_pn(acc, pniels_cneg(e, neg), last_t);
      } else {
        const Niels q = niels_cneg_lazy(pa, neg);
        acc = last_t ? ext_madd<true>(acc, q) : ext_madd<false>(acc, q);
      }
    } else {
      acc = last_t ? ext_dbl<true>(acc) : ext_dbl<false>(acc);
    }
  }
  return acc;
}

// ---- one item ----------------------------------------------------------------------------------------------------------------------
// p = A_i + (sum of the digits) * P_i, ready for the affine epilogue; add == nullptr: A_i = the identity.  Coordinates >= r are reduced
// mod r by the conversion.  false: P_i or A_i fails the curve equation ((0, 0) does) and p is not meaningful.
template <bool TABLE, bool ADD>
BJJ_HD bool cs_item(const uint8_t* pts, const uint8_t* add, size_t i, const CsDigits& D, u32* tbl, Ext& p, const Consts& K) {
  u32 w[8];
  load_w8(pts + i * 64, w);      const Fr x = fr_to_mont_words(w);
  load_w8(pts + i * 64 + 32, w); const Fr y = fr_to_mont_words(w);
  bool on = ref_on_curve(x, y, K);
  Fr ax = fr_zero(), ay = fr_one();
  if (ADD) {
    load_w8(add + i * 64, w);      ax = fr_to_mont_words(w);
    load_w8(add + i * 64 + 32, w); ay = fr_to_mont_words(w);
    on = ref_on_curve(ax, ay, K) && on;
  }
  if (!on) return false;
  p = cs_mul<TABLE, ADD>(x, y, D, tbl, K);
  if (ADD) {   // a mixed addition of A's affine Niels triple; nothing reads the sum's T
    const PNiels a1 = ext_to_pniels(ext_from_ref_affine(ax, ay, K), K);
    p = ext_madd<false>(p, Niels{a1.ymx, a1.ypx, a1.t2d});
  }
  return true;
}
// the subgroup epilogue: is p the identity (0 : Z : Z)?  Projective, no inversion.
BJJ_HD bool cs_is_identity(const Ext& p) { return fr_is_zero(p.X) && fr_eq(p.Y, p.Z); }

}  // namespace bjj
