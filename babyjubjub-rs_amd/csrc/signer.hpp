// Verification against ONE signer's fixed-base table (include/bjj_hip_signer.h): the per-item body of bjj_k_verify_signer and its
// verdict step.  __host__ __device__ like bases.hpp, so that tests/signer_emul runs exactly this code on the CPU.
//
// The reference (src/lib.rs:395-412; verify_schnorr :375-385) computes l = B8.mul_scalar(s), t = pk.mul_scalar(8 hm) (Schnorr: hm),
// r = R.projective().add(&t.projective()).affine() and answers l == r.  With pk ON the curve (bjj_base_create refuses any other
// point) l and t are canonical affine points of the group, so any correct evaluation of them is the reference's, with the scalars
// reduced: s mod l over the context's B8 table, 8 (hm mod l) < 8l (Schnorr: hm mod 8l) over the signer's table.  Both chains end
// in projective form with Z != 0 (the addition law of the a' = -1 curve is complete: D' is a non-square).  R is NOT assumed to be
// on the curve: the last addition is the reference's own formula sequence, ref_add, with t left projective -- see signer_verdict.
#pragma once
#include "bases.hpp"

namespace bjj {

// What bjj_k_verify_signer knows of a call besides the item arrays; travels in the kernel arguments (136 bytes).  T: the signer's
// table (scalar mod 8l), L: the context's B8 table (scalar mod l), pk: the signer's point as the hash takes it -- Montgomery form,
// converted ONCE per call on the host (signer_point: the conversion the kernels apply to a record, so coordinates >= r are
// reduced), wave-uniform in the kernel: it stays in scalar registers and costs an item nothing.
struct SignerPoint { Fr x, y; };
struct SignerArgs { BaseDesc T, L; SignerPoint pk; };
BJJ_HD SignerPoint signer_point(const u32 xy[16]) {
  SignerPoint p;
  p.x = fr_to_mont_words(xy); p.y = fr_to_mont_words(xy + 8);
  return p;
}
// Reads through a pointer the compiler cannot connect with an earlier read of the same record: the record is FETCHED again instead
// of its words being kept (in registers the two table chains need, i.e. in scratch memory) since the first read.
BJJ_HD const void* signer_reload(const void* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(p));
#endif
  return p;
}
// the descriptor set of ONE base for mul_bases_item: t = 1 is a constant here, so its loop over the bases folds away
BJJ_HD BasesArgs signer_one_base(const BaseDesc& d) {
  BasesArgs a;
  a.b[0] = d; a.t = 1;
  return a;
}

// l == (R + t).affine() with l = L and t = T given PROJECTIVELY on the internal curve (x' = F x, Z != 0), R = (rx, ry) affine on the
// reference curve (Montgomery, any field elements).  PointProjective::add (src/lib.rs:88-131) is homogeneous of degree 4 in its
// second operand when the first has z = 1: with (x2, y2, 1) replaced by (c x2, c y2, c)
//     a, c, d, aux, dac  pick up c;    b, e, f, g  pick up c^2;    x3, y3, z3  pick up c^4
// so ref_add((rx, ry, 1), (T.X / F, T.Y, T.Z)) is the reference's sum times T.Z^4 != 0: the same affine(), and z == 0 exactly when
// the reference's is.  z == 0 makes the reference's r = (0, 0) (:71-76), which l, a curve point, never is: verdict 0.  Otherwise
// r == l  <=>  sum.x * L.Z == (L.X / F) * sum.z  and  sum.y * L.Z == L.Y * sum.z  (L.Z, sum.z != 0).  No inversion, no branch.
BJJ_HD int signer_verdict(const Ext& L, const Ext& T, const Fr& rx, const Fr& ry, const Consts& K) {
  RefProj rp; rp.x = rx; rp.y = ry; rp.z = fr_one();
  RefProj tp; tp.x = fr_mul(T.X, K.FINV); tp.y = T.Y; tp.z = T.Z;
  const RefProj sum = ref_add(rp, tp, K);                                   // :407-410 / :382
  const Fr lx = fr_mul(L.X, K.FINV);
  const bool same_x = fr_eq(fr_mul(sum.x, L.Z), fr_mul(lx, sum.z));
  const bool same_y = fr_eq(fr_mul(sum.y, L.Z), fr_mul(L.Y, sum.z));
  return (!fr_is_zero(sum.z) && same_x && same_y) ? 1 : 0;                  // :411 / :384
}

// One item, from the message read to the verdict: 0 / 1 (EdDSA), 0 / 1 / 2 (SCHNORR: 2 = Err, msg > Q) -- what verify_fast_t /
// verify_exact_t give for the key pk, whose table dT describes (scalar mod 8l; dL: the context's B8 table, scalar mod l).  The body
// of bjj_k_verify_signer and of bjj_k_verify_set (signer_set.hpp), which differ in where pk comes from and in how the signer chain
// gathers: gT is the policy of the chain over dT, gL of the chain over dL.  Straight-line: an item whose verdict is known early
// (msg > Q) runs through the same arithmetic, because the cooperative gather needs every lane of the wave.  Two chains of
// mul_bases_item, t = 1 each, whose `load` hook hands over a scalar held in registers; the signer chain's result is down to
// (X, Y, Z) before the second chain starts, and R is read again after it (two multiplications) instead of living through both.
template <bool SCHNORR, class GT, class GL>
BJJ_HD int signer_item_verdict(const BaseDesc& dT, const BaseDesc& dL, const SignerPoint& pk, const GT& gT, const GL& gL, const void* r,
                               const void* s, const void* msg, const Consts& K) {
  u32 w[8];
  load_w8(msg, w);
  const bool msg_gt = words_gt_modulus(w);                                  // :396-398 / :365-367
  Fr h[5];
  h[4] = fr_to_mont_words(w);                                               // msg == Q wraps to 0, as there
  {
    const Fr ax = pk.x, ay = pk.y;
    load_w8(r, w);                   const Fr rx = fr_to_mont_words(w);
    load_w8((const char*)r + 32, w); const Fr ry = fr_to_mont_words(w);
    if (SCHNORR) { h[0] = ax; h[1] = ay; h[2] = rx; h[3] = ry; }            // :369
    else         { h[0] = rx; h[1] = ry; h[2] = ax; h[3] = ay; }            // :400
  }
  const Fr hm_plain = fr_canon(fr_mul(poseidon5_t<true>(h, K), fr_one_plain()));
  u32 kw[8];
  if (SCHNORR) {
    fr_to_words(hm_plain, kw);                                              // hm < r; the chain reduces it mod 8l
  } else {
    u32 kp[8];
    fr_to_words(plain_mod_l(hm_plain, K), kp);
    kw[0] = kp[0] << 3;
#pragma unroll
    for (int i = 1; i < 8; i++) kw[i] = (kp[i] << 3) | (kp[i - 1] >> 29);   // 8 (hm mod l) < 8l < 2^254
  }
  Ext T = mul_bases_item(signer_one_base(dT), gT, [&](int, u32 raw[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) raw[i] = kw[i];
  }, K);
  T.T = fr_zero();
  u32 sw[8];
  load_w8(s, sw);
  const Ext L = mul_bases_item(signer_one_base(dL), gL, [&](int, u32 raw[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) raw[i] = sw[i];
  }, K);
  const void* r2 = signer_reload(r);
  load_w8(r2, w);                   const Fr rx = fr_to_mont_words(w);
  load_w8((const char*)r2 + 32, w); const Fr ry = fr_to_mont_words(w);
  const int verdict = signer_verdict(L, T, rx, ry, K);
  return msg_gt ? (SCHNORR ? 2 : 0) : verdict;
}
// One item of bjj_k_verify_signer: the key and both gathers are the call's own.
template <bool SCHNORR, class G>
BJJ_HD int verify_signer_item(const SignerArgs& A, const G& g, const void* r, const void* s, const void* msg, const Consts& K) {
  return signer_item_verdict<SCHNORR>(A.T, A.L, A.pk, g, g, r, s, msg, K);
}

}  // namespace bjj
