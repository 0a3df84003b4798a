// Two points, two scalars, and Chaum-Pedersen proofs over them (include/bjj_hip_dleq.h): the per-item bodies of bjj_k_mul_pair,
// bjj_k_dleq_verify, bjj_k_dleq_nonce and bjj_k_dleq_respond.  __host__ __device__ like elgamal.hpp, so that tests/dleq_emul runs
// exactly this code on the CPU.
//
// out = A + a P + b Q is the joint windowed loop of the EdDSA fast path (joint_mul_windowed, bjj_device.hpp) with two full-width
// scalars: both reduced mod 8l (< 2^254, what 64 signed 4-bit windows hold), two per-lane tables {0 .. 8} P and {0 .. 8} Q built
// from the affine points (vb_build_table with affine_base), 63 x 4 doublings shared by the two additions of a window.  The last
// addition produces T, and A goes in as one mixed addition of its affine Niels triple (as cs_item does, common_scalar.hpp).  For
// ON-CURVE inputs -- torsion points and points outside the prime-order subgroup included -- the addition law is complete and
// canonical affine coordinates are unique (the argument of common_scalar.hpp), so the bytes are those of
// bjj_point_add(bjj_point_add(A, bjj_mul_var_base(P, a)), bjj_mul_var_base(Q, b)).
//
// A proof that log_G PK = log_C1 D is (A, B, z) with c = Poseidon5(Poseidon5(tag, C1, D), A, B):   z G = A + c PK,   z C1 = B + c D.
// The verifier evaluates the two equations as   z G + (-c) PK == A   (ONE walk over the fixed-base tables of G and PK, table_chains
// of bases.hpp, as bjj_k_elgamal_encrypt walks m G + r PK)   and   z C1 + c (-D) == B   (the joint loop over the per-lane tables of
// C1 and -D), each compared projectively with the affine point the proof carries: X == F x Z and Y == y Z with Z != 0, which holds
// for exactly one affine (x, y) -- the point the walk computed, a curve point.  An A or B off the curve can therefore never pass,
// and nothing is inverted.
#pragma once
#include "signer.hpp"

namespace bjj {

// ---- shared pieces -----------------------------------------------------------------------------------------------------------------
// record i of a 64-byte point array as Montgomery coordinates (>= r: reduced by the conversion)
BJJ_HD void dleq_load_xy(const uint8_t* a, size_t i, Fr& x, Fr& y) {
  u32 w[8];
  load_w8(a + i * 64, w);      x = fr_to_mont_words(w);
  load_w8(a + i * 64 + 32, w); y = fr_to_mont_words(w);
}
// is record i of a 64-byte point array two canonical field elements (both < r)?
BJJ_HD bool dleq_xy_canonical(const uint8_t* a, size_t i) {
  u32 w[8];
  load_w8(a + i * 64, w);      const bool xg = words_ge_modulus(w);
  load_w8(a + i * 64 + 32, w); const bool yg = words_ge_modulus(w);
  return !xg && !yg;
}
// c = Poseidon5(Poseidon5(tag, C1.x, C1.y, D.x, D.y), A.x, A.y, B.x, B.y) as a canonical plain integer (< r); inputs Montgomery
template <bool PAIRS>
BJJ_HD Fr dleq_challenge(const Fr& tag, const Fr& c1x, const Fr& c1y, const Fr& dx, const Fr& dy, const Fr& ax, const Fr& ay, const Fr& bx,
                         const Fr& by, const Consts& K) {
  Fr h[5];
  h[0] = tag; h[1] = c1x; h[2] = c1y; h[3] = dx; h[4] = dy;
  h[0] = poseidon5_t<PAIRS>(h, K);
  h[1] = ax; h[2] = ay; h[3] = bx; h[4] = by;
  return fr_canon(fr_mul(poseidon5_t<PAIRS>(h, K), fr_one_plain()));
}
// p == (x, y) with p projective on the internal curve (x' = F x) and (x, y) affine on the reference curve (Montgomery)
BJJ_HD bool dleq_same_point(const Ext& p, const Fr& x, const Fr& y, const Consts& K) {
  return fr_eq(p.X, fr_mul(fr_mul(x, K.F), p.Z)) && fr_eq(p.Y, fr_mul(y, p.Z));
}

// ---- bjj_mul_pair ------------------------------------------------------------------------------------------------------------------
struct PairArgs { const uint8_t *p, *q, *a, *b, *add; };   // P, Q (64 B), a, b (32 B), A (64 B or nullptr) per item

// a P + b Q for on-curve affine P, Q (Montgomery, reference curve) and raw 256-bit a, b.  tbl: 2 * VB_TABLE_WORDS words of this lane.
// The result carries T (the caller may go on adding).
BJJ_HD Ext pair_mul(const Fr& px, const Fr& py, const Fr& qx, const Fr& qy, const u32 a[8], const u32 b[8], u32* tbl, const Consts& K) {
  u32 ra[8], rb[8];
  scalar_mod_order(a, ra, K);
  scalar_mod_order(b, rb, K);
  u32* const tbl2 = tbl + VB_TABLE_WORDS;
  vb_build_table(ext_from_ref_affine(px, py, K), tbl, K, true);
  vb_build_table(ext_from_ref_affine(qx, qy, K), tbl2, K, true);
  return joint_mul_windowed(tbl, tbl2, fr_from_words(ra), fr_from_words(rb), 64, K);
}
// ONE item: p = A_i + a_i P_i + b_i Q_i, ready for the affine epilogue.  false: P_i, Q_i or A_i fails the curve equation ((0, 0)
// does) and p is not meaningful.  The lanes of a wave may diverge here: nothing below is wave-cooperative.
BJJ_HD bool pair_item(const PairArgs& A, size_t i, u32* tbl, Ext& p, const Consts& K) {
  Fr px, py, qx, qy;
  dleq_load_xy(A.p, i, px, py);
  dleq_load_xy(A.q, i, qx, qy);
  bool on = ref_on_curve(px, py, K) && ref_on_curve(qx, qy, K);
  if (A.add) {
    Fr ax, ay;
    dleq_load_xy(A.add, i, ax, ay);
    on = ref_on_curve(ax, ay, K) && on;
  }
  if (!on) return false;
  u32 a[8], b[8];
  load_w8(A.a + i * 32, a);
  load_w8(A.b + i * 32, b);
  p = pair_mul(px, py, qx, qy, a, b, tbl, K);
  if (A.add) {   // the addend is read again here rather than held over the loop; nothing reads the sum's T
    Fr ax, ay;
    dleq_load_xy(A.add, i, ax, ay);
    const PNiels n = ext_to_pniels(ext_from_ref_affine(ax, ay, K), K);
    p = ext_madd<false>(p, Niels{n.ymx, n.ypx, n.t2d});
  }
  return true;
}

// ---- bjj_dleq_verify ---------------------------------------------------------------------------------------------------------------
// b[0]: G's table (mod_l set for the context's B8 table), b[1]: PK's table; tag: Montgomery, converted once per call on the host
struct DleqVerifyArgs {
  BaseDesc b[2];
  Fr tag;
  const uint8_t *c1, *d, *a, *b_xy, *z;
};
enum : int { DLEQ_REJECT = 0, DLEQ_ACCEPT = 1, DLEQ_OFF_CURVE = 2 };

// (8l - (c mod 8l)) mod 8l as 8 words: the scalar of -c over a table whose scalars are taken mod 8l
BJJ_HD void dleq_neg_mod_order(const u32 c[8], u32 out[8], const Consts& K) {
  u32 r[8];
  scalar_mod_order(c, r, K);
  const Fr rc = fr_from_words(r);
  Fr t = K.ORDER;
  limbs_submul(t, 1u, rc);                     // 8l - c: in (0, 8l]
  t = fr_select(limbs_is_zero(rc), rc, t);     // c == 0 (mod 8l): 0
  fr_to_words(t, out);
}
// ONE item, from the reads to the verdict.  Straight-line like signer_item_verdict: the table chains gather wave-cooperatively, so an
// item whose verdict is known early (off the curve, a non-canonical field) runs through the same arithmetic on its meaningless data.
// g: the gather policy of both chains; tbl: 2 * VB_TABLE_WORDS words of this lane.
template <class G>
BJJ_HD int dleq_verify_item(const DleqVerifyArgs& A, G g, size_t i, u32* tbl, const Consts& K) {
  // Three phases, each of which hands the next as little as it can (registers): the hash leaves c (8 words) and two flags, the table
  // walk one more flag; every record is read again where it is used (signer_reload: a fresh fetch, not words kept since the first).
  u32 cw[8];
  bool on, canonical;
  {
    u32 zw[8];
    load_w8(A.z + i * 32, zw);
    canonical = limbs_lt(fr_from_words(zw), K.L) && dleq_xy_canonical(A.a, i) && dleq_xy_canonical(A.b_xy, i);
    Fr c1x, c1y, dx, dy, ax, ay, bx, by;
    dleq_load_xy(A.c1, i, c1x, c1y);
    dleq_load_xy(A.d, i, dx, dy);
    on = ref_on_curve(c1x, c1y, K) && ref_on_curve(dx, dy, K);
    dleq_load_xy(A.a, i, ax, ay);
    dleq_load_xy(A.b_xy, i, bx, by);
    fr_to_words(dleq_challenge<true>(A.tag, c1x, c1y, dx, dy, ax, ay, bx, by, K), cw);
  }
  // z G + (-c) PK in one walk over the two fixed-base tables
  bool same_a;
  {
    const Ext w1 = table_chains<false>(A.b, 2, g, [&](int j, const BaseDesc& B, u32 sc[8]) {
      if (j == 0) {
        u32 zw[8];
        load_w8((const uint8_t*)signer_reload(A.z) + i * 32, zw);
        if (B.mod_l) scalar_mod_l(zw, sc, K); else scalar_mod_order(zw, sc, K);
      } else {
        dleq_neg_mod_order(cw, sc, K);
      }
    }, K);
    Fr ax, ay;
    dleq_load_xy((const uint8_t*)signer_reload(A.a), i, ax, ay);
    same_a = dleq_same_point(w1, ax, ay, K);
  }
  // z C1 + c (-D) over two per-lane tables; z < l or the verdict is 0 whatever comes out (the reduction keeps the walk in range)
  u32 zr[8], cr[8];
  load_w8((const uint8_t*)signer_reload(A.z) + i * 32, zr);
  scalar_mod_order(zr, zr, K);
  scalar_mod_order(cw, cr, K);
  u32* const tbl2 = tbl + VB_TABLE_WORDS;
  {
    Fr c1x, c1y, dx, dy;
    dleq_load_xy((const uint8_t*)signer_reload(A.c1), i, c1x, c1y);
    dleq_load_xy((const uint8_t*)signer_reload(A.d), i, dx, dy);
    vb_build_table(ext_from_ref_affine(c1x, c1y, K), tbl, K, true);
    vb_build_table(ext_from_ref_affine(fr_neg(dx), dy, K), tbl2, K, true);
  }
  const Ext w2 = joint_mul_windowed(tbl, tbl2, fr_from_words(zr), fr_from_words(cr), 64, K);
  Fr bx, by;
  dleq_load_xy((const uint8_t*)signer_reload(A.b_xy), i, bx, by);
  const bool same_b = dleq_same_point(w2, bx, by, K);
  return !on ? DLEQ_OFF_CURVE : (canonical && same_a && same_b) ? DLEQ_ACCEPT : DLEQ_REJECT;
}

// ---- bjj_dleq_prove ----------------------------------------------------------------------------------------------------------------
// The points come from a launch chain (bjj_dleq.inc): D = sk' C1 (bjj_k_mul_common), A = w' G (bjj_k_mul_bases), B = w' C1 (K2).
// Two bodies frame it.  dleq_nonce_item writes w' = w mod l where z will stand, so that every launcher of the chain reads a scalar its
// own reduction (mod l or mod 8l) leaves alone.  dleq_respond_item reads the three points back, hashes, and replaces w' by
// z = w' + (c mod l) sk' mod l: the scalar-field arithmetic of sign_item's S (sign.hpp).
BJJ_HD void dleq_nonce_item(const uint8_t* w, size_t i, uint8_t* z, const Consts& K) {
  u32 raw[8], red[8];
  load_w8(w + i * 32, raw);
  scalar_mod_l(raw, red, K);
  store_w8(z + i * 32, red);
}
// sk: sk mod l as 8 words (by value in the kernel arguments); tag Montgomery.  on == false (C1 off the curve): the four outputs are zeroed.
struct DleqRespondArgs {
  u32 sk[8];
  Fr tag;
  const uint8_t* c1;
  uint8_t *d, *a, *b_xy, *z;
};
BJJ_HD void dleq_respond_item(const DleqRespondArgs& A, size_t i, bool on, const Consts& K) {
  if (!on) {
    const u32 zero[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    store_w8(A.d + i * 64, zero); store_w8(A.d + i * 64 + 32, zero);
    store_w8(A.a + i * 64, zero); store_w8(A.a + i * 64 + 32, zero);
    store_w8(A.b_xy + i * 64, zero); store_w8(A.b_xy + i * 64 + 32, zero);
    store_w8(A.z + i * 32, zero);
    return;
  }
  Fr c1x, c1y, dx, dy, ax, ay, bx, by;
  dleq_load_xy(A.c1, i, c1x, c1y);
  dleq_load_xy(A.d, i, dx, dy);
  dleq_load_xy(A.a, i, ax, ay);
  dleq_load_xy(A.b_xy, i, bx, by);
  const Fr c = dleq_challenge<false>(A.tag, c1x, c1y, dx, dy, ax, ay, bx, by, K);   // < r < 2^254
  u32 ww[8];
  load_w8(A.z + i * 32, ww);                                     // w' < l
  const Fr t = fl_mul(fr_from_words(A.sk), K.L_R2, K);           // sk' 2^261 mod l, < 2l
  const Fr z = fl_canon4(fr_add(fl_mul(c, t, K), fr_from_words(ww)), K);   // c sk' (< 2l) + w' (< l)
  u32 zw[8];
  fr_to_words(z, zw);
  store_w8(A.z + i * 32, zw);
}

}  // namespace bjj
