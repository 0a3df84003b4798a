// Reusable fixed-base tables for caller-chosen points (include/bjj_hip_bases.h): the table of an ARBITRARY curve point and the
// per-item body of bjj_k_mul_bases, out = sum_j k_j * P_j over up to BJJ_MAX_BASES tables.  __host__ __device__ like
// bjj_device.hpp, so that tests/bases_emul runs exactly this code on the CPU.
//
// A custom table has the layout of the B8 table (bjj_device.hpp "fixed base": signed W-bit digits, 2^(W-1) + 1 entries of 128
// bytes per window, window 0 in T form) and differs in two numbers.  B8 has order l, a curve point in general only an order that
// divides 8l: its scalar is reduced mod 8l (scalar_mod_order, exact for every curve point), and since 8l < 2^254 the table has
// nwin = ceil(255 / W) windows -- the top window then holds at most W - 1 bits of the scalar, so top digit + carry <= 2^(W-1)
// stays a non-negative digit and no carry leaves the table.  The same argument as the 252 of fixed_nwin, where l < 2^251.
#pragma once
#include "bjj_device.hpp"

#define BJJ_BASES_MAX 8   // BJJ_MAX_BASES of include/bjj_hip_bases.h

namespace bjj {

// What the kernel knows of one base, and of a call: plain values that travel in the kernel arguments (no descriptor memory on
// the device).  mod_l: the table is the context's B8 table (scalar mod l, fixed_nwin windows); otherwise mod 8l, base_nwin windows.
struct BaseDesc { const u32* table; const uint8_t* scalars; int W, nwin, mod_l, pad; };
struct BasesArgs { BaseDesc b[BJJ_BASES_MAX]; int t; };

BJJ_HD int base_nwin(int W) { return (255 + W - 1) / W; }

// entry (j, k) = Niels( k * 2^(W j) * P ) of the table of P = (bx, by) (Montgomery, reference curve, ON the curve): the
// independent per-entry definition, fixed_table_entry with the base point as a parameter
BJJ_HD Niels base_table_entry(const Fr& bx, const Fr& by, u32 k, int j, int W, const Consts& K, bool tform = false) {
  Ext base = ext_from_ref_affine(bx, by, K);
  PNiels bn = ext_to_pniels(base, K);
  PNiels idn = pniels_identity();
  Ext acc = ext_identity();
#pragma unroll 1
  for (int b = W - 1; b >= 0; b--) {
    acc = ext_dbl<true>(acc);
    const bool bit = (k >> b) & 1;
    PNiels sel;
    sel.ymx = fr_select(bit, bn.ymx, idn.ymx); sel.ypx = fr_select(bit, bn.ypx, idn.ypx);
    sel.t2d = fr_select(bit, bn.t2d, idn.t2d); sel.z2 = fr_select(bit, bn.z2, idn.z2);
    acc = ext_add_pn(acc, sel);
  }
#pragma unroll 1
  for (int d = 0; d < W * j; d++) acc = ext_dbl<true>(acc);
  Fr zi = fr_inv(acc.Z);
  return niels_from_affine(fr_mul(acc.X, zi), fr_mul(acc.Y, zi), K, tform);
}
// The induction check of the table of P: fixed_table_check_slot's conditions with the anchor point as a parameter (P_0 = P where
// that function has P_0 = B8).  A sibling, not a wrapper: it shares the helpers and restates the conditions, so that neither an
// edit of that function's body can make this one miscount nor this one change the code of the B8 kernels.
//   T[j][0] = identity, T[j][1] = P_j, T[j][k] + P_j = T[j][k+1], P_{j+1} = 2 * T[j][2^(W-1)], P_0 = (ax, ay),
//   every entry canonical with 2D'x'y consistent.  Returns the number of violated conditions for slot (j, k).
BJJ_HD int base_table_check_slot(const u32* table, const u32* bases, int j, u32 k, int W, int nwin, const Fr& ax, const Fr& ay,
                                 const Consts& K) {
  const size_t stride = fixed_stride(W);
  const Niels e = load_niels(table + ((size_t)j * stride + k) * NIELS_WORDS);
  const Niels base = load_niels(bases + (size_t)j * NIELS_WORDS);
  const bool tform = j == 0;   // window 0 holds 2x'y in the third word, the bases (and every other window) 2D'x'y
  int bad = 0;
  for (int i = 0; i < NL; i++) bad += (e.ymx.v[i] >> 29) != 0 || (e.ypx.v[i] >> 29) != 0 || (e.t2d.v[i] >> 29) != 0;
  bad += !niels_limbs_equal(e, Niels{fr_canon(e.ymx), fr_canon(e.ypx), fr_canon(e.t2d)});
  const Fr dsq = fr_sub(fr_sqr(e.ypx), fr_sqr(e.ymx));             // 2 * t2d == D' * (ypx^2 - ymx^2); T form: without the D'
  bad += !fr_eq(tform ? dsq : fr_mul(dsq, K.DP), fr_dbl(e.t2d));
  if (k == 0) bad += !niels_limbs_equal(e, Niels{fr_one(), fr_one(), fr_zero()});
  if (k == 1) bad += !niels_limbs_equal(Niels{e.ymx, e.ypx, tform ? fr_canon(fr_mul(e.t2d, K.DP)) : e.t2d}, base);
  if (k + 1 < stride) {
    const Niels nx = load_niels(table + ((size_t)j * stride + k + 1) * NIELS_WORDS);
    bad += !ext_equals_niels(ext_madd(niels_lift(e, K, tform), base), nx);
  } else if (j + 1 < nwin) {
    const Niels nb = load_niels(bases + (size_t)(j + 1) * NIELS_WORDS);
    bad += !ext_equals_niels(ext_dbl<false>(niels_lift(e, K, tform)), nb);
  }
  if (j == 0 && k == 1) bad += !ext_equals_niels(ext_from_ref_affine(ax, ay, K), e);   // the anchor
  return bad;
}

// The table-chain walk: sum_j k_j * P_j for ONE item over the t tables of b, where k_j is the scalar `scalar(j, b[j], sc)` delivers
// ALREADY REDUCED for that table (8 words) and D is any descriptor with `table`, `W` and `nwin` (BaseDesc; EgChain of
// elgamal.hpp) -- nothing else of a descriptor is read here.  The chains of fixed_base_mul (chain 0: window 0's entry lifted from
// scratch, no multiplication) and fixed_base_accumulate (every further chain: window 0's entry times D', then a 7M addition) run
// as one stream of additions.  Chain 0 starts as fixed_base_mul does, with the gathers of windows 0 and 1 in flight together
// (hence two staging buffers; nwin >= 3 for every table and every W <= 28); from then on one gather is in flight during every
// addition.  The addition that ends chain j is kept back until the first gather of chain j + 1 is issued, so the table reads
// stay overlapped across the seam, and every addition but the very last produces T (another addition reads it).  WANT_T: the
// caller adds to the result, so the last addition produces T too.  G: a gather policy with two staging buffers whose `table`
// member can be re-pointed.
template <bool WANT_T, class D, class G, class Scalar>
BJJ_HD Ext table_chains(const D* b, int t, G g, const Scalar& scalar, const Consts& K) {
  static_assert(G::kBuffers >= 2, "the gathers of windows 0 and 1 of the first chain are in flight together");
  Ext acc = ext_identity();
  Niels cur = Niels{fr_one(), fr_one(), fr_zero()};
  typename G::Pending p0, p;
  int q = 0;   // staging buffer of the next gather; strictly alternating
  bool neg0, neg;
#pragma unroll 1
  for (int j = 0; j < t; j++) {
    const D& B = b[j];
    u32 sc[8];
    scalar(j, B, sc);
    DigitStream ds = digit_stream(sc, B.W);
    g.table = B.table;
    g.issue(digit_next(ds, neg0), p0, q);
    if (j == 0) {
      g.issue(digit_next(ds, neg), p, q ^ 1);                      // window 1 with window 0
      const Niels n0 = niels_cneg_lazy(g.finish(p0, q), neg0);
      acc.X = fr_reduce_weak(fr_sub(n0.ypx, n0.ymx));              // (2x' : 2y : 2 : 2x'y), as fixed_base_mul
      acc.Y = fr_add(n0.ypx, n0.ymx);
      acc.Z = fr_add(fr_one(), fr_one()); acc.T = fr_add(n0.t2d, fr_zero());
    } else {
      acc = ext_madd(acc, cur);                                    // the previous chain's last addition
      BJJ_SCHED_FENCE();
      Niels n0 = niels_cneg_lazy(g.finish(p0, q), neg0);
      g.issue(digit_next(ds, neg), p, q ^ 1);
      n0.t2d = fr_mul(n0.t2d, K.DP);                               // window 0 is stored in T form
      acc = ext_madd(acc, n0);
    }
    BJJ_SCHED_FENCE();
    cur = niels_cneg_lazy(g.finish(p, q ^ 1), neg);                // two gathers since the top of the loop: q is next again
#pragma unroll 1
    for (int w = 2; w < B.nwin; w++) {
      g.issue(digit_next(ds, neg), p, q);
      acc = ext_madd(acc, cur);
      BJJ_SCHED_FENCE();
      cur = niels_cneg_lazy(g.finish(p, q), neg);
      q ^= 1;
    }
  }
  return ext_madd<WANT_T>(acc, cur);
}

// sum_j k_j * P_j for ONE item of bjj_k_mul_bases: the walk over the descriptors of A.  `load(j, raw)` hands over the raw 256-bit
// scalar of base j; the mod-l / mod-8l choice depends on the descriptor alone.  The item's last addition produces no T: the
// epilogue reads X, Y, Z only.
template <class G, class LoadScalar>
BJJ_HD Ext mul_bases_item(const BasesArgs& A, G g, const LoadScalar& load, const Consts& K) {
  return table_chains<false>(A.b, A.t, g, [&](int j, const BaseDesc& B, u32 sc[8]) {
    u32 raw[8];
    load(j, raw);
    if (B.mod_l) scalar_mod_l(raw, sc, K); else scalar_mod_order(raw, sc, K);
  }, K);
}

}  // namespace bjj
