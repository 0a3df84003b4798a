// Exponential-ElGamal encryption and re-randomisation in one launch (include/bjj_hip_elgamal.h): the per-item body of
// bjj_k_elgamal_encrypt,   c1 = A1 + r G,   c2 = A2 + m G + r PK,   over the fixed-base tables of G and PK.  __host__ __device__
// like bases.hpp, so that tests/elgamal_emul runs exactly this code on the CPU.
//
// The chains are those of mul_bases_item (bases.hpp) with two differences.  The m-chain walks only nwin_m = ceil(65 / W) windows
// of G's table: m < 2^64 <= 2^(W nwin_m - 1), so the top window holds at most W - 1 bits of m, top digit + carry <= 2^(W-1) stays
// a non-negative digit and no carry leaves the chain -- the argument of base_nwin with 65 in place of 255; m needs no reduction.
// And when an addend follows, the chain's last addition produces T, and the addend goes in as one more mixed addition of its
// affine Niels triple (as cs_item does, common_scalar.hpp).
#pragma once
#include "bases.hpp"

namespace bjj {

// how a chain obtains its scalar: r reduced mod 8l (a caller's table), r reduced mod l (the context's B8 table), or m as it is
enum : int { EG_R_MOD_ORDER = 0, EG_R_MOD_L = 1, EG_M = 2 };
struct EgChain { const u32* table; int W, nwin, kind; };
// b[0]: r over G (c1);  b[1]: m over G, b[2]: r over PK (c2; m == nullptr: the m-chain is not run).  add_c1 / add_c2: both or neither.
struct ElgamalArgs {
  EgChain b[3];
  const uint64_t* m;
  const uint8_t* r;
  const uint8_t* add_c1;
  const uint8_t* add_c2;
};

BJJ_HD int elgamal_nwin_m(int W) { return (65 + W - 1) / W; }

// sum over the t chains of b for ONE item: mul_bases_item's stream of additions -- the first chain starts with the gathers of
// windows 0 and 1 in flight together (nwin >= 3 for every chain and every W <= 28), the addition that ends a chain is kept back
// until the first gather of the next chain is issued.  WANT_T: the caller adds to the result, so the last addition produces T.
template <bool WANT_T, class G, class LoadScalar>
BJJ_HD Ext elgamal_chains(const EgChain* b, int t, G g, const LoadScalar& load, const Consts& K) {
  static_assert(G::kBuffers >= 2, "the gathers of windows 0 and 1 of the first chain are in flight together");
  Ext acc = ext_identity();
  Niels cur = Niels{fr_one(), fr_one(), fr_zero()};
  typename G::Pending p0, p;
  int q = 0;   // staging buffer of the next gather; strictly alternating
  bool neg0, neg;
#pragma unroll 1
  for (int j = 0; j < t; j++) {
    const EgChain& B = b[j];
    u32 raw[8], sc[8];
    load(B.kind, raw);
    if (B.kind == EG_R_MOD_L) scalar_mod_l(raw, sc, K);
    else if (B.kind == EG_R_MOD_ORDER) scalar_mod_order(raw, sc, K);
    else { for (int i = 0; i < 8; i++) sc[i] = raw[i]; }
    DigitStream ds = digit_stream(sc, B.W);
    g.table = B.table;
    g.issue(digit_next(ds, neg0), p0, q);
    if (j == 0) {
      g.issue(digit_next(ds, neg), p, q ^ 1);
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

// record i of an add array: on the curve?  ((0, 0) is not.)  Coordinates >= r are reduced by the conversion.
BJJ_HD bool elgamal_add_on_curve(const uint8_t* add, size_t i, const Consts& K) {
  u32 w[8];
  load_w8(add + i * 64, w);      const Fr x = fr_to_mont_words(w);
  load_w8(add + i * 64 + 32, w); const Fr y = fr_to_mont_words(w);
  return ref_on_curve(x, y, K);
}
// p + A_i, A_i as its affine Niels triple; nothing reads the sum's T.  `on` false: the identity goes in (the sum is not used).
BJJ_HD Ext elgamal_add(const Ext& p, const uint8_t* add, size_t i, bool on, const Consts& K) {
  u32 w[8];
  load_w8(add + i * 64, w);      const Fr x = fr_select(on, fr_to_mont_words(w), fr_zero());
  load_w8(add + i * 64 + 32, w); const Fr y = fr_select(on, fr_to_mont_words(w), fr_one());
  const PNiels a = ext_to_pniels(ext_from_ref_affine(x, y, K), K);
  return ext_madd<false>(p, Niels{a.ymx, a.ypx, a.t2d});
}

// ONE item.  sink(0, c1, on) is called before the chains of c2 start, sink(1, c2, on) at the end: one accumulator is live at a
// time.  Every lane of a wave runs every gather whatever its addends are; on == false: A1 or A2 fails the curve equation and the
// point the sink receives is not meaningful.  The addends are read again where they are added rather than held over a chain
// (registers); an item's own output records may be its addend records: each is read for the last time before the sink that
// overwrites it runs.
template <bool ADD, class G, class Sink>
BJJ_HD bool elgamal_item(const ElgamalArgs& A, G g, size_t i, const Sink& sink, const Consts& K) {
  bool on = true;
  if (ADD) {
    const bool on1 = elgamal_add_on_curve(A.add_c1, i, K), on2 = elgamal_add_on_curve(A.add_c2, i, K);
    on = on1 && on2;
  }
  const auto load = [&](int kind, u32 raw[8]) {
    if (kind == EG_M) {
      const uint64_t m = A.m[i];
      raw[0] = (u32)m; raw[1] = (u32)(m >> 32);
      for (int k = 2; k < 8; k++) raw[k] = 0u;
    } else {
      load_w8(A.r + i * 32, raw);
    }
  };
#pragma unroll 1
  for (int which = 0; which < 2; which++) {
    const EgChain* b = which == 0 ? A.b : A.m ? A.b + 1 : A.b + 2;
    Ext p = elgamal_chains<ADD>(b, which == 1 && A.m ? 2 : 1, g, load, K);
    BJJ_SCHED_FENCE();   // the addend's loads and conversions stay behind the chain: they are not live over its last addition
    if (ADD) p = elgamal_add(p, which ? A.add_c2 : A.add_c1, i, on, K);
    sink(which, p, on);
  }
  return on;
}

}  // namespace bjj
