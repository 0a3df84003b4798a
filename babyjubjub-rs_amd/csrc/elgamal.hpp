// Exponential-ElGamal encryption and re-randomisation in one launch (include/bjj_hip_elgamal.h): the per-item body of
// bjj_k_elgamal_encrypt,   c1 = A1 + r G,   c2 = A2 + m G + r PK,   over the fixed-base tables of G and PK.  __host__ __device__
// like bases.hpp, so that tests/elgamal_emul runs exactly this code on the CPU.
//
// The chains are walked by table_chains (bases.hpp), as bjj_k_mul_bases' are, with two differences.  The m-chain walks only
// nwin_m = ceil(65 / W) windows of G's table: m < 2^64 <= 2^(W nwin_m - 1), so the top window holds at most W - 1 bits of m, top
// digit + carry <= 2^(W-1) stays a non-negative digit and no carry leaves the chain -- the argument of base_nwin with 65 in place
// of 255; m needs no reduction.  And when an addend follows, the chain's last addition produces T, and the addend goes in as one
// more mixed addition of its affine Niels triple (as cs_item does, common_scalar.hpp).
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
  const auto scalar = [&](int, const EgChain& B, u32 sc[8]) {
    if (B.kind == EG_M) {
      const uint64_t m = A.m[i];
      sc[0] = (u32)m; sc[1] = (u32)(m >> 32);
      for (int k = 2; k < 8; k++) sc[k] = 0u;
    } else {
      u32 raw[8];
      load_w8(A.r + i * 32, raw);
      if (B.kind == EG_R_MOD_L) scalar_mod_l(raw, sc, K); else scalar_mod_order(raw, sc, K);
    }
  };
#pragma unroll 1
  for (int which = 0; which < 2; which++) {
    const EgChain* b = which == 0 ? A.b : A.m ? A.b + 1 : A.b + 2;
    Ext p = table_chains<ADD>(b, which == 1 && A.m ? 2 : 1, g, scalar, K);   // ADD: the addend's addition reads T
    BJJ_SCHED_FENCE();   // the addend's loads and conversions stay behind the chain: they are not live over its last addition
    if (ADD) p = elgamal_add(p, which ? A.add_c2 : A.add_c1, i, on, K);
    sink(which, p, on);
  }
  return on;
}

}  // namespace bjj
