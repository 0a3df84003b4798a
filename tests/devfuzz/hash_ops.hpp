// TEST-ONLY: one item of the shipped Poseidon layer (csrc/poseidon.hpp: poseidon5_t in both forms of its partial rounds, one
// poseidon_full_round) and of the DLEQ challenge built on it (csrc/dleq.hpp: dleq_challenge in both forms), on raw limbs chosen
// by the test.  The same body runs on the GPU (hash.hip -> libbjj_hash_test.so) and on the CPU (tests/emul/emul_hash_ops.cpp:
// emul_hash_op, with the BJJ_ASSERTs and the operand checks of fr_dot3 live), so tests/test_gpu_hash_ops.py can compare the two
// builds bit for bit and both against the plain integers of tests/hash_ref.py.  Every op calls the function the kernels call;
// nothing here restates the arithmetic.  The includer provides csrc/dleq.hpp (and with it csrc/poseidon.hpp).
#pragma once

namespace bjj {

enum {
  HO_P5_PLAIN = 0,          // in: 5 x 9 raw limbs (Montgomery)      out: poseidon5_t<false>, 9 raw limbs, then its plain canonical 8 words
  HO_P5_PAIRS = 1,          // in: 5 x 9 raw limbs                   out: poseidon5_t<true>, 9 raw limbs, then 8 words
  HO_FULL_ROUND = 2,        // in: 6 x 9 raw limbs, 1 word (round)   out: the state after poseidon_full_round, 6 x 9 raw limbs
  HO_CHALLENGE_PLAIN = 3,   // in: 9 x 9 raw limbs (tag, C1, D, A, B) out: dleq_challenge<false>, 8 words
  HO_CHALLENGE_PAIRS = 4,   // in: 9 x 9 raw limbs                   out: dleq_challenge<true>, 8 words
  HO_NOPS = 5
};
// record widths in words; which = 0: in, 1: out
BJJ_HD int hash_words(int op, int which) {
  switch (op) {
    case HO_P5_PLAIN: case HO_P5_PAIRS: return which == 0 ? 5 * NL : NL + 8;
    case HO_FULL_ROUND: return which == 0 ? 6 * NL + 1 : 6 * NL;
    default: return which == 0 ? 9 * NL : 8;
  }
}
BJJ_HD Fr ho_raw(const u32* p) { Fr f; for (int i = 0; i < NL; i++) f.v[i] = p[i]; return f; }
BJJ_HD void ho_put_raw(u32* p, const Fr& f) { for (int i = 0; i < NL; i++) p[i] = f.v[i]; }
// the hash as raw limbs, then as the plain canonical integer verify_fast_t and dleq_challenge derive from it
BJJ_HD void ho_put_hash(u32* o, const Fr& h) {
  ho_put_raw(o, h);
  fr_to_words(fr_canon(fr_mul(h, fr_one_plain())), o + NL);
}
template <bool PAIRS>
BJJ_HD void ho_challenge(const u32* in, u32* o, const Consts& K) {
  fr_to_words(dleq_challenge<PAIRS>(ho_raw(in), ho_raw(in + NL), ho_raw(in + 2 * NL), ho_raw(in + 3 * NL), ho_raw(in + 4 * NL), ho_raw(in + 5 * NL),
                                    ho_raw(in + 6 * NL), ho_raw(in + 7 * NL), ho_raw(in + 8 * NL), K), o);
}

BJJ_HD void hash_op(int op, const u32* in, u32* o, const Consts& K) {
  switch (op) {
    case HO_P5_PLAIN: case HO_P5_PAIRS: {
      Fr x[5];
      for (int j = 0; j < 5; j++) x[j] = ho_raw(in + j * NL);
      ho_put_hash(o, op == HO_P5_PLAIN ? poseidon5_t<false>(x, K) : poseidon5_t<true>(x, K));
      break;
    }
    case HO_FULL_ROUND: {
      Fr st[6];
      for (int j = 0; j < 6; j++) st[j] = ho_raw(in + j * NL);
      const u32 r = in[6 * NL] < 8u ? in[6 * NL] : 7u;
      if (r < 7u) {
        poseidon_full_round<false>(st, &K.PCF[r * 6], K);
      } else {   // the last round forms row 0 only: the other five are not defined, and written as zeros
        poseidon_full_round<true>(st, &K.PCF[7 * 6], K);
        for (int j = 1; j < 6; j++) st[j] = fr_zero();
      }
      for (int j = 0; j < 6; j++) ho_put_raw(o + j * NL, st[j]);
      break;
    }
    case HO_CHALLENGE_PLAIN: ho_challenge<false>(in, o, K); break;
    case HO_CHALLENGE_PAIRS: ho_challenge<true>(in, o, K); break;
    default: break;
  }
}

}  // namespace bjj
