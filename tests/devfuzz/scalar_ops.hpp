// TEST-ONLY: one item of the shipped scalar arithmetic (integers mod l and mod 8l, csrc/curve.hpp, bjj_device.hpp, sign.hpp)
// on raw words chosen by the test.  The same body runs on the GPU (scalar.hip -> libbjj_scalar_test.so) and on the CPU
// (tests/emul/emul_bodies.cpp: emul_scalar_op), so tests/test_gpu_scalar_fuzz.py can compare the two builds bit for bit and
// both against Python integers.  Every op calls the function the kernels call; nothing here restates the arithmetic.
#pragma once

namespace bjj {

enum {
  SC_MOD_L = 0,        // a: 8 words                          out: scalar_mod_l, 8 words
  SC_MOD_ORDER = 1,    // a: 8 words                          out: scalar_mod_order, 8 words
  SC_PLAIN_MOD_L = 2,  // a: 8 words (< r)                    out: plain_mod_l, 8 words
  SC_FL_MUL = 3,       // a, b: 9 raw limbs                   out: fl_mul, 9 raw limbs
  SC_FL_CANON4 = 4,    // a: 9 raw limbs                      out: fl_canon4, 9 raw limbs
  SC_DIGEST = 5,       // a: 16 words (512-bit digest)        out: digest_mod_l, 8 words
  SC_NONCE = 6,        // a: 32 words (1024-bit nonce)        out: nonce_mod_l, 8 words
  SC_WIDE = 7,         // a: nw words                         out: wide_scalar_mod_order, 8 words
  SC_VERIFY_C = 8,     // a: 8 words s; b: 8 words |v|, 1 word sign        out: verify_fb_scalar, 8 words
  SC_SHORT_PAIR = 9,   // a: 8 words kappa (< l)              out: lattice_short_pair: u (8 words), |v| (8 words), sign (1 word)
  SC_EUCLID = 10,      // a: r0, r1, t0, t1 (8 words each)    out: euclid_partial_step: r0', t0' as 9 raw limbs each
  SC_NOPS = 11
};
BJJ_HD int sc_a_words(int op, int nw) {
  switch (op) {
    case SC_FL_MUL: case SC_FL_CANON4: return 9;
    case SC_DIGEST: return 16;
    case SC_NONCE: return 32;
    case SC_WIDE: return nw;
    case SC_EUCLID: return 32;
    default: return 8;
  }
}
BJJ_HD int sc_b_words(int op) { return op == SC_FL_MUL ? 9 : op == SC_VERIFY_C ? 9 : 0; }
BJJ_HD int sc_out_words(int op) {
  switch (op) {
    case SC_FL_MUL: case SC_FL_CANON4: return 9;
    case SC_SHORT_PAIR: return 17;
    case SC_EUCLID: return 18;
    default: return 8;
  }
}
BJJ_HD Fr sc_raw(const u32* p) { Fr f; for (int i = 0; i < NL; i++) f.v[i] = p[i]; return f; }
BJJ_HD void sc_put_raw(u32* p, const Fr& f) { for (int i = 0; i < NL; i++) p[i] = f.v[i]; }

BJJ_HD void sc_item(int op, const u32* a, const u32* b, u32* o, int nw, const Consts& K) {
  switch (op) {
    case SC_MOD_L: scalar_mod_l(a, o, K); break;
    case SC_MOD_ORDER: scalar_mod_order(a, o, K); break;
    case SC_PLAIN_MOD_L: fr_to_words(plain_mod_l(fr_from_words(a), K), o); break;
    case SC_FL_MUL: sc_put_raw(o, fl_mul(sc_raw(a), sc_raw(b), K)); break;
    case SC_FL_CANON4: sc_put_raw(o, fl_canon4(sc_raw(a), K)); break;
    case SC_DIGEST: fr_to_words(digest_mod_l(a, K), o); break;
    case SC_NONCE: fr_to_words(nonce_mod_l(a, K), o); break;
    case SC_WIDE: wide_scalar_mod_order(a, nw, o, K); break;
    case SC_VERIFY_C: fr_to_words(verify_fb_scalar(a, fr_from_words(b), b[8] != 0, K), o); break;
    case SC_SHORT_PAIR: {
      Fr u, vm;
      bool neg;
      lattice_short_pair(fr_from_words(a), u, vm, neg, K);
      fr_to_words(u, o); fr_to_words(vm, o + 8); o[16] = neg ? 1u : 0u;
      break;
    }
    case SC_EUCLID: {
      Fr r0 = fr_from_words(a), t0 = fr_from_words(a + 16);
      euclid_partial_step(r0, fr_from_words(a + 8), t0, fr_from_words(a + 24));
      sc_put_raw(o, r0); sc_put_raw(o + 9, t0);
      break;
    }
    default: break;
  }
}

}  // namespace bjj
