// TEST-ONLY: one item of the shipped field layer (csrc/fr.hpp: the additive forms, fr_reduce_weak, fr_canon / fr_is_zero /
// fr_eq, the word and Montgomery conversions) and of the square-root and codec block of csrc/bjj_device.hpp (fr_sqrt,
// plain_gt_halfq, words_ge_modulus / words_gt_modulus, decompress_item, compress_item) plus ref_on_curve (csrc/curve.hpp), on
// raw limbs or words chosen by the test.  The same body runs on the GPU (field.hip -> libbjj_field_test.so) and on the CPU
// (tests/emul/emul_field_ops.cpp: emul_field_op, with the BJJ_ASSERTs live), so tests/test_gpu_field_ops.py can compare the
// two builds bit for bit and both against the plain integers of tests/field_ref.py.  Every op calls the function the kernels
// call; nothing here restates the arithmetic.  The includer provides csrc/bjj_device.hpp.
#pragma once

namespace bjj {

enum {
  FO_ADD = 0,            // a, b: 9 raw limbs                   out: fr_add, 9 raw limbs
  FO_DBL = 1,            // a: 9 raw limbs                      out: fr_dbl
  FO_ADD_LAZY = 2,       // a, b: 9 raw limbs                   out: fr_add_lazy
  FO_SUB = 3,            // a, b: 9 raw limbs                   out: fr_sub
  FO_NEG = 4,            // a: 9 raw limbs                      out: fr_neg
  FO_SUB8 = 5,           // a, b: 9 raw limbs                   out: fr_sub8
  FO_SUB_LAZY = 6,       // a, b: 9 raw limbs                   out: fr_sub_lazy
  FO_SUB8_OF_LAZY = 7,   // a, b: 9 raw limbs                   out: fr_sub8_of_lazy
  FO_REDUCE_WEAK = 8,    // a: 9 raw limbs                      out: fr_reduce_weak
  FO_CANON = 9,          // a: 9 raw limbs                      out: fr_canon
  FO_IS_ZERO = 10,       // a: 9 raw limbs                      out: 1 word, fr_is_zero
  FO_EQ = 11,            // a, b: 9 raw limbs                   out: 1 word, fr_eq
  FO_FROM_WORDS = 12,    // a: 8 words                          out: fr_from_words, 9 raw limbs
  FO_TO_WORDS = 13,      // a: 9 raw limbs                      out: fr_to_words, 8 words
  FO_TO_MONT = 14,       // a: 8 words                          out: fr_to_mont_words, 9 raw limbs
  FO_FROM_MONT = 15,     // a: 9 raw limbs                      out: fr_from_mont_words, 8 words
  FO_GT_HALFQ = 16,      // a: 9 raw limbs (canonical)          out: 1 word, plain_gt_halfq
  FO_WORDS_GE_R = 17,    // a: 8 words                          out: 1 word, words_ge_modulus
  FO_WORDS_GT_R = 18,    // a: 8 words                          out: 1 word, words_gt_modulus
  FO_SQRT = 19,          // a: 9 raw limbs (Montgomery)         out: 1 word flag, then the root as 9 raw limbs
  FO_ON_CURVE = 20,      // a: x, b: y, 9 raw limbs (Montgomery) out: 1 word, ref_on_curve
  FO_DECOMPRESS = 21,    // a: 8 words                          out: 1 word flag, x (8 words), y (8 words): decompress_item
  FO_COMPRESS = 22,      // a: x, b: y, 8 words each            out: compress_item, 8 words
  FO_NOPS = 23
};
// record widths in words; which = 0: a, 1: b (0: the op has no second operand), 2: out
BJJ_HD int field_words(int op, int which) {
  if (which == 0) {
    switch (op) {
      case FO_FROM_WORDS: case FO_TO_MONT: case FO_WORDS_GE_R: case FO_WORDS_GT_R: case FO_DECOMPRESS: case FO_COMPRESS: return 8;
      default: return 9;
    }
  }
  if (which == 1) {
    switch (op) {
      case FO_ADD: case FO_ADD_LAZY: case FO_SUB: case FO_SUB8: case FO_SUB_LAZY: case FO_SUB8_OF_LAZY: case FO_EQ: case FO_ON_CURVE:
        return 9;
      case FO_COMPRESS: return 8;
      default: return 0;
    }
  }
  switch (op) {
    case FO_IS_ZERO: case FO_EQ: case FO_GT_HALFQ: case FO_WORDS_GE_R: case FO_WORDS_GT_R: case FO_ON_CURVE: return 1;
    case FO_TO_WORDS: case FO_FROM_MONT: case FO_COMPRESS: return 8;
    case FO_SQRT: return 10;
    case FO_DECOMPRESS: return 17;
    default: return 9;
  }
}
BJJ_HD Fr fo_raw(const u32* p) { Fr f; for (int i = 0; i < NL; i++) f.v[i] = p[i]; return f; }
BJJ_HD void fo_put_raw(u32* p, const Fr& f) { for (int i = 0; i < NL; i++) p[i] = f.v[i]; }

BJJ_HD void field_op(int op, const u32* a, const u32* b, u32* o, const Consts& K) {
  switch (op) {
    case FO_ADD: fo_put_raw(o, fr_add(fo_raw(a), fo_raw(b))); break;
    case FO_DBL: fo_put_raw(o, fr_dbl(fo_raw(a))); break;
    case FO_ADD_LAZY: fo_put_raw(o, fr_add_lazy(fo_raw(a), fo_raw(b))); break;
    case FO_SUB: fo_put_raw(o, fr_sub(fo_raw(a), fo_raw(b))); break;
    case FO_NEG: fo_put_raw(o, fr_neg(fo_raw(a))); break;
    case FO_SUB8: fo_put_raw(o, fr_sub8(fo_raw(a), fo_raw(b))); break;
    case FO_SUB_LAZY: fo_put_raw(o, fr_sub_lazy(fo_raw(a), fo_raw(b))); break;
    case FO_SUB8_OF_LAZY: fo_put_raw(o, fr_sub8_of_lazy(fo_raw(a), fo_raw(b))); break;
    case FO_REDUCE_WEAK: fo_put_raw(o, fr_reduce_weak(fo_raw(a))); break;
    case FO_CANON: fo_put_raw(o, fr_canon(fo_raw(a))); break;
    case FO_IS_ZERO: o[0] = fr_is_zero(fo_raw(a)) ? 1u : 0u; break;
    case FO_EQ: o[0] = fr_eq(fo_raw(a), fo_raw(b)) ? 1u : 0u; break;
    case FO_FROM_WORDS: fo_put_raw(o, fr_from_words(a)); break;
    case FO_TO_WORDS: fr_to_words(fo_raw(a), o); break;
    case FO_TO_MONT: fo_put_raw(o, fr_to_mont_words(a)); break;
    case FO_FROM_MONT: fr_from_mont_words(fo_raw(a), o); break;
    case FO_GT_HALFQ: o[0] = plain_gt_halfq(fo_raw(a), K) ? 1u : 0u; break;
    case FO_WORDS_GE_R: o[0] = words_ge_modulus(a) ? 1u : 0u; break;
    case FO_WORDS_GT_R: o[0] = words_gt_modulus(a) ? 1u : 0u; break;
    case FO_SQRT: {
      Fr root;
      o[0] = fr_sqrt(fo_raw(a), root, K) ? 1u : 0u;
      fo_put_raw(o + 1, root);
      break;
    }
    case FO_ON_CURVE: o[0] = ref_on_curve(fo_raw(a), fo_raw(b), K) ? 1u : 0u; break;
    case FO_DECOMPRESS: o[0] = decompress_item(a, o + 1, o + 9, K) ? 1u : 0u; break;
    case FO_COMPRESS: compress_item(a, b, o, K); break;
    default: break;
  }
}

}  // namespace bjj
