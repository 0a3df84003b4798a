// TEST-ONLY: one item of the shipped group-law layer (csrc/curve.hpp: ext_madd / ext_add_pn / ext_dbl, the conversions, ref_add)
// and of the per-lane table, ladder and fixed-table code of csrc/bjj_device.hpp (niels_cneg_lazy, pniels_cneg, vb_build_table,
// vb_table_load, vb_mul_windowed, ref_mul_scalar, var_base_item, fixed_table_entry / _chain / _check_slot) on raw limbs chosen
// by the test.  The same body runs on the GPU (curve.hip -> libbjj_curve_test.so and, with BJJ_PNIELS_LAYOUT=1,
// libbjj_curve_test_packed.so) and on the CPU (tests/emul/emul_curve_ops.cpp: emul_curve_op, with the BJJ_ASSERTs live), so
// tests/test_gpu_curve_ops.py can compare the two builds bit for bit and both against the plain integers of
// tests/curve_ref.py.  Every op calls the function the kernels call; nothing here restates the arithmetic.  The includer
// provides csrc/bjj_device.hpp.
#pragma once

namespace bjj {

// records are raw limbs: Ext = X, Y, Z, T (36 words), Niels = ymx, ypx, t2d (27), PNiels = ymx, ypx, t2d, z2 (36), RefProj = x, y,
// z (27); "neg", "need_t" and the like are one word each, 0 or 1; scalars are 32-bit words, little-endian
enum {
  CO_MADD_T = 0,        // a: Ext  b: Niels, neg            out: ext_madd<true>(a, niels_cneg_lazy(b, neg)), Ext
  CO_MADD = 1,          //                                  out: ext_madd<false>
  CO_ADDPN_T = 2,       // a: Ext  b: PNiels, neg           out: ext_add_pn(a, pniels_cneg(b, neg), true), Ext
  CO_ADDPN = 3,         //                                  out: ext_add_pn(.., false)
  CO_DBL_T = 4,         // a: Ext                           out: ext_dbl<true>
  CO_DBL = 5,           //                                  out: ext_dbl<false>
  CO_WINDOW = 6,        // a: Ext  b: PNiels, neg, need_t   out: one window of vb_mul_windowed: ext_dbl<false> x 3, ext_dbl<true>,
                        //                                       ext_add_pn(., pniels_cneg(b, neg), need_t)
  CO_TO_PNIELS = 7,     // a: Ext                           out: ext_to_pniels, PNiels
  CO_PN2EXT_T = 8,      // a: PNiels, neg                   out: pniels_to_ext(pniels_cneg(a, neg), true), Ext
  CO_PN2EXT = 9,        //                                  out: pniels_to_ext(.., false)
  CO_LIFT_T = 10,       // a: Niels                         out: niels_lift(a, tform = true), Ext
  CO_LIFT = 11,         //                                  out: niels_lift(a, tform = false)
  CO_EQ_NIELS = 12,     // a: Ext  b: Niels                 out: 1 word, ext_equals_niels
  CO_NFA_T = 13,        // a: x  b: y (9 limbs each)        out: niels_from_affine(x, y, tform = true), Niels
  CO_NFA = 14,          //                                  out: niels_from_affine(x, y, tform = false)
  CO_FROM_REF = 15,     // a: x  b: y                       out: ext_from_ref_affine, Ext
  CO_REF_ADD = 16,      // a, b: RefProj                    out: ref_add, RefProj
  CO_REF_MUL8 = 17,     // a: x, y  b: 8 words              out: ref_mul_scalar(nw = 8): x, y
  CO_REF_MUL2 = 18,     // a: x, y  b: 2 words              out: ref_mul_scalar(nw = 2): x, y
  CO_VAR_BASE = 19,     // a: x, y  b: 8 words              out: var_base_item (both paths), Ext
  CO_TABLE = 20,        // a: Ext                           out: vb_build_table(affine_base = false), then vb_table_load of 0 .. 8: 9 PNiels
  CO_TABLE_AFFINE = 21, // a: Ext with Z == 1               out: the same with affine_base = true
  CO_MULW64 = 22,       // a: Ext  b: 8 words (< 2^254)     out: vb_build_table, vb_mul_windowed(nwin = 64, final_t = false), Ext
  CO_MULW64_T = 23,     //                                  out: final_t = true
  CO_MULW2 = 24,        // a: Ext  b: 8 words (< 2^6)       out: nwin = 2, final_t = false
  CO_MULW2_T = 25,
  CO_MULW1 = 26,        // a: Ext  b: 8 words (< 2^2)       out: nwin = 1, final_t = false
  CO_MULW1_T = 27,
  CO_FIXED_ENTRY = 28,  // a: k, j, tform                   out: fixed_table_entry(k, j, W = 4, tform), Niels
  CO_FIXED_CHAIN = 29,  // a: chain length (1 .. 9)         out: per slot of a W = 4 table of CO_FT_NWIN windows built by fixed_table_chain
                        //                                       (bases from fixed_table_entry(1, j)): the entry (Niels), then per slot
                        //                                       the count of fixed_table_check_slot
  CO_FIXED_FLIP = 30,   // a: chain length, slot, word, bit out: 2 words: the table as above with that bit of that slot flipped:
                        //                                       fixed_table_check_slot of the slot, and of the slot before it in
                        //                                       the same window (0 when the slot is the window's first)
  CO_NOPS = 31
};
constexpr int CO_FT_W = 4, CO_FT_NWIN = 3;
constexpr int CO_FT_SLOTS = CO_FT_NWIN * 9;                                  // fixed_stride(4) = 9 entries per window
constexpr int CO_FT_WORDS = (CO_FT_SLOTS + CO_FT_NWIN) * NIELS_WORDS;       // the table, then the bases

// record widths in words; which = 0: a, 1: b (0: the op has no second operand), 2: out, 3: per-item scratch (16-byte aligned)
BJJ_HD int curve_words(int op, int which) {
  if (which == 0) {
    switch (op) {
      case CO_PN2EXT_T: case CO_PN2EXT: return 37;
      case CO_LIFT_T: case CO_LIFT: case CO_REF_ADD: return 27;
      case CO_NFA_T: case CO_NFA: case CO_FROM_REF: return 9;
      case CO_REF_MUL8: case CO_REF_MUL2: case CO_VAR_BASE: return 18;
      case CO_FIXED_ENTRY: return 3;
      case CO_FIXED_CHAIN: return 1;
      case CO_FIXED_FLIP: return 4;
      default: return 36;
    }
  }
  if (which == 1) {
    switch (op) {
      case CO_MADD_T: case CO_MADD: return 28;
      case CO_ADDPN_T: case CO_ADDPN: return 37;
      case CO_WINDOW: return 38;
      case CO_EQ_NIELS: case CO_REF_ADD: return 27;
      case CO_NFA_T: case CO_NFA: case CO_FROM_REF: return 9;
      case CO_REF_MUL8: case CO_VAR_BASE: case CO_MULW64: case CO_MULW64_T: case CO_MULW2: case CO_MULW2_T: case CO_MULW1: case CO_MULW1_T:
        return 8;
      case CO_REF_MUL2: return 2;
      default: return 0;
    }
  }
  if (which == 2) {
    switch (op) {
      case CO_EQ_NIELS: return 1;
      case CO_NFA_T: case CO_NFA: case CO_REF_ADD: case CO_FIXED_ENTRY: return 27;
      case CO_REF_MUL8: case CO_REF_MUL2: return 18;
      case CO_TABLE: case CO_TABLE_AFFINE: return 9 * 36;
      case CO_FIXED_CHAIN: return CO_FT_SLOTS * 28;
      case CO_FIXED_FLIP: return 2;
      default: return 36;
    }
  }
  switch (op) {
    case CO_VAR_BASE: case CO_TABLE: case CO_TABLE_AFFINE: case CO_MULW64: case CO_MULW64_T: case CO_MULW2: case CO_MULW2_T: case CO_MULW1:
    case CO_MULW1_T:
      return VB_TABLE_WORDS_MAX;
    case CO_FIXED_CHAIN: case CO_FIXED_FLIP: return CO_FT_WORDS;
    default: return 0;
  }
}
BJJ_HD Fr co_raw(const u32* p) { Fr f; for (int i = 0; i < NL; i++) f.v[i] = p[i]; return f; }
BJJ_HD void co_put_raw(u32* p, const Fr& f) { for (int i = 0; i < NL; i++) p[i] = f.v[i]; }
BJJ_HD Ext co_ext(const u32* p) { Ext e; e.X = co_raw(p); e.Y = co_raw(p + 9); e.Z = co_raw(p + 18); e.T = co_raw(p + 27); return e; }
BJJ_HD void co_put_ext(u32* p, const Ext& e) { co_put_raw(p, e.X); co_put_raw(p + 9, e.Y); co_put_raw(p + 18, e.Z); co_put_raw(p + 27, e.T); }
BJJ_HD Niels co_niels(const u32* p) { Niels n; n.ymx = co_raw(p); n.ypx = co_raw(p + 9); n.t2d = co_raw(p + 18); return n; }
BJJ_HD void co_put_niels(u32* p, const Niels& n) { co_put_raw(p, n.ymx); co_put_raw(p + 9, n.ypx); co_put_raw(p + 18, n.t2d); }
BJJ_HD PNiels co_pniels(const u32* p) {
  PNiels n; n.ymx = co_raw(p); n.ypx = co_raw(p + 9); n.t2d = co_raw(p + 18); n.z2 = co_raw(p + 27); return n;
}
BJJ_HD void co_put_pniels(u32* p, const PNiels& n) {
  co_put_raw(p, n.ymx); co_put_raw(p + 9, n.ypx); co_put_raw(p + 18, n.t2d); co_put_raw(p + 27, n.z2);
}
// the W = 4 table of CO_FT_NWIN windows in scr: bases by the independent definition, entries in chains of `chain` digits
// per window, the way the build kernel cuts them
BJJ_HD void co_fixed_table(u32* scr, u32 chain, const Consts& K) {
  u32* bases = scr + CO_FT_SLOTS * NIELS_WORDS;
  const u32 stride = (u32)fixed_stride(CO_FT_W);
  if (chain < 1) chain = 1;
  if (chain > stride) chain = stride;
#pragma unroll 1
  for (int j = 0; j < CO_FT_NWIN; j++) {
    store_niels(bases + j * NIELS_WORDS, fixed_table_entry(1u, j, CO_FT_W, K));
#pragma unroll 1
    for (u32 k0 = 0; k0 < stride; k0 += chain) {
      const u32 cnt = stride - k0 < chain ? stride - k0 : chain;
      fixed_table_chain(scr, load_niels(bases + j * NIELS_WORDS), (size_t)j * stride + k0, k0, cnt, CO_FT_W, K);
    }
  }
}

BJJ_HD void curve_op(int op, const u32* a, const u32* b, u32* o, u32* scr, const Consts& K) {
  switch (op) {
    case CO_MADD_T: co_put_ext(o, ext_madd<true>(co_ext(a), niels_cneg_lazy(co_niels(b), b[27] != 0))); break;
    case CO_MADD: co_put_ext(o, ext_madd<false>(co_ext(a), niels_cneg_lazy(co_niels(b), b[27] != 0))); break;
    case CO_ADDPN_T: co_put_ext(o, ext_add_pn(co_ext(a), pniels_cneg(co_pniels(b), b[36] != 0), true)); break;
    case CO_ADDPN: co_put_ext(o, ext_add_pn(co_ext(a), pniels_cneg(co_pniels(b), b[36] != 0), false)); break;
    case CO_DBL_T: co_put_ext(o, ext_dbl<true>(co_ext(a))); break;
    case CO_DBL: co_put_ext(o, ext_dbl<false>(co_ext(a))); break;
    case CO_WINDOW: {
      Ext acc = co_ext(a);
#pragma unroll 1
      for (int k = 0; k < 3; k++) acc = ext_dbl<false>(acc);
      acc = ext_dbl<true>(acc);
      co_put_ext(o, ext_add_pn(acc, pniels_cneg(co_pniels(b), b[36] != 0), b[37] != 0));
      break;
    }
    case CO_TO_PNIELS: co_put_pniels(o, ext_to_pniels(co_ext(a), K)); break;
    case CO_PN2EXT_T: co_put_ext(o, pniels_to_ext(pniels_cneg(co_pniels(a), a[36] != 0), K, true)); break;
    case CO_PN2EXT: co_put_ext(o, pniels_to_ext(pniels_cneg(co_pniels(a), a[36] != 0), K, false)); break;
    case CO_LIFT_T: co_put_ext(o, niels_lift(co_niels(a), K, true)); break;
    case CO_LIFT: co_put_ext(o, niels_lift(co_niels(a), K, false)); break;
    case CO_EQ_NIELS: o[0] = ext_equals_niels(co_ext(a), co_niels(b)) ? 1u : 0u; break;
    case CO_NFA_T: co_put_niels(o, niels_from_affine(co_raw(a), co_raw(b), K, true)); break;
    case CO_NFA: co_put_niels(o, niels_from_affine(co_raw(a), co_raw(b), K, false)); break;
    case CO_FROM_REF: co_put_ext(o, ext_from_ref_affine(co_raw(a), co_raw(b), K)); break;
    case CO_REF_ADD: {
      RefProj p, q;
      p.x = co_raw(a); p.y = co_raw(a + 9); p.z = co_raw(a + 18);
      q.x = co_raw(b); q.y = co_raw(b + 9); q.z = co_raw(b + 18);
      const RefProj r = ref_add(p, q, K);
      co_put_raw(o, r.x); co_put_raw(o + 9, r.y); co_put_raw(o + 18, r.z);
      break;
    }
    case CO_REF_MUL8: case CO_REF_MUL2: {
      Fr ox, oy;
      ref_mul_scalar(co_raw(a), co_raw(a + 9), b, op == CO_REF_MUL8 ? 8 : 2, ox, oy, K);
      co_put_raw(o, ox); co_put_raw(o + 9, oy);
      break;
    }
    case CO_VAR_BASE: co_put_ext(o, var_base_item(co_raw(a), co_raw(a + 9), b, scr, K)); break;
    case CO_TABLE: case CO_TABLE_AFFINE: {
      vb_build_table(co_ext(a), scr, K, op == CO_TABLE_AFFINE);
#pragma unroll 1
      for (u32 k = 0; k <= 8; k++) co_put_pniels(o + 36 * k, vb_table_load(scr, k));
      break;
    }
    case CO_MULW64: case CO_MULW64_T: case CO_MULW2: case CO_MULW2_T: case CO_MULW1: case CO_MULW1_T: {
      const int nwin = op <= CO_MULW64_T ? 64 : op <= CO_MULW2_T ? 2 : 1;
      const bool final_t = op == CO_MULW64_T || op == CO_MULW2_T || op == CO_MULW1_T;
      vb_build_table(co_ext(a), scr, K, false);
      co_put_ext(o, vb_mul_windowed(scr, b, nwin, K, final_t));
      break;
    }
    case CO_FIXED_ENTRY: co_put_niels(o, fixed_table_entry(a[0], (int)a[1], CO_FT_W, K, a[2] != 0)); break;
    case CO_FIXED_CHAIN: {
      co_fixed_table(scr, a[0], K);
      const u32* bases = scr + CO_FT_SLOTS * NIELS_WORDS;
#pragma unroll 1
      for (int s = 0; s < CO_FT_SLOTS; s++) {
        co_put_niels(o + 28 * s, load_niels(scr + s * NIELS_WORDS));
        o[28 * s + 27] = (u32)fixed_table_check_slot(scr, bases, s / 9, (u32)(s % 9), CO_FT_W, CO_FT_NWIN, K);
      }
      break;
    }
    case CO_FIXED_FLIP: {
      co_fixed_table(scr, a[0], K);
      const u32* bases = scr + CO_FT_SLOTS * NIELS_WORDS;
      const u32 s = a[1] % CO_FT_SLOTS, w = a[2] % NIELS_WORDS, bit = a[3] & 31u;
      scr[s * NIELS_WORDS + w] ^= 1u << bit;
      o[0] = (u32)fixed_table_check_slot(scr, bases, (int)(s / 9), s % 9, CO_FT_W, CO_FT_NWIN, K);
      o[1] = (s % 9) ? (u32)fixed_table_check_slot(scr, bases, (int)(s / 9), s % 9 - 1, CO_FT_W, CO_FT_NWIN, K) : 0u;
      break;
    }
    default: break;
  }
}

}  // namespace bjj
