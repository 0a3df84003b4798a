// TEST-ONLY: one item of the four-lane ("quad") point arithmetic of csrc/k_small.hip -- quad_dbl, quad_add, quad_entry,
// quad_lift, quad_from_ref_affine, qtbl_build / qtbl_store / qtbl_load, quad_walk, quad_walk_joint, quad_affine,
// quad_is_identity, qfb_load, quad_mul_fixed_base, quad_add_fixed_base -- on raw limbs chosen by the test, the four lanes
// 4k .. 4k + 3 of a wave holding item k as they do in the short-call kernels.  Device only: the functions move operands with DPP
// quad permutes and wave shuffles, so there is no CPU build of this dispatcher; tests/test_gpu_quad_ops.py holds the results
// against the plain integers of tests/quad_ref.py and against the one-item-per-lane functions of libbjj_curve_test.so.
// Every op calls the function the kernels call, in the sequence the kernels call it; nothing here restates the arithmetic.
// The includer provides csrc/k_small.hip.
#pragma once

// records are raw limbs, one field element = 9 words.  Ext = X, Y, Z, T (36 words): lane q holds element q.  PNiels = ymx, ypx,
// t2d, z2 (36 words), the order of tests/devfuzz/curve_ops.hpp: the quad's lanes 0, 1, 2, 3 hold Y-X, Y+X, 2Z, 2D'T, that is
// elements 0, 1, 3, 2 of the record (qd_pn).  Flags and counts are one word each; scalars are 32-bit words, little-endian.
enum {
  QD_DBL = 0,         // a: Ext                                  out: quad_dbl, Ext
  QD_DBL4 = 1,        //                                         out: quad_dbl four times, as in one window
  QD_ADD = 2,         // a: Ext  b: PNiels, k (0..8), neg        out: qtbl_store of the entry at slot k, quad_add(q, a, qtbl_load(tbl, neg ? -k : k, q)), Ext
  QD_ENTRY = 3,       // a: Ext                                  out: quad_entry, PNiels
  QD_LIFT_T = 4,      // a: PNiels, k, neg                       out: the entry through the table as in QD_ADD, quad_lift<true>, Ext
  QD_LIFT = 5,        //                                         out: quad_lift<false> (T: the zero limbs)
  QD_FROM_REF = 6,    // a: x  b: y                              out: quad_from_ref_affine, Ext
  QD_TABLE = 7,       // a: Ext                                  out: qtbl_build, then qtbl_load of d = -8 .. 8: 17 PNiels
  QD_WALK = 8,        // a: Ext  b: 8 words, need                out: qtbl_build, recode_signed4, jw = wave_max_int(need), quad_lift<false> of window
                      //                                              jw - 1, quad_walk over jw - 2 .. 0: Ext, then jw as every lane of the quad has it (4 words)
  QD_WALK_JOINT = 9,  // a: 2 Ext  b: 2 x 8 words, need          out: two tables, quad_lift<true> of u's window jw - 1, quad_add of v's, quad_walk_joint: Ext, jw x 4
  QD_AFFINE = 10,     // a: Ext                                  out: quad_affine(q, a, fr_inv(quad_bcast<2>(a))): x, y as 8 words each (fr_to_words)
  QD_IS_IDENTITY = 11,// a: Ext                                  out: 1 word, quad_is_identity
  QD_FB_LOAD = 12,    // a: slot, neg                            out: qfb_load over the fixed-base table, PNiels order (z2 = lane 2's constant)
  QD_FB_MUL = 13,     // a: 8 words (< l)                        out: quad_mul_fixed_base, Ext
  QD_FB_ADD = 14,     // a: 8 words (< l)  b: Ext                out: quad_add_fixed_base, Ext
  QD_NOPS = 15
};
// the fixed-base table of the QD_FB ops: the narrowest window the tests of the short fixed-base calls use
constexpr int QD_FB_W = 8;
constexpr int QD_FB_NWIN = (252 + QD_FB_W - 1) / QD_FB_W;                       // fixed_nwin
constexpr int QD_FB_STRIDE = (1 << (QD_FB_W - 1)) + 1;                         // fixed_stride
constexpr int QD_FB_SLOTS = QD_FB_NWIN * QD_FB_STRIDE;
constexpr int QD_FB_WORDS = (QD_FB_SLOTS + QD_FB_NWIN) * NIELS_WORDS;         // the table, then the bases of its windows

// record widths in words; which = 0: a, 1: b (0: the op has no second operand), 2: out
static inline __host__ __device__ int quad_words(int op, int which) {
  if (which == 0) {
    switch (op) {
      case QD_LIFT_T: case QD_LIFT: return 38;
      case QD_FROM_REF: return 9;
      case QD_WALK_JOINT: return 72;
      case QD_FB_LOAD: return 2;
      case QD_FB_MUL: case QD_FB_ADD: return 8;
      default: return 36;
    }
  }
  if (which == 1) {
    switch (op) {
      case QD_ADD: return 38;
      case QD_FROM_REF: case QD_WALK: return 9;
      case QD_WALK_JOINT: return 17;
      case QD_FB_ADD: return 36;
      default: return 0;
    }
  }
  switch (op) {
    case QD_TABLE: return 17 * 36;
    case QD_WALK: case QD_WALK_JOINT: return 40;
    case QD_AFFINE: return 16;
    case QD_IS_IDENTITY: return 1;
    default: return 36;
  }
}
__device__ __forceinline__ Fr qd_raw(const u32* p) { Fr f; for (int i = 0; i < NL; i++) f.v[i] = p[i]; return f; }
__device__ __forceinline__ void qd_put(u32* p, const Fr& f) { for (int i = 0; i < NL; i++) p[i] = f.v[i]; }
__device__ __forceinline__ int qd_pn(int q) { return q == 2 ? 3 : q == 3 ? 2 : q; }   // the PNiels record's element of lane q
__device__ __forceinline__ int qd_need(u32 v) { return v < 1u ? 1 : v > 64u ? 64 : (int)v; }

// The four lanes of a quad call this together (q = lane & 3) with the quad's records; o is null on the quads beyond the batch,
// which repeat the last item and store nothing.  tbl: this quad's two tables in LDS; fb: the fixed-base table (QD_FB_WORDS).
// The op is the same on every lane of the workgroup, so the barriers inside are reached by all of them.
__device__ __forceinline__ void quad_op(int op, int q, const u32* a, const u32* b, u32* o, u32* tbl, const u32* __restrict__ fb) {
  switch (op) {
    case QD_DBL: {
      const Fr r = quad_dbl(q, qd_raw(a + 9 * q));
      if (o) qd_put(o + 9 * q, r);
      break;
    }
    case QD_DBL4: {
      Fr acc = qd_raw(a + 9 * q);
#pragma unroll 1
      for (int k = 0; k < 4; k++) acc = quad_dbl(q, acc);
      if (o) qd_put(o + 9 * q, acc);
      break;
    }
    case QD_ADD: case QD_LIFT_T: case QD_LIFT: {
      const u32* ent = op == QD_ADD ? b : a;
      const int k = (int)(ent[36] % 9u), d = ent[37] ? -k : k;
      qtbl_store(tbl, k, q, qd_raw(ent + 9 * qd_pn(q)));
      __syncthreads();
      const Fr e = qtbl_load(tbl, d, q);
      const Fr r = op == QD_ADD ? quad_add(q, qd_raw(a + 9 * q), e) : op == QD_LIFT_T ? quad_lift<true>(q, e) : quad_lift<false>(q, e);
      if (o) qd_put(o + 9 * q, r);
      break;
    }
    case QD_ENTRY: {
      const Fr r = quad_entry(q, qd_raw(a + 9 * q));
      if (o) qd_put(o + 9 * qd_pn(q), r);
      break;
    }
    case QD_FROM_REF: {
      const Fr r = quad_from_ref_affine(q, qd_raw(a), qd_raw(b));
      if (o) qd_put(o + 9 * q, r);
      break;
    }
    case QD_TABLE: {
      qtbl_build(q, tbl, qd_raw(a + 9 * q));
      __syncthreads();
#pragma unroll 1
      for (int d = -8; d <= 8; d++) {
        const Fr e = qtbl_load(tbl, d, q);
        if (o) qd_put(o + 36 * (d + 8) + 9 * qd_pn(q), e);
      }
      break;
    }
    case QD_WALK: {   // bjj_k_mul_var_base_quad (need = 64), bjj_k_eddsa_verify_small's waves, bjj_k_schnorr_verify_small
      qtbl_build(q, tbl, qd_raw(a + 9 * q));
      __syncthreads();
      u32 t[8];
      recode_signed4(b, t);
      const int jw = wave_max_int(qd_need(b[8]));
      Fr acc = quad_lift<false>(q, qtbl_load(tbl, signed4_digit(t, jw - 1), q));
      acc = quad_walk(tbl, t, jw - 2, q, acc);
      if (o) { qd_put(o + 9 * q, acc); o[36 + q] = (u32)jw; }
      break;
    }
    case QD_WALK_JOINT: {   // bjj_k_eddsa_verify_small_joint
      u32* tbl2 = tbl + QTBL_ITEM_WORDS;
      qtbl_build(q, tbl, qd_raw(a + 9 * q));
      qtbl_build(q, tbl2, qd_raw(a + 36 + 9 * q));
      __syncthreads();
      u32 tu[8], tv[8];
      recode_signed4(b, tu);
      recode_signed4(b + 8, tv);
      const int jw = wave_max_int(qd_need(b[16]));
      Fr acc = quad_lift<true>(q, qtbl_load(tbl, signed4_digit(tu, jw - 1), q));
      acc = quad_add(q, acc, qtbl_load(tbl2, signed4_digit(tv, jw - 1), q));
      acc = quad_walk_joint(tbl, tbl2, tu, tv, jw - 2, q, acc);
      if (o) { qd_put(o + 9 * q, acc); o[36 + q] = (u32)jw; }
      break;
    }
    case QD_AFFINE: {
      const Fr c = qd_raw(a + 9 * q);
      const Fr v = quad_affine(q, c, fr_inv(quad_bcast<2>(c)));
      if (o && q < 2) {
        u32 w[8];
        fr_to_words(v, w);
#pragma unroll
        for (int i = 0; i < 8; i++) o[8 * q + i] = w[i];
      }
      break;
    }
    case QD_IS_IDENTITY: {
      const bool id = quad_is_identity(qd_raw(a + 9 * q));
      if (o && q == 0) o[0] = id ? 1u : 0u;
      break;
    }
    case QD_FB_LOAD: {
      const Fr r = qfb_load(fb, (size_t)(a[0] % (u32)QD_FB_SLOTS), a[1] != 0, q);
      if (o) qd_put(o + 9 * qd_pn(q), r);
      break;
    }
    case QD_FB_MUL: {
      const Fr r = quad_mul_fixed_base(fb, QD_FB_W, QD_FB_NWIN, a, q);
      if (o) qd_put(o + 9 * q, r);
      break;
    }
    case QD_FB_ADD: {
      const Fr r = quad_add_fixed_base(fb, QD_FB_W, QD_FB_NWIN, a, q, qd_raw(b + 9 * q));
      if (o) qd_put(o + 9 * q, r);
      break;
    }
    default: break;
  }
}
