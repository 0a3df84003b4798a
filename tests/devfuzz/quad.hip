// TEST-ONLY library (not part of libbjj_hip.so): the short-call kernel unit csrc/k_small.hip as it ships, compiled with the
// product's flags, and one kernel beside its own that hands raw limbs to the four-lane point arithmetic in it (quad_ops.hpp).
// That arithmetic is a second implementation of the group law, the table of 0 .. 8 P, the signed-window ladder and the affine
// epilogue -- operands routed by fr_select on the lane's position, moved by DPP quad permutes, with lazy forms of its own --
// which the C ABI reaches only with canonical affine inputs; tests/test_gpu_quad_ops.py drives it with every representative
// and every edge Z, as tests/test_gpu_curve_ops.py drives the one-item-per-lane forms through curve.hip.
// The kernel has the shape of bjj_k_mul_var_base_quad: workgroups of one wave = 16 items, lane 4k + q on coordinate q of item k,
// the tables in LDS in the product's layout (two per quad, as bjj_k_eddsa_verify_small_joint keeps them), the quads beyond the
// batch repeating the last item and storing nothing.
#include "../../babyjubjub-rs_amd/csrc/k_small.hip"
#include "quad_ops.hpp"

__global__ void __launch_bounds__(BJJ_QUAD_BLOCK) qd_kernel(int op, const u32* __restrict__ a, const u32* __restrict__ b, u32* __restrict__ out,
                                                            const u32* __restrict__ fb, size_t n) {
  __shared__ u32 tbl_all[BJJ_QUAD_ITEMS * 2 * QTBL_ITEM_WORDS];   // 41.5 KB
  const int lane = threadIdx.x, q = lane & 3;
  u32* tbl = tbl_all + (lane >> 2) * 2 * QTBL_ITEM_WORDS;
  const size_t item = (size_t)blockIdx.x * BJJ_QUAD_ITEMS + (size_t)(lane >> 2);
  const bool live = item < n;
  const size_t i = live ? item : n - 1;          // a quad beyond the batch repeats the last item and stores nothing
  const size_t wa = quad_words(op, 0), wb = quad_words(op, 1), wo = quad_words(op, 2);
  quad_op(op, q, a + i * wa, b + i * wb, live ? out + i * wo : nullptr, tbl, fb);
}

// the fixed-base table of the QD_FB ops, by the product's own table code (as curve_ops.hpp: co_fixed_table does for W = 4): the
// base of window j by the independent definition, the window's entries in one chain; one lane per window
__global__ void __launch_bounds__(64) qd_fb_kernel(u32* __restrict__ table) {
  const int j = threadIdx.x;
  if (j >= QD_FB_NWIN) return;
  u32* bases = table + (size_t)QD_FB_SLOTS * NIELS_WORDS;
  store_niels(bases + j * NIELS_WORDS, fixed_table_entry(1u, j, QD_FB_W, c_K));
  fixed_table_chain(table, load_niels(bases + j * NIELS_WORDS), (size_t)j * QD_FB_STRIDE, 0u, (u32)QD_FB_STRIDE, QD_FB_W, c_K);
}

#define QD_EXPORT extern "C" __attribute__((visibility("default")))
// a: n records of qd_words(op, 0) words, b: n of qd_words(op, 1) (may be null when 0), out: n of qd_words(op, 2); fb: the table
// qd_fb_build made (the QD_FB ops; may be null for the others).  One wave per workgroup: n > 16 runs more than one.
QD_EXPORT int qd_run(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, const uint32_t* fb, size_t n, void* stream) {
  if (op < 0 || op >= QD_NOPS || (quad_words(op, 1) && !b) || (op >= QD_FB_LOAD && !fb) || !a || !out) return -1;
  if (!n) return 0;
  if (n > ((size_t)1 << 24)) return -1;
  hipLaunchKernelGGL(qd_kernel, grid_for(n, BJJ_QUAD_ITEMS), dim3(BJJ_QUAD_BLOCK), 0, (hipStream_t)stream, op, a, b ? b : a, out, fb, n);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
// table: qd_fb_words() words of device memory, 16-byte aligned
QD_EXPORT int qd_fb_build(uint32_t* table, void* stream) {
  if (!table || ((uintptr_t)table & 15)) return -1;
  hipLaunchKernelGGL(qd_fb_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, table);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
QD_EXPORT int qd_words(int op, int which) { return (op < 0 || op >= QD_NOPS || which < 0 || which > 2) ? -1 : quad_words(op, which); }
QD_EXPORT int qd_fb_words(void) { return QD_FB_WORDS; }
QD_EXPORT int qd_fb_window_bits(void) { return QD_FB_W; }
