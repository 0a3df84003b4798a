// TEST-ONLY kernel (not part of libbjj_hip.so): the group law that ships -- ext_madd / ext_add_pn / ext_dbl on entries passed
// through niels_cneg_lazy / pniels_cneg, the Niels / PNiels / Ext conversions, ref_add, ref_mul_scalar, var_base_item -- and
// the per-lane table, ladder and fixed-table code (vb_build_table, vb_table_load, vb_mul_windowed, fixed_table_entry,
// fixed_table_chain, fixed_table_check_slot) on raw limbs chosen by the test, one item per lane, grid-strided (curve_ops.hpp).
// Built with the product's flags, once per per-lane table layout that ships (BJJ_PNIELS_LAYOUT 0 and 1).
// tests/test_gpu_curve_ops.py checks it against the plain integers of tests/curve_ref.py and, bit for bit, against the same
// body built by g++ (tests/emul/emul_curve_ops.cpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../babyjubjub-rs_amd/csrc/bjj_device.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
#include "curve_ops.hpp"

using namespace bjj;

static __constant__ Consts c_K = BJJ_CONSTS_INIT;

__global__ void __launch_bounds__(64) co_kernel(int op, const u32* __restrict__ a, const u32* __restrict__ b, u32* __restrict__ out,
                                                u32* __restrict__ scratch, size_t n) {
  const size_t nthreads = (size_t)gridDim.x * blockDim.x;
  const size_t wa = curve_words(op, 0), wb = curve_words(op, 1), wo = curve_words(op, 2), ws = curve_words(op, 3);
#pragma unroll 1
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nthreads)
    curve_op(op, a + i * wa, b + i * wb, out + i * wo, scratch + i * ws, c_K);
}

// a: n records of curve_words(op, 0) words, b: n of curve_words(op, 1) (may be null when 0), out: n of curve_words(op, 2),
// scratch: n of curve_words(op, 3), 16-byte aligned (may be null when 0).  Workgroups of one wave: n > 64 runs more than one.
extern "C" __attribute__((visibility("default"))) int co_run(int op, const uint32_t* a, const uint32_t* b, uint32_t* out,
                                                              uint32_t* scratch, size_t n, void* stream) {
  if (op < 0 || op >= CO_NOPS || (curve_words(op, 1) && !b) || (curve_words(op, 3) && (!scratch || ((uintptr_t)scratch & 15))) || !a || !out)
    return -1;
  if (!n) return 0;
  const size_t want = (n + 63) / 64;
  const int grid = (int)(want < 4096 ? want : 4096);
  hipLaunchKernelGGL(co_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, op, a, b, out, scratch, n);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
extern "C" __attribute__((visibility("default"))) int co_words(int op, int which) {   // 0: a, 1: b, 2: out, 3: scratch
  return (op < 0 || op >= CO_NOPS || which < 0 || which > 3) ? -1 : curve_words(op, which);
}
extern "C" __attribute__((visibility("default"))) int co_layout() { return BJJ_PNIELS_LAYOUT; }
