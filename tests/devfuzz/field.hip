// TEST-ONLY kernel (not part of libbjj_hip.so): the field layer that ships -- fr_add / fr_sub and their lazy forms,
// fr_reduce_weak, fr_canon / fr_is_zero / fr_eq, the word and Montgomery conversions, fr_sqrt, ref_on_curve, the comparisons
// with r and (r-1)/2, decompress_item and compress_item -- on raw limbs or words chosen by the test, one item per lane,
// grid-strided (field_ops.hpp).  Built with the product's flags.  tests/test_gpu_field_ops.py checks it against the plain
// integers of tests/field_ref.py and, bit for bit, against the same body built by g++ (tests/emul/emul_field_ops.cpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../babyjubjub-rs_amd/csrc/bjj_device.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
#include "field_ops.hpp"

using namespace bjj;

static __constant__ Consts c_K = BJJ_CONSTS_INIT;

__global__ void __launch_bounds__(256) fo_kernel(int op, const u32* __restrict__ a, const u32* __restrict__ b, u32* __restrict__ out,
                                                 size_t n) {
  const size_t nthreads = (size_t)gridDim.x * blockDim.x;
  const size_t wa = field_words(op, 0), wb = field_words(op, 1), wo = field_words(op, 2);
#pragma unroll 1
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nthreads)
    field_op(op, a + i * wa, b + i * wb, out + i * wo, c_K);
}

// a: n records of field_words(op, 0) words, b: n records of field_words(op, 1) (may be null when 0), out: n records of
// field_words(op, 2)
extern "C" __attribute__((visibility("default"))) int fo_run(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n,
                                                              void* stream) {
  if (op < 0 || op >= FO_NOPS || (field_words(op, 1) && !b) || !a || !out) return -1;
  if (!n) return 0;
  const size_t want = (n + 255) / 256;
  const int grid = (int)(want < 2048 ? want : 2048);
  hipLaunchKernelGGL(fo_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, op, a, b, out, n);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
extern "C" __attribute__((visibility("default"))) int fo_words(int op, int which) {   // 0: a, 1: b, 2: out
  return (op < 0 || op >= FO_NOPS || which < 0 || which > 2) ? -1 : field_words(op, which);
}
