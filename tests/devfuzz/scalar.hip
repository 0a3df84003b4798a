// TEST-ONLY kernel (not part of libbjj_hip.so): the scalar arithmetic that ships -- scalar_mod_l, scalar_mod_order, plain_mod_l,
// fl_mul / fl_canon4, the digest and nonce reductions of the signers, wide_scalar_mod_order, verify's c = v*s mod l,
// lattice_short_pair and euclid_partial_step -- on raw words chosen by the test, one item per lane, grid-strided
// (scalar_ops.hpp).  Built with the product's flags (-fno-fast-math), so the f64 quotient of euclid_partial_step is the
// division the verify kernels execute.  tests/test_gpu_scalar_fuzz.py checks it against Python integers and, bit for bit,
// against the same body built by g++ (tests/emul).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../babyjubjub-rs_amd/csrc/sign.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
#include "scalar_ops.hpp"

using namespace bjj;

static __constant__ Consts c_K = BJJ_CONSTS_INIT;

__global__ void __launch_bounds__(256) sc_kernel(int op, const u32* __restrict__ a, const u32* __restrict__ b, u32* __restrict__ out,
                                                 size_t n, int nw) {
  const size_t nthreads = (size_t)gridDim.x * blockDim.x;
  const size_t wa = sc_a_words(op, nw), wb = sc_b_words(op), wo = sc_out_words(op);
#pragma unroll 1
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nthreads)
    sc_item(op, a + i * wa, b + i * wb, out + i * wo, nw, c_K);
}

// a: n records of sc_a_words(op, nw) words, b: n records of sc_b_words(op) (may be null when 0), out: n records of sc_out_words(op)
extern "C" __attribute__((visibility("default"))) int sc_run(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n,
                                                              int nw, void* stream) {
  if (op < 0 || op >= SC_NOPS || (op == SC_WIDE && (nw < 1 || nw > 1024)) || (sc_b_words(op) && !b) || !a || !out) return -1;
  if (!n) return 0;
  const size_t want = (n + 255) / 256;
  const int grid = (int)(want < 2048 ? want : 2048);
  hipLaunchKernelGGL(sc_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, op, a, b, out, n, nw);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
extern "C" __attribute__((visibility("default"))) int sc_words(int op, int nw, int which) {   // 0: a, 1: b, 2: out
  return which == 0 ? sc_a_words(op, nw) : which == 1 ? sc_b_words(op) : sc_out_words(op);
}
