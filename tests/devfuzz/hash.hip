// TEST-ONLY library (not part of libbjj_hip.so): the Poseidon permutation that ships, as field elements.
//   * ho_kernel: the dispatcher of hash_ops.hpp -- poseidon5_t in both forms of its partial rounds, one poseidon_full_round,
//     dleq_challenge in both forms -- on raw limbs chosen by the test, one item per lane, grid-strided.
//   * p5c_kernel: p5c_hash5, the six-lane form of csrc/k_small.hip fed Montgomery values directly as the short-call verify and
//     signer kernels feed it, in the launch shape of bjj_k_poseidon5_coop: 64-lane workgroups, groups of eight lanes, one item per
//     group, the groups beyond the batch repeating the last item and storing nothing.  Every lane of a group stores the limbs it
//     holds: the function promises the hash on all eight.
// The short-call unit is included as it ships and everything is built with the product's flags, so the asm dot products are the
// shipped ones.  tests/test_gpu_hash_ops.py checks the results against the plain integers of tests/hash_ref.py and, bit for
// bit, against the same dispatcher built by g++ (tests/emul/emul_hash_ops.cpp).
#include "../../babyjubjub-rs_amd/csrc/k_small.hip"
#include "../../babyjubjub-rs_amd/csrc/dleq.hpp"
#include "hash_ops.hpp"

__global__ void __launch_bounds__(256) ho_kernel(int op, const u32* __restrict__ in, u32* __restrict__ out, size_t n) {
  const size_t nthreads = (size_t)gridDim.x * blockDim.x;
  const size_t wi = hash_words(op, 0), wo = hash_words(op, 1);
#pragma unroll 1
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nthreads) hash_op(op, in + i * wi, out + i * wo, c_K);
}

// in: n records of 5 x 9 raw limbs; out: n records of 8 x 9 raw limbs, lane gl of the item's group at words 9 gl .. 9 gl + 8
__global__ void __launch_bounds__(BJJ_P5C_BLOCK) p5c_kernel(const u32* __restrict__ in, u32* __restrict__ out, size_t n) {
  const int lane = threadIdx.x, gl = lane & (BJJ_P5C_GROUP - 1);
  const size_t item = (size_t)blockIdx.x * (BJJ_P5C_BLOCK / BJJ_P5C_GROUP) + (size_t)(lane >> 3);
  const bool live = item < n;
  const size_t i = live ? item : n - 1;
  const u32* rec = in + i * 5 * NL;
  const Fr h = p5c_hash5(gl, ho_raw(rec), ho_raw(rec + NL), ho_raw(rec + 2 * NL), ho_raw(rec + 3 * NL), ho_raw(rec + 4 * NL));
  if (live) ho_put_raw(out + (i * BJJ_P5C_GROUP + (size_t)gl) * NL, h);
}

#define HO_EXPORT extern "C" __attribute__((visibility("default")))
// in: n records of ho_words(op, 0) words, out: n records of ho_words(op, 1)
HO_EXPORT int ho_run(int op, const uint32_t* in, uint32_t* out, size_t n, void* stream) {
  if (op < 0 || op >= HO_NOPS || !in || !out) return -1;
  if (!n) return 0;
  const size_t want = (n + 255) / 256;
  const int grid = (int)(want < 2048 ? want : 2048);
  hipLaunchKernelGGL(ho_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, op, in, out, n);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
HO_EXPORT int ho_words(int op, int which) { return (op < 0 || op >= HO_NOPS || which < 0 || which > 1) ? -1 : hash_words(op, which); }
// in: n records of 45 words, out: n records of 72 words.  One wave per workgroup: n > 8 runs more than one.
HO_EXPORT int p5c_run(const uint32_t* in, uint32_t* out, size_t n, void* stream) {
  if (!in || !out) return -1;
  if (!n) return 0;
  if (n > ((size_t)1 << 24)) return -1;
  hipLaunchKernelGGL(p5c_kernel, grid_for(n, BJJ_P5C_BLOCK / BJJ_P5C_GROUP), dim3(BJJ_P5C_BLOCK), 0, (hipStream_t)stream, in, out, n);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
