// libbjj_hip.so, kernel unit 10: verification against one signer's fixed-base table (include/bjj_hip_signer.h; bodies: signer.hpp).
//   bjj_k_verify_signer<SCHNORR>: ok[i] = verify(pk, (R_i, s_i), msg_i) (src/lib.rs:395-412), resp. verify_schnorr (:375-385), for
//   the ONE pk whose table bjj_base_create built: one Poseidon permutation, two table-gather chains (8 hm * pk over the signer's
//   table, s * B8 over the context's), the reference's last addition with t left projective and a cross-multiplied comparison.
//   No inversion, no per-lane table, no work list: one item per lane, grid-strided, nothing but the staging rows in LDS.
#include "k_common.hpp"
#include "signer.hpp"

// 256-lane workgroups, two per CU: 4 waves x 2 staging areas x 8 KB = 64 KB of LDS each, 2 waves per SIMD (256 VGPRs) -- the
// register and LDS budget of bjj_k_mul_bases (k_bases.hip) in halves, because these waves never meet at a barrier: a workgroup
// that runs out of items frees its half of the CU at once.
#define BJJ_SIGNER_BLOCK 256

// Every lane of a wave takes part in every gather (GatherCoopLds), so the trip count is wave-uniform and lanes past n work on
// item n - 1 without storing, as in bjj_k_mul_bases.
template <bool SCHNORR>
__device__ __forceinline__ void verify_signer_body(const SignerArgs& A, const uint8_t* __restrict__ r, const uint8_t* __restrict__ s,
                                                   const uint8_t* __restrict__ msg, size_t n, uint8_t* __restrict__ ok) {
  __shared__ __attribute__((aligned(16))) u32 stage[(BJJ_SIGNER_BLOCK / 64) * 2 * FB_STAGE_WORDS];
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nthreads = (size_t)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  const GatherCoopLds<2> fb = {A.T.table, stage + (threadIdx.x >> 6) * 2 * FB_STAGE_WORDS, lane};
#pragma unroll 1
  for (size_t i = tid; i - lane < n; i += nthreads) {
    const bool valid = i < n;
    const size_t item = valid ? i : n - 1;
    const int v = verify_signer_item<SCHNORR>(A, fb, r + item * 64, s + item * 32, msg + item * 32, c_K);
    if (valid) ok[i] = (uint8_t)v;
  }
}
__global__ void __launch_bounds__(BJJ_SIGNER_BLOCK, 2) bjj_k_eddsa_verify_signer(const SignerArgs A, const uint8_t* __restrict__ r,
                                                                                const uint8_t* __restrict__ s, const uint8_t* __restrict__ msg,
                                                                                size_t n, uint8_t* __restrict__ ok) {
  verify_signer_body<false>(A, r, s, msg, n, ok);
}
__global__ void __launch_bounds__(BJJ_SIGNER_BLOCK, 2) bjj_k_schnorr_verify_signer(const SignerArgs A, const uint8_t* __restrict__ r,
                                                                                  const uint8_t* __restrict__ s, const uint8_t* __restrict__ msg,
                                                                                  size_t n, uint8_t* __restrict__ ok) {
  verify_signer_body<true>(A, r, s, msg, n, ok);
}

// ---- launchers (declared in bjj_launch.hpp) ------------------------------------------------------------
namespace bjjk {
int signer_lanes_per_cu() { return lanes_for_both(bjj_k_eddsa_verify_signer, bjj_k_schnorr_verify_signer, BJJ_SIGNER_BLOCK); }
hipError_t verify_signer(hipStream_t st, int cus, int lanes_per_cu, bool schnorr, const SignerArgs& A, const uint8_t* r, const uint8_t* s,
                         const uint8_t* msg, size_t n, uint8_t* ok) {
  const int grid = capped_grid(n, BJJ_SIGNER_BLOCK, (size_t)cus * (size_t)(lanes_per_cu / BJJ_SIGNER_BLOCK));
  if (schnorr) BJJ_LAUNCH(bjj_k_schnorr_verify_signer, dim3(grid), dim3(BJJ_SIGNER_BLOCK), 0, st, A, r, s, msg, n, ok);
  else BJJ_LAUNCH(bjj_k_eddsa_verify_signer, dim3(grid), dim3(BJJ_SIGNER_BLOCK), 0, st, A, r, s, msg, n, ok);
  return hipGetLastError();
}
}  // namespace bjjk
