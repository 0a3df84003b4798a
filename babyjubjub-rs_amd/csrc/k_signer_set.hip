// libbjj_hip.so, kernel unit 11: verification against a set of signers' tables, by per-item index (include/bjj_hip_signer_set.h;
// bodies: signer_set.hpp).
//   bjj_k_set_window_bases / bjj_k_set_fill / bjj_k_set_check: the tables of ALL k signers of a set in three launches -- window
//   bases, entries, induction check -- each thread finding its signer from its index (signer j at entry offset j * E)
//   bjj_k_verify_set<SCHNORR>: bjj_k_verify_signer (k_signer.hip) with the key and the table chosen per item: ok[i] =
//   verify(pks[idx_i], (R_i, s_i), msg_i), or 3 when idx_i is not an index of the set
#include "k_common.hpp"
#include "signer_set.hpp"

// the shape of k_signer.hip: 256-lane workgroups, two per CU, 4 waves x 2 staging areas x 8 KB of LDS each
#define BJJ_SET_BLOCK 256

__global__ void __launch_bounds__(64) bjj_k_set_window_bases(u32* bases, const u32* __restrict__ keys, int W, int nwin, size_t k) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= k * (size_t)nwin) return;
  set_window_base(bases, keys, t, W, nwin, c_K);
}
__global__ void __launch_bounds__(BJJ_BLOCK) bjj_k_set_fill(u32* table, const u32* __restrict__ bases, int W, int nwin, u32 chain, size_t k) {
  const size_t cpw = (fixed_stride(W) + chain - 1) / chain;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= k * (size_t)nwin * cpw) return;
  set_fill_chain(table, bases, t, W, nwin, chain, c_K);
}
__global__ void __launch_bounds__(BJJ_BLOCK) bjj_k_set_check(const u32* __restrict__ table, const u32* __restrict__ bases,
                                                         const u32* __restrict__ keys, int W, int nwin, size_t k, unsigned long long* bad) {
  const size_t total = k * (size_t)set_entries_per_signer(W), nthreads = (size_t)gridDim.x * blockDim.x;
  unsigned long long mine = 0;
#pragma unroll 1
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += nthreads)
    mine += (unsigned long long)set_check_entry(table, bases, keys, e, W, nwin, c_K);
  if (mine) atomicAdd(bad, mine);
}

// Every lane of a wave takes part in every gather (GatherCoopLds), so the trip count is wave-uniform and lanes past n work on
// item n - 1 without storing, as in bjj_k_verify_signer.  The table base is wave-uniform (kernel arguments); the signer is per lane.
template <bool SCHNORR>
__device__ __forceinline__ void verify_set_body(const SetArgs& A, const u32* __restrict__ idx, const uint8_t* __restrict__ r,
                                                const uint8_t* __restrict__ s, const uint8_t* __restrict__ msg, size_t n,
                                                uint8_t* __restrict__ ok) {
  __shared__ __attribute__((aligned(16))) u32 stage[(BJJ_SET_BLOCK / 64) * 2 * FB_STAGE_WORDS];
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nthreads = (size_t)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  const GatherCoopLds<2> fb = {A.T.table, stage + (threadIdx.x >> 6) * 2 * FB_STAGE_WORDS, lane};
#pragma unroll 1
  for (size_t i = tid; i - lane < n; i += nthreads) {
    const bool valid = i < n;
    const size_t item = valid ? i : n - 1;
    const int v = verify_set_item<SCHNORR>(A, fb, idx[item], r + item * 64, s + item * 32, msg + item * 32, c_K);
    if (valid) ok[i] = (uint8_t)v;
  }
}
__global__ void __launch_bounds__(BJJ_SET_BLOCK, 2) bjj_k_eddsa_verify_set(const SetArgs A, const u32* __restrict__ idx,
                                                                          const uint8_t* __restrict__ r, const uint8_t* __restrict__ s,
                                                                          const uint8_t* __restrict__ msg, size_t n, uint8_t* __restrict__ ok) {
  verify_set_body<false>(A, idx, r, s, msg, n, ok);
}
__global__ void __launch_bounds__(BJJ_SET_BLOCK, 2) bjj_k_schnorr_verify_set(const SetArgs A, const u32* __restrict__ idx,
                                                                            const uint8_t* __restrict__ r, const uint8_t* __restrict__ s,
                                                                            const uint8_t* __restrict__ msg, size_t n, uint8_t* __restrict__ ok) {
  verify_set_body<true>(A, idx, r, s, msg, n, ok);
}

// ---- launchers (declared in bjj_launch.hpp) ------------------------------------------------------------
namespace bjjk {
int set_lanes_per_cu() { return lanes_for_both(bjj_k_eddsa_verify_set, bjj_k_schnorr_verify_set, BJJ_SET_BLOCK); }
// the chain length of fill_fixed_table (k_fixed.hip), from the entries of the whole set
static size_t set_chain(size_t k, int W, int nwin) {
  const size_t chain = (k * fixed_stride(W) * (size_t)nwin) >> 18;
  return chain < 4 ? 4 : (chain > 256 ? 256 : chain);
}
hipError_t build_signer_set(hipStream_t st, u32* table, u32* bases, const u32* keys, size_t k, int W, int nwin) {
  const size_t nb = k * (size_t)nwin;
  BJJ_LAUNCH(bjj_k_set_window_bases, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, st, bases, keys, W, nwin, k);
  const size_t chain = set_chain(k, W, nwin);
  const size_t chains = ((fixed_stride(W) + chain - 1) / chain) * nb;
  BJJ_LAUNCH(bjj_k_set_fill, dim3((unsigned)((chains + BJJ_BLOCK - 1) / BJJ_BLOCK)), dim3(BJJ_BLOCK), 0, st, table, bases, W, nwin, (u32)chain, k);
  return hipGetLastError();
}
hipError_t check_signer_set(hipStream_t st, int grid, const u32* table, const u32* bases, const u32* keys, size_t k, int W, int nwin,
                            unsigned long long* d_bad) {
  BJJ_LAUNCH(bjj_k_set_check, dim3((unsigned)grid), dim3(BJJ_BLOCK), 0, st, table, bases, keys, W, nwin, k, d_bad);
  return hipGetLastError();
}
hipError_t verify_set(hipStream_t st, int cus, int lanes_per_cu, bool schnorr, const SetArgs& A, const uint32_t* idx, const uint8_t* r,
                      const uint8_t* s, const uint8_t* msg, size_t n, uint8_t* ok) {
  const int grid = capped_grid(n, BJJ_SET_BLOCK, (size_t)cus * (size_t)(lanes_per_cu / BJJ_SET_BLOCK));
  if (schnorr) BJJ_LAUNCH(bjj_k_schnorr_verify_set, dim3(grid), dim3(BJJ_SET_BLOCK), 0, st, A, idx, r, s, msg, n, ok);
  else BJJ_LAUNCH(bjj_k_eddsa_verify_set, dim3(grid), dim3(BJJ_SET_BLOCK), 0, st, A, idx, r, s, msg, n, ok);
  return hipGetLastError();
}
}  // namespace bjjk
