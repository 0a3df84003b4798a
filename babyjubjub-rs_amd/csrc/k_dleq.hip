// libbjj_hip.so, kernel unit 16: two points with two scalars, and Chaum-Pedersen proofs of discrete-log equality
// (include/bjj_hip_dleq.h; bodies: dleq.hpp).
//   bjj_k_mul_pair / bjj_k_mul_pair_add   out[i] = A[i] + a[i] P[i] + b[i] Q[i]: the fold of two Point::mul_scalar (src/lib.rs:149-164)
//                                         with PointProjective::add (src/lib.rs:88-131), then .affine() (src/lib.rs:70-85), ONE inversion pass
//   bjj_k_dleq_verify                     ok[i] = the verdict on the proof (A, B, z) that log_G PK = log_C1 D; no inversion, no point output
//   bjj_k_dleq_nonce, bjj_k_dleq_respond  the two ends of the prover's launch chain: w' = w mod l, and the hash with z = w' + c sk'
// per-lane table entries of this unit: raw (bjj_device.hpp "per-lane variable-base table") -- two tables per lane and 128 entry loads
// per item, the case the verify kernel measured 3.7-5 % faster raw than packed.
#define BJJ_PNIELS_LAYOUT 0
#include "k_common.hpp"
#include "dleq.hpp"

// 256-lane workgroups, two per CU: 2 waves per SIMD (256 VGPRs), the budget the verify kernel -- the other user of the joint loop --
// and K1 were measured best at (k_var.hip, "Workgroup size").  Grid-strided over one resident set of workgroups: a lane's two tables
// are vb_tables + global lane * DLEQ_LANE_WORDS, which the host sizes for exactly that set (dleq_tables, bjj_dleq.inc).
#define BJJ_DLEQ_BLOCK 256
#define BJJ_DLEQ_MIN_BLOCKS 2
#define DLEQ_LANE_WORDS (2 * VB_TABLE_WORDS)
static_assert(DLEQ_LANE_WORDS == BJJ_DLEQ_LANE_WORDS, "bjj_launch.hpp: the host sizes two raw tables per lane");

// Phase 1 stashes the items of a lane (tid, tid + nthreads, ..), an item that is refused stays out of the running product (Z = 0 marks
// its record, EPI_SKIPPABLE) and has its output zeroed here; phase 2 is the shared epilogue.  Nothing is wave-cooperative: a lane
// past n takes no item but reaches the barriers of the inversion.
template <bool ADD>
__device__ __forceinline__ void mul_pair_body(PairArgs A, size_t n, uint8_t* __restrict__ out, uint8_t* __restrict__ ok,
                                              u32* __restrict__ scratch, u32* __restrict__ vb_tables) {
  __shared__ u32 lds[NL * 64];
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nthreads = (size_t)gridDim.x * blockDim.x;
  u32* const tbl = vb_tables + tid * DLEQ_LANE_WORDS;
  if (!ADD) A.add = nullptr;
  Fr run = fr_one();
#pragma unroll 1
  for (size_t i = tid; i < n; i += nthreads) {
    Ext p;
    if (pair_item(A, i, tbl, p, c_K)) {
      epilogue_stash(p, run, out + i * 64, scratch + i * 16);
      ok[i] = 1;   // BJJ_DLEQ_OK
    } else {
      const u32 z[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
      epilogue_stash_skipped(scratch + i * 16);
      store_w8(out + i * 64, z); store_w8(out + i * 64 + 32, z);
      ok[i] = 2;   // BJJ_DLEQ_OFF_CURVE
    }
  }
  epilogue_run<BJJ_DLEQ_BLOCK, EPI_SKIPPABLE>(run, n, tid, nthreads, out, scratch, lds);
}
// Two kernels with names of their own, not two instantiations of one template: a name has one machine code (srchash.py keys by name).
__global__ void __launch_bounds__(BJJ_DLEQ_BLOCK, BJJ_DLEQ_MIN_BLOCKS) bjj_k_mul_pair(const PairArgs A, size_t n, uint8_t* __restrict__ out,
                                                                                     uint8_t* __restrict__ ok, u32* __restrict__ scratch,
                                                                                     u32* __restrict__ vb_tables) {
  mul_pair_body<false>(A, n, out, ok, scratch, vb_tables);
}
__global__ void __launch_bounds__(BJJ_DLEQ_BLOCK, BJJ_DLEQ_MIN_BLOCKS) bjj_k_mul_pair_add(const PairArgs A, size_t n, uint8_t* __restrict__ out,
                                                                                         uint8_t* __restrict__ ok, u32* __restrict__ scratch,
                                                                                         u32* __restrict__ vb_tables) {
  mul_pair_body<true>(A, n, out, ok, scratch, vb_tables);
}

// bjj_k_eddsa_verify_signer's shape (k_signer.hip): 4 waves x 2 staging areas x 8 KB = 64 KB of LDS per workgroup.  Every lane of a wave
// takes part in every gather (GatherCoopLds), so the trip count is wave-uniform and lanes past n work on item n - 1 without storing.
__global__ void __launch_bounds__(BJJ_DLEQ_BLOCK, BJJ_DLEQ_MIN_BLOCKS) bjj_k_dleq_verify(const DleqVerifyArgs A, size_t n, uint8_t* __restrict__ ok,
                                                                                        u32* __restrict__ vb_tables) {
  __shared__ __attribute__((aligned(16))) u32 stage[(BJJ_DLEQ_BLOCK / 64) * 2 * FB_STAGE_WORDS];
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nthreads = (size_t)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  const GatherCoopLds<2> fb = {A.b[0].table, stage + (threadIdx.x >> 6) * 2 * FB_STAGE_WORDS, lane};
  u32* const tbl = vb_tables + tid * DLEQ_LANE_WORDS;
#pragma unroll 1
  for (size_t i = tid; i - lane < n; i += nthreads) {
    const bool valid = i < n;
    const size_t item = valid ? i : n - 1;
    const int v = dleq_verify_item(A, fb, item, tbl, c_K);
    if (valid) ok[i] = (uint8_t)v;
  }
}

// The prover's two small kernels: one item per lane, grid-strided, no scratch
__global__ void __launch_bounds__(BJJ_BLOCK) bjj_k_dleq_nonce(const uint8_t* __restrict__ w, size_t n, uint8_t* __restrict__ z) {
  const size_t nthreads = (size_t)gridDim.x * blockDim.x;
#pragma unroll 1
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nthreads) dleq_nonce_item(w, i, z, c_K);
}
// ok[i] as the first launch of the chain (bjj_k_mul_common) left it: 1, or 2 for a C1 off the curve
__global__ void __launch_bounds__(BJJ_BLOCK) bjj_k_dleq_respond(const DleqRespondArgs A, size_t n, const uint8_t* __restrict__ ok) {
  const size_t nthreads = (size_t)gridDim.x * blockDim.x;
#pragma unroll 1
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nthreads) dleq_respond_item(A, i, ok[i] == 1, c_K);
}

// ---- launchers (declared in bjj_launch.hpp) ------------------------------------------------------------
namespace bjjk {
// resident lanes per CU that serve the three kernels with per-lane tables: one table area and one grid cap for all of them
int dleq_lanes_per_cu() {
  const int a = lanes_for_both(bjj_k_mul_pair, bjj_k_mul_pair_add, BJJ_DLEQ_BLOCK), b = occupancy_of(bjj_k_dleq_verify, BJJ_DLEQ_BLOCK) * BJJ_DLEQ_BLOCK;
  return a < b ? a : b;
}
int dleq_block() { return BJJ_DLEQ_BLOCK; }
int occ_dleq_respond() { return occupancy_of(bjj_k_dleq_respond, BJJ_BLOCK); }
hipError_t mul_pair(hipStream_t st, int cus, int lanes_per_cu, const PairArgs& A, size_t n, uint8_t* out, uint8_t* ok, u32* scratch, u32* vb_tables) {
  const int grid = capped_grid(n, BJJ_DLEQ_BLOCK, (size_t)cus * (size_t)(lanes_per_cu / BJJ_DLEQ_BLOCK));
  if (A.add) BJJ_LAUNCH(bjj_k_mul_pair_add, dim3(grid), dim3(BJJ_DLEQ_BLOCK), 0, st, A, n, out, ok, scratch, vb_tables);
  else BJJ_LAUNCH(bjj_k_mul_pair, dim3(grid), dim3(BJJ_DLEQ_BLOCK), 0, st, A, n, out, ok, scratch, vb_tables);
  return hipGetLastError();
}
hipError_t dleq_verify(hipStream_t st, int cus, int lanes_per_cu, const DleqVerifyArgs& A, size_t n, uint8_t* ok, u32* vb_tables) {
  const int grid = capped_grid(n, BJJ_DLEQ_BLOCK, (size_t)cus * (size_t)(lanes_per_cu / BJJ_DLEQ_BLOCK));
  BJJ_LAUNCH(bjj_k_dleq_verify, dim3(grid), dim3(BJJ_DLEQ_BLOCK), 0, st, A, n, ok, vb_tables);
  return hipGetLastError();
}
hipError_t dleq_nonce(hipStream_t st, int grid, const uint8_t* w, size_t n, uint8_t* z) {
  BJJ_LAUNCH(bjj_k_dleq_nonce, dim3(grid), dim3(BJJ_BLOCK), 0, st, w, n, z);
  return hipGetLastError();
}
hipError_t dleq_respond(hipStream_t st, int grid, const DleqRespondArgs& A, size_t n, const uint8_t* ok) {
  BJJ_LAUNCH(bjj_k_dleq_respond, dim3(grid), dim3(BJJ_BLOCK), 0, st, A, n, ok);
  return hipGetLastError();
}
}  // namespace bjjk
