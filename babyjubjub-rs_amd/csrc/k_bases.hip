// libbjj_hip.so, kernel unit 9: fixed-base tables for caller-chosen points (include/bjj_hip_bases.h; bodies: bases.hpp).
//   bjj_k_base_window_bases / bjj_k_check_base_table: k_fixed.hip's table kernels with the base point as an argument (the
//   entries between them are filled by k_fixed.hip's bjj_k_build_fixed_table, which never looks at the base point)
//   bjj_k_mul_bases: out[i] = sum_j scalars[j][i] * P_j over up to BJJ_MAX_BASES tables, one item per lane -- the fold of
//   Point::mul_scalar (src/lib.rs:149-164) with PointProjective::add (src/lib.rs:88-131), then .affine() (src/lib.rs:70-85)
#include "k_common.hpp"
#include "bases.hpp"

// One shape: one 512-lane workgroup per CU, two staging areas per wave -- K1's (k_fixed.hip), with its LDS budget (149 760 B of
// the CU's 160 KB as compiled, the same as K1: 8 waves x 2 x 8 KB of staging, the rest the workgroup inversion's exchange areas)
// and its register budget (2 waves per SIMD).
#define BJJ_BASES_BLOCK BJJ_EPI_BLOCK

// a base point as it travels in the kernel arguments: x, y of the caller's record (reduced mod r by the Montgomery conversion)
struct BasePointArg { u32 x[8], y[8]; };

__global__ void __launch_bounds__(64) bjj_k_base_window_bases(u32* bases, int W, int nwin, BasePointArg P) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nwin) return;
  store_niels(bases + (size_t)j * NIELS_WORDS, base_table_entry(fr_to_mont_words(P.x), fr_to_mont_words(P.y), 1u, j, W, c_K));
}
__global__ void __launch_bounds__(BJJ_BLOCK) bjj_k_check_base_table(const u32* __restrict__ table, const u32* __restrict__ bases, int W,
                                                                int nwin, BasePointArg P, unsigned long long* bad) {
  const size_t stride = fixed_stride(W);
  const size_t total = stride * (size_t)nwin, nthreads = (size_t)gridDim.x * blockDim.x;
  const Fr bx = fr_to_mont_words(P.x), by = fr_to_mont_words(P.y);
  unsigned long long mine = 0;
#pragma unroll 1
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += nthreads)
    mine += (unsigned long long)base_table_check_slot(table, bases, (int)(e / stride), (u32)(e % stride), W, nwin, bx, by, c_K);
  if (mine) atomicAdd(bad, mine);
}

// Every lane of a wave takes part in every gather (GatherCoopLds), so the trip count is wave-uniform and lanes past n work on
// item n - 1 without storing, as in mul_fixed_base_body; the loop over the bases runs on the kernel arguments alone.
__global__ void __launch_bounds__(BJJ_BASES_BLOCK, 1) bjj_k_mul_bases(const BasesArgs A, size_t n, uint8_t* __restrict__ out,
                                                                     u32* __restrict__ scratch) {
  __shared__ u32 lds[NL * 64];
  __shared__ __attribute__((aligned(16))) u32 stage[(BJJ_BASES_BLOCK / 64) * 2 * FB_STAGE_WORDS];
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nthreads = (size_t)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  const GatherCoopLds<2> fb = {A.b[0].table, stage + (threadIdx.x >> 6) * 2 * FB_STAGE_WORDS, lane};
  Fr run = fr_one();
#pragma unroll 1
  for (size_t i = tid; i - lane < n; i += nthreads) {
    const bool valid = i < n;
    const size_t item = valid ? i : n - 1;
    Ext p = mul_bases_item(A, fb, [&](int j, u32 raw[8]) { load_w8(A.b[j].scalars + item * 32, raw); }, c_K);
    if (valid) epilogue_stash(p, run, out + i * 64, scratch + i * 16);
  }
  epilogue_run<BJJ_BASES_BLOCK, EPI_AFFINE, INV_K1>(run, n, tid, nthreads, out, scratch, lds);
}

// ---- launchers (declared in bjj_launch.hpp) ------------------------------------------------------------
namespace bjjk {
static BasePointArg point_arg(const uint32_t xy[16]) {
  BasePointArg P;
  for (int i = 0; i < 8; i++) { P.x[i] = xy[i]; P.y[i] = xy[8 + i]; }
  return P;
}
int bases_lanes_per_cu() { return occupancy_of(bjj_k_mul_bases, BJJ_BASES_BLOCK) * BJJ_BASES_BLOCK; }
hipError_t base_window_bases(hipStream_t st, u32* bases, int W, int nwin, const uint32_t xy[16]) {
  BJJ_LAUNCH(bjj_k_base_window_bases, dim3((nwin + 63) / 64), dim3(64), 0, st, bases, W, nwin, point_arg(xy));
  return hipGetLastError();
}
hipError_t check_base_table(hipStream_t st, int grid, const u32* table, const u32* bases, int W, int nwin, const uint32_t xy[16],
                            unsigned long long* d_bad) {
  BJJ_LAUNCH(bjj_k_check_base_table, dim3((unsigned)grid), dim3(BJJ_BLOCK), 0, st, table, bases, W, nwin, point_arg(xy), d_bad);
  return hipGetLastError();
}
hipError_t mul_bases(hipStream_t st, int cus, int lanes_per_cu, const BasesArgs& A, size_t n, uint8_t* out, u32* scratch) {
  const int grid = capped_grid(n, BJJ_BASES_BLOCK, (size_t)cus * (size_t)(lanes_per_cu / BJJ_BASES_BLOCK));
  BJJ_LAUNCH(bjj_k_mul_bases, dim3(grid), dim3(BJJ_BASES_BLOCK), 0, st, A, n, out, scratch);
  return hipGetLastError();
}
}  // namespace bjjk
