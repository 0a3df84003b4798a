// libbjj_hip.so, kernel unit 15: exponential-ElGamal encryption and re-randomisation in one launch (include/bjj_hip_elgamal.h;
// body: elgamal.hpp).
//   bjj_k_elgamal_encrypt / bjj_k_elgamal_encrypt_add (the form with add arrays): c1[i] = A1[i] + r[i] G, c2[i] = A2[i] + m[i] G +
//   r[i] PK over the fixed-base tables of G and PK, one item per lane -- the fold of Point::mul_scalar (src/lib.rs:149-164) with PointProjective::add (src/lib.rs:88-131), then
//   .affine() (src/lib.rs:70-85), twice per item with ONE inversion pass
#include "k_common.hpp"
#include "elgamal.hpp"

// bjj_k_mul_bases' shape (k_bases.hip): one 512-lane workgroup per CU, two staging areas per wave, 2 waves per SIMD.
#define BJJ_ELGAMAL_BLOCK BJJ_EPI_BLOCK

// Every lane of a wave takes part in every gather (GatherCoopLds), so the trip count is wave-uniform and lanes past n work on
// item n - 1 without storing.  Phase 1 stashes c1 and then c2 of an item: records 2i and 2i + 1 of the scratch set, both Z's in
// the lane's running product.  An item with an off-curve addend stays out of the product (Z = 0 marks its two records,
// EPI_SKIPPABLE) and has its outputs zeroed here.  Phase 2 walks the lane's items backwards, c2 and then c1.
// out_c1 / out_c2 carry no __restrict__: they may be add_c1 / add_c2 (elgamal_item reads an addend before its slot is written).
template <bool ADD>
__device__ __forceinline__ void elgamal_encrypt_body(const ElgamalArgs& A, size_t n, uint8_t* out_c1, uint8_t* out_c2, uint8_t* ok,
                                                     u32* __restrict__ scratch) {
  __shared__ u32 lds[NL * 64];
  __shared__ __attribute__((aligned(16))) u32 stage[(BJJ_ELGAMAL_BLOCK / 64) * 2 * FB_STAGE_WORDS];
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nthreads = (size_t)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  const GatherCoopLds<2> fb = {A.b[0].table, stage + (threadIdx.x >> 6) * 2 * FB_STAGE_WORDS, lane};
  Fr run = fr_one();
#pragma unroll 1
  for (size_t i = tid; i - lane < n; i += nthreads) {
    const bool valid = i < n;
    const size_t item = valid ? i : n - 1;
    const bool on = elgamal_item<ADD>(A, fb, item, [&](int which, const Ext& p, bool on_curve) {
      if (!valid) return;
      uint8_t* const o = (which ? out_c2 : out_c1) + i * 64;
      u32* const rec = scratch + (2 * i + (size_t)which) * 16;
      if (!ADD || on_curve) {
        epilogue_stash(p, run, o, rec);
      } else {
        const u32 z[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        epilogue_stash_skipped(rec);
        store_w8(o, z); store_w8(o + 32, z);
      }
    }, c_K);
    if (valid && ok) ok[i] = on ? 1 : 2;   // BJJ_ELGAMAL_OK / BJJ_ELGAMAL_OFF_CURVE
  }
  Fr inv = fr_mul(block_invert<BJJ_ELGAMAL_BLOCK, INV_K1>(run, lds), fr_one_plain());  // out of Montgomery form once per lane
  if (tid >= n) return;
  const size_t cnt = (n - tid + nthreads - 1) / nthreads;
#pragma unroll 1
  for (size_t k = cnt; k-- > 0;) {
    const size_t i = tid + k * nthreads;
    epilogue_finish<ADD ? EPI_SKIPPABLE : EPI_AFFINE>(inv, out_c2 + i * 64, out_c2 + i * 64, scratch + (2 * i + 1) * 16);
    epilogue_finish<ADD ? EPI_SKIPPABLE : EPI_AFFINE>(inv, out_c1 + i * 64, out_c1 + i * 64, scratch + 2 * i * 16);
  }
}
// Two kernels with names of their own, not two instantiations of one template: a name has one machine code (srchash.py keys by name).
__global__ void __launch_bounds__(BJJ_ELGAMAL_BLOCK, 1) bjj_k_elgamal_encrypt(const ElgamalArgs A, size_t n, uint8_t* out_c1, uint8_t* out_c2,
                                                                            uint8_t* ok, u32* scratch) {
  elgamal_encrypt_body<false>(A, n, out_c1, out_c2, ok, scratch);
}
__global__ void __launch_bounds__(BJJ_ELGAMAL_BLOCK, 1) bjj_k_elgamal_encrypt_add(const ElgamalArgs A, size_t n, uint8_t* out_c1, uint8_t* out_c2,
                                                                                uint8_t* ok, u32* scratch) {
  elgamal_encrypt_body<true>(A, n, out_c1, out_c2, ok, scratch);
}

// ---- launchers (declared in bjj_launch.hpp) ------------------------------------------------------------
namespace bjjk {
int elgamal_lanes_per_cu() { return lanes_for_both(bjj_k_elgamal_encrypt_add, bjj_k_elgamal_encrypt, BJJ_ELGAMAL_BLOCK); }
hipError_t elgamal_encrypt(hipStream_t st, int cus, int lanes_per_cu, const ElgamalArgs& A, size_t n, uint8_t* out_c1, uint8_t* out_c2,
                           uint8_t* ok, u32* scratch) {
  const int grid = capped_grid(n, BJJ_ELGAMAL_BLOCK, (size_t)cus * (size_t)(lanes_per_cu / BJJ_ELGAMAL_BLOCK));
  if (A.add_c1) BJJ_LAUNCH(bjj_k_elgamal_encrypt_add, dim3(grid), dim3(BJJ_ELGAMAL_BLOCK), 0, st, A, n, out_c1, out_c2, ok, scratch);
  else BJJ_LAUNCH(bjj_k_elgamal_encrypt, dim3(grid), dim3(BJJ_ELGAMAL_BLOCK), 0, st, A, n, out_c1, out_c2, ok, scratch);
  return hipGetLastError();
}
}  // namespace bjjk
