// libbjj_hip.so, kernel unit 8: bjj_msm_batch -- m independent sums Q_s = sum_{i in segment s} k_i * P_i in ONE launch chain
// (bodies: msm.hpp, "batched form").  Segment s is the index range [offsets[s], offsets[s + 1]) of one point / scalar array (CSR).
// The sort key carries the segment, key = (s W + j) B + |d| - 1, so the scan, the slice / level reduction and the window sums of
// k_msm.hip run as they are over m W "windows" (bjjk::msm_scan, bjjk::msm_reduce); this unit holds the two passes that form
// keys, the offsets check and the finish, which runs the Horner chain of every segment on a lane of its own.
#include "k_msm_common.hpp"

#define MSM_FINISH_BLOCK 64   // one lane per segment; small workgroups spread few segments over many CUs

// ---- 0. the offsets contract (the device form cannot look at them on the host): any violation sets flag[0] --------------------
__global__ void __launch_bounds__(MSM_BLOCK) bjj_k_msm_batch_check_offsets(const u64* __restrict__ offsets, size_t m, u64 n,
                                                                          u32* __restrict__ flag) {
  const size_t k = (size_t)blockIdx.x * MSM_BLOCK + threadIdx.x;
  if (k > m) return;
  if (!msm_offset_ok(offsets, m, n, k)) atomicOr(flag, 1u);
}

// ---- 1. prepare: as bjj_k_msm_prepare, with the item's segment in the key and in the status word ------------------------------
__global__ void __launch_bounds__(MSM_BLOCK) bjj_k_msm_batch_prepare(const uint8_t* __restrict__ pts, const uint8_t* __restrict__ scalars,
                                                                    size_t n, const u64* __restrict__ offsets, size_t m, int c,
                                                                    u32* __restrict__ niels, u32* __restrict__ red, u32* __restrict__ seg,
                                                                    u32* __restrict__ counts, unsigned long long* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * MSM_BLOCK + threadIdx.x;
  const bool valid = i < n;
  u32 k[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  u32 s = 0;
  if (valid) {
    s = msm_find_segment(offsets, m, (u64)i);   // in [0, m - 1] whatever offsets[] holds
    seg[i] = s;
    const bool on = msm_prepare_point(pts + i * 64, niels + i * NIELS_WORDS, c_K);
    if (!on) atomicMin(status + s, (unsigned long long)i);   // every word starts at ~0: the smallest offending index of the segment wins
    msm_prepare_scalar(scalars + i * 32, on, k, c_K);
    store_w8(red + i * 8, k);
  }
  const int W = msm_windows(c);
  const u32 B = msm_buckets(c);
  u32 carry = 0;
#pragma unroll 1
  for (int j = 0; j < W; j++) {   // wave-uniform trip count: wave_counter_add needs every lane
    const int d = msm_digit(k, j, c, carry);
    const u32 b = (u32)(d < 0 ? -d : d);
    // the FULL key goes into the aggregation: two lanes with one digit in two segments are two counters
    wave_counter_add<u32>(counts, msm_batch_key(s, W, j, B, b), valid && b != 0);
  }
}

// ---- 3. scatter: as bjj_k_msm_scatter; the segment comes from the word prepare left (no second search) ------------------------
__global__ void __launch_bounds__(MSM_BLOCK) bjj_k_msm_batch_scatter(const u32* __restrict__ red, const u32* __restrict__ seg, size_t n, int c,
                                                                    u64* __restrict__ cursor, u64* __restrict__ rec) {
  const size_t i = (size_t)blockIdx.x * MSM_BLOCK + threadIdx.x;
  const bool valid = i < n;
  u32 k[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  u32 s = 0;
  if (valid) { load_w8(red + i * 8, k); s = seg[i]; }
  const int W = msm_windows(c);
  const u32 B = msm_buckets(c);
  u32 carry = 0;
#pragma unroll 1
  for (int j = 0; j < W; j++) {
    const int d = msm_digit(k, j, c, carry);
    const u32 b = (u32)(d < 0 ? -d : d);
    const u32 key = msm_batch_key(s, W, j, B, b);
    const bool active = valid && b != 0;
    const u64 pos = wave_counter_add<u64>(cursor, key, active);
    if (active) rec[pos] = msm_record(key, (u32)i, d < 0);
  }
}

// ---- 6. finish: one lane per segment -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MSM_FINISH_BLOCK) bjj_k_msm_batch_finish(const u32* __restrict__ wsum, size_t m, int W, int c,
                                                                          unsigned long long* __restrict__ status,
                                                                          const u32* __restrict__ flag, uint8_t* __restrict__ out) {
  const size_t s = (size_t)blockIdx.x * MSM_FINISH_BLOCK + threadIdx.x;
  if (s >= m) return;
  msm_batch_finish(wsum, s, W, c, status, flag[0] != 0u, out, c_K);
}

namespace bjjk {
static unsigned blocks(u64 items, int block = MSM_BLOCK) { return (unsigned)((items + block - 1) / block); }
#define MSM_CK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)
hipError_t msm_batch(hipStream_t st, const MsmLayout& L, const uint8_t* pts, const uint8_t* scalars, size_t n, const uint64_t* offsets,
                     size_t m, uint8_t* scratch, uint8_t* out, unsigned long long* status) {
  u32* niels = (u32*)(scratch + L.o_niels);
  u32* red = (u32*)(scratch + L.o_red);
  u32* counts = (u32*)(scratch + L.o_counts);
  u64* cursor = (u64*)(scratch + L.o_cursor);
  u64* rec = (u64*)(scratch + L.o_rec);
  u32* flag = (u32*)(scratch + L.o_flag);
  u32* seg = (u32*)(scratch + L.o_seg);
  MSM_CK(hipMemsetAsync(status, 0xff, m * sizeof(unsigned long long), st));
  MSM_CK(hipMemsetAsync(flag, 0, 8, st));
  BJJ_LAUNCH(bjj_k_msm_batch_check_offsets, dim3(blocks((u64)m + 1)), dim3(MSM_BLOCK), 0, st, (const u64*)offsets, m, (u64)n, flag);
  MSM_CK(hipGetLastError());
  if (n == 0) {   // every segment is empty: the identity (0, 1), Horner over no windows
    BJJ_LAUNCH(bjj_k_msm_batch_finish, dim3(blocks(m, MSM_FINISH_BLOCK)), dim3(MSM_FINISH_BLOCK), 0, st, (const u32*)(scratch + L.o_w0), m, 0,
               L.c, status, (const u32*)flag, out);
    return hipGetLastError();
  }
  MSM_CK(hipMemsetAsync(counts, 0, L.keys * 4, st));
  BJJ_LAUNCH(bjj_k_msm_batch_prepare, dim3(blocks(n)), dim3(MSM_BLOCK), 0, st, pts, scalars, n, (const u64*)offsets, m, L.c, niels, red, seg,
             counts, status);
  MSM_CK(hipGetLastError());
  MSM_CK(msm_scan(st, L, scratch));
  BJJ_LAUNCH(bjj_k_msm_batch_scatter, dim3(blocks(n)), dim3(MSM_BLOCK), 0, st, (const u32*)red, (const u32*)seg, n, L.c, cursor, rec);
  MSM_CK(hipGetLastError());
  const u32* wsum = nullptr;
  MSM_CK(msm_reduce(st, L, scratch, &wsum));
  BJJ_LAUNCH(bjj_k_msm_batch_finish, dim3(blocks(m, MSM_FINISH_BLOCK)), dim3(MSM_FINISH_BLOCK), 0, st, wsum, m, L.W, L.c, status,
             (const u32*)flag, out);
  return hipGetLastError();
}
}  // namespace bjjk
