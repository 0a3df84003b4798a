// libbjj_hip.so, kernel unit 13: bjj_point_sum -- m signed point sums Q_s = sum_{i in segment s} +-P_i over the CSR segments of
// one point array (bodies and the description of the levels: point_sum.hpp).  One launch per level of the segmented reduction, one
// item per lane, PSUM_TILE lanes per workgroup; whole segments leave through the workgroup-wide simultaneous inversion.
#include "k_common.hpp"
#include "point_sum.hpp"

#define PSUM_SEG_BLOCK 256   // the two passes over the segments (begin, finish)

// The core the one inverting wave of a workgroup runs (k_common.hpp).  The division-step core against the binary GCD, alternating
// builds in one session: 0.48 against 0.56 ms for 2^20 singletons, 0.63 against 0.69 ms for 2^18 segments of 4.
// A/B: make BUILD=build_x OUT=../../tools/ab_x.so EXTRA="-DPSUM_INV_CORE=INV_GCD"
#ifndef PSUM_INV_CORE
#define PSUM_INV_CORE INV_K1
#endif

// ---- begin: every status word to ~0 (the atomicMin of level 0 needs it) and the offsets contract, which the device form cannot look
// at on the host: any violation sets flag[0].  One lane per k = 0 .. m --------------------------------------------------------------
__global__ void __launch_bounds__(PSUM_SEG_BLOCK) bjj_k_point_sum_begin(const u64* __restrict__ offsets, size_t m, u64 n,
                                                                      unsigned long long* __restrict__ status, u32* __restrict__ flag) {
  const size_t k = (size_t)blockIdx.x * PSUM_SEG_BLOCK + threadIdx.x;
  if (k > m) return;
  if (k < m) status[k] = ~0ull;
  if (!msm_offset_ok(offsets, m, n, k)) atomicOr(flag, 1u);
}

// ---- one level: POINTS = the caller's records (level 0), else the entries of the level before -----------------------------------
// entries == nullptr: the last level, one tile holds the whole list and every run in it is a whole segment.
template <bool POINTS>
__global__ void __launch_bounds__(PSUM_TILE) bjj_k_point_sum_level(const uint8_t* __restrict__ pts, const uint8_t* __restrict__ neg,
                                                                  const u32* __restrict__ in, u64 len, const u64* __restrict__ offsets,
                                                                  size_t m, const u32* __restrict__ flag, u32* __restrict__ entries,
                                                                  uint8_t* __restrict__ out, unsigned long long* __restrict__ status) {
  __shared__ u32 s_val[PSUM_EXT_WORDS * PSUM_TILE];   // 144 B per lane
  __shared__ u32 s_seg[PSUM_TILE], s_live[PSUM_TILE];
  __shared__ u32 s_inv[NL * 64];
  __shared__ u32 s_edge[2];
  if (flag[0] != 0u) return;   // broken offsets: the finish pass answers for every segment (the whole grid leaves, no barrier is split)
  const PsumXch x{s_val, s_seg, s_live, PSUM_TILE};
  const int t = (int)threadIdx.x;
  const u64 lo = (u64)blockIdx.x * PSUM_TILE;
  const u64 hi = lo + PSUM_TILE < len ? lo + PSUM_TILE : len;
  const int cnt = (int)(hi - lo);   // >= 1: the grid is ceil(len / PSUM_TILE)
  const bool valid = t < cnt;
  PsumLane a;
  a.v = ext_identity(); a.seg = PSUM_NO_SEG; a.live = false;
  if (valid) {
    if (POINTS) {
      bool on;
      a = psum_load_point(pts, neg, (size_t)(lo + t), offsets, m, &on, c_K);
      if (!on) atomicMin(status + a.seg, (unsigned long long)(lo + t));   // every word starts at ~0: the smallest offending index wins
    } else {
      a = psum_load_entry(in, (size_t)(lo + t));
    }
    psum_xch_put(x, t, a);
  }
  if (t == 0) s_edge[0] = !entries ? PSUM_NO_SEG : POINTS ? psum_point_neighbour(offsets, m, len, lo, hi, false) : psum_entry_neighbour(in, len, lo, hi, false);
  if (t == cnt - 1) s_edge[1] = !entries ? PSUM_NO_SEG : POINTS ? psum_point_neighbour(offsets, m, len, lo, hi, true) : psum_entry_neighbour(in, len, lo, hi, true);
  __syncthreads();
#pragma unroll 1
  for (int d = 1; d < cnt; d <<= 1) {   // workgroup-uniform trip count
    Ext other;
    const bool take = valid && psum_scan_read(x, t, d, a, other);
    __syncthreads();
    if (take) psum_scan_write(x, t, a, other, c_K);
    __syncthreads();
  }
  u32 what = 0u;
  bool head_live = false, tail_live = false;
  if (valid) what = psum_classify(x, t, cnt, a, s_edge[0], s_edge[1], &head_live, &tail_live);
  if (entries && what) psum_store_entries(entries, blockIdx.x, what, a, head_live, tail_live);
  const bool whole = (what & PSUM_WHOLE) != 0u;
  // a tile inside one long segment has nothing to write: its workgroup does not pay for an inversion (workgroup-uniform: the barrier's or)
  if (!__syncthreads_or(whole ? 1 : 0)) return;
  const Fr zi = block_invert<PSUM_TILE, PSUM_INV_CORE>(whole ? a.v.Z : fr_one(), s_inv);   // the Z of a sum of curve points is never 0
  if (whole) psum_store_result(out + (size_t)a.seg * 64, a.v, zi, c_K);
}

// ---- the segments no run owns: empty, spoiled, or all of them when the offsets are broken -----------------------------------------
__global__ void __launch_bounds__(PSUM_SEG_BLOCK) bjj_k_point_sum_finish(const u64* __restrict__ offsets, size_t m,
                                                                       unsigned long long* __restrict__ status,
                                                                       const u32* __restrict__ flag, uint8_t* __restrict__ out) {
  const size_t s = (size_t)blockIdx.x * PSUM_SEG_BLOCK + threadIdx.x;
  if (s >= m) return;
  psum_finish(offsets, s, status, flag[0] != 0u, out);
}

namespace bjjk {
static size_t psum_up256(size_t v) { return (v + 255) & ~(size_t)255; }
PointSumLayout point_sum_layout(size_t n) {
  PointSumLayout L;
  const uint64_t tiles0 = n ? psum_tiles(n, PSUM_TILE) : 0, tiles1 = tiles0 > 1 ? psum_tiles(2 * tiles0, PSUM_TILE) : 0;
  L.levels = n ? psum_level_count(n, PSUM_TILE) : 0;
  L.o_flag = 0;
  L.o_e0 = 256;
  L.o_e1 = L.o_e0 + psum_up256((size_t)(tiles0 > 1 ? 2 * tiles0 : 0) * MSM_ENTRY_WORDS * 4);
  L.bytes = L.o_e1 + psum_up256((size_t)(tiles1 > 1 ? 2 * tiles1 : 0) * MSM_ENTRY_WORDS * 4);
  return L;
}
#define PSUM_CK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)
hipError_t point_sum(hipStream_t st, const PointSumLayout& L, const uint8_t* pts, const uint8_t* neg, size_t n, const uint64_t* offsets,
                     size_t m, uint8_t* scratch, uint8_t* out, unsigned long long* status) {
  u32* flag = (u32*)(scratch + L.o_flag);
  u32* e[2] = {(u32*)(scratch + L.o_e0), (u32*)(scratch + L.o_e1)};
  const unsigned seg_blocks = (unsigned)(((uint64_t)m + PSUM_SEG_BLOCK - 1) / PSUM_SEG_BLOCK);
  PSUM_CK(hipMemsetAsync(flag, 0, 8, st));
  BJJ_LAUNCH(bjj_k_point_sum_begin, dim3((unsigned)(((uint64_t)m + 1 + PSUM_SEG_BLOCK - 1) / PSUM_SEG_BLOCK)), dim3(PSUM_SEG_BLOCK), 0, st,
             (const u64*)offsets, m, (u64)n, status, flag);
  PSUM_CK(hipGetLastError());
  uint64_t len = n;
  for (int l = 0; l < L.levels; l++) {
    const uint64_t tiles = psum_tiles(len, PSUM_TILE);
    u32* entries = tiles > 1 ? e[l & 1] : nullptr;   // level l reads e[(l - 1) & 1] and writes e[l & 1]
    if (l == 0)
      BJJ_LAUNCH(bjj_k_point_sum_level<true>, dim3((unsigned)tiles), dim3(PSUM_TILE), 0, st, pts, neg, (const u32*)nullptr, (u64)len,
                 (const u64*)offsets, m, (const u32*)flag, entries, out, status);
    else
      BJJ_LAUNCH(bjj_k_point_sum_level<false>, dim3((unsigned)tiles), dim3(PSUM_TILE), 0, st, (const uint8_t*)nullptr, (const uint8_t*)nullptr,
                 (const u32*)e[(l - 1) & 1], (u64)len, (const u64*)offsets, m, (const u32*)flag, entries, out, status);
    PSUM_CK(hipGetLastError());
    len = 2 * tiles;
  }
  BJJ_LAUNCH(bjj_k_point_sum_finish, dim3(seg_blocks), dim3(PSUM_SEG_BLOCK), 0, st, (const u64*)offsets, m, status, (const u32*)flag, out);
  return hipGetLastError();
}
}  // namespace bjjk
