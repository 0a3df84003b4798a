// Shared by the MSM kernel units (k_msm.hip: bjj_msm, k_msm_batch.hip: bjj_msm_batch): the workgroup size and the wave-aggregated
// counters of the two passes that form sort keys.
#pragma once
#include "k_common.hpp"
#include "msm.hpp"

#define MSM_BLOCK 256

// ---- wave-aggregated counters ------------------------------------------------------------------------------------------------
// arr[key] += 1 for every active lane, returning the lane's old value.  The caller controls the scalars, so a whole wave may name
// ONE key (all scalars equal, every digit in one bucket), and even random scalars give the top window only a handful of values
// when c does not divide 255 evenly: each round serves the lanes that share the first pending lane's key with ONE atomic (rank by
// popcount), and the rounds go on while they serve at least 4 lanes; the rest (distinct keys) take one atomic each.  Same-address
// atomics of a wave would otherwise queue at one L2 channel (2^20 items, c = 14: 3.3 ms for the histogram alone).  All 64 lanes of
// the wave call this together.
template <typename T>
__device__ __forceinline__ T wave_counter_add(T* arr, u32 key, bool active) {
  const int lane = (int)(threadIdx.x & 63);
  const u64 below = (1ull << lane) - 1ull;
  bool pending = active;
  T pos = 0;
#pragma unroll 1
  for (int round = 0; round < 64; round++) {
    const u64 m = __ballot(pending);
    if (m == 0) break;
    const int leader = __ffsll((long long)m) - 1;
    const u32 lkey = (u32)__shfl((int)key, leader, 64);
    const bool mine = pending && key == lkey;
    const u64 grp = __ballot(mine);
    T base = 0;
    if (lane == leader) base = atomicAdd(&arr[lkey], (T)__popcll(grp));
    u64 b64 = (u64)base;
    const u32 lo = (u32)__shfl((int)(u32)b64, leader, 64), hi = (u32)__shfl((int)(u32)(b64 >> 32), leader, 64);
    if (mine) { pos = (T)((((u64)hi << 32) | lo) + (u64)__popcll(grp & below)); pending = false; }
    if (__popcll(grp) < 4) break;
  }
  if (pending) pos = atomicAdd(&arr[key], (T)1);
  return pos;
}
