// libbjj_hip.so, kernel unit 7: bjj_msm -- Q = sum k_i * P_i by Pippenger's bucket method (bodies and pipeline: msm.hpp).
// No reference counterpart: the result equals the fold acc = acc.add(&P_i.mul_scalar(k_i).projective()) from (0, 1, 1), then
// .affine() (src/lib.rs:149-164, 88-131, 70-85), for on-curve points; an off-curve point makes the call's result (0, 0) and its
// index the status word.
#include "k_msm_common.hpp"

#define MSM_SCAN_PER_THREAD 16
#define MSM_SCAN_TILE (MSM_BLOCK * MSM_SCAN_PER_THREAD)
#define MSM_TOP_BLOCK 1024

// ---- 1. prepare: on-curve check, Niels points, reduced scalars, histogram -----------------------------------------------------
__global__ void __launch_bounds__(MSM_BLOCK) bjj_k_msm_prepare(const uint8_t* __restrict__ pts, const uint8_t* __restrict__ scalars, size_t n,
                                                              int c, u32* __restrict__ niels, u32* __restrict__ red, u32* __restrict__ counts,
                                                              unsigned long long* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * MSM_BLOCK + threadIdx.x;
  const bool valid = i < n;
  u32 k[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (valid) {
    const bool on = msm_prepare_point(pts + i * 64, niels + i * NIELS_WORDS, c_K);
    if (!on) atomicMin(status, (unsigned long long)i);   // status starts at ~0 (= -1 as int64): the smallest offending index wins
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
    wave_counter_add<u32>(counts, (u32)j * B + b - 1u, valid && b != 0);
  }
}

// ---- 2. exclusive scan of the histogram into the scatter cursors --------------------------------------------------------------
// exclusive prefix over the block of v (u64), and the block total
template <int BLOCK>
__device__ __forceinline__ u64 block_exclusive_scan(u64 v, u64* lds, u64& total) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
#pragma unroll 1
  for (int d = 1; d < BLOCK; d <<= 1) {
    const u64 add = t >= d ? lds[t - d] : 0ull;
    __syncthreads();
    lds[t] += add;
    __syncthreads();
  }
  const u64 incl = lds[t];
  total = lds[BLOCK - 1];
  __syncthreads();
  return incl - v;
}
__global__ void __launch_bounds__(MSM_BLOCK) bjj_k_msm_scan_tiles(const u32* __restrict__ counts, size_t M, u64* __restrict__ bsum) {
  __shared__ u64 lds[MSM_BLOCK];
  const size_t base = (size_t)blockIdx.x * MSM_SCAN_TILE + (size_t)threadIdx.x * MSM_SCAN_PER_THREAD;
  u64 s = 0;
#pragma unroll
  for (int e = 0; e < MSM_SCAN_PER_THREAD; e++) s += base + e < M ? counts[base + e] : 0u;
  u64 total;
  block_exclusive_scan<MSM_BLOCK>(s, lds, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
// one workgroup: bsum[b] <- exclusive prefix; total[0] <- number of records
__global__ void __launch_bounds__(MSM_TOP_BLOCK) bjj_k_msm_scan_top(u64* __restrict__ bsum, size_t nb, u64* __restrict__ total) {
  __shared__ u64 lds[MSM_TOP_BLOCK];
  u64 carry = 0;
#pragma unroll 1
  for (size_t c0 = 0; c0 < nb; c0 += MSM_TOP_BLOCK) {
    const size_t b = c0 + threadIdx.x;
    const u64 v = b < nb ? bsum[b] : 0ull;
    u64 chunk;
    const u64 ex = block_exclusive_scan<MSM_TOP_BLOCK>(v, lds, chunk);
    if (b < nb) bsum[b] = carry + ex;
    carry += chunk;
  }
  if (threadIdx.x == 0) total[0] = carry;
}
__global__ void __launch_bounds__(MSM_BLOCK) bjj_k_msm_scan_apply(const u32* __restrict__ counts, size_t M, const u64* __restrict__ bsum,
                                                                 u64* __restrict__ cursor) {
  __shared__ u64 lds[MSM_BLOCK];
  const size_t base = (size_t)blockIdx.x * MSM_SCAN_TILE + (size_t)threadIdx.x * MSM_SCAN_PER_THREAD;
  u32 v[MSM_SCAN_PER_THREAD];
  u64 s = 0;
#pragma unroll
  for (int e = 0; e < MSM_SCAN_PER_THREAD; e++) { v[e] = base + e < M ? counts[base + e] : 0u; s += v[e]; }
  u64 total;
  u64 run = bsum[blockIdx.x] + block_exclusive_scan<MSM_BLOCK>(s, lds, total);
#pragma unroll
  for (int e = 0; e < MSM_SCAN_PER_THREAD; e++) {
    if (base + e < M) cursor[base + e] = run;
    run += v[e];
  }
}

// ---- 3. scatter: (key, item, sign) records in key order -------------------------------------------------------------------------
__global__ void __launch_bounds__(MSM_BLOCK) bjj_k_msm_scatter(const u32* __restrict__ red, size_t n, int c, u64* __restrict__ cursor,
                                                              u64* __restrict__ rec) {
  const size_t i = (size_t)blockIdx.x * MSM_BLOCK + threadIdx.x;
  const bool valid = i < n;
  u32 k[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (valid) load_w8(red + i * 8, k);
  const int W = msm_windows(c);
  const u32 B = msm_buckets(c);
  u32 carry = 0;
#pragma unroll 1
  for (int j = 0; j < W; j++) {
    const int d = msm_digit(k, j, c, carry);
    const u32 b = (u32)(d < 0 ? -d : d);
    const u32 key = (u32)j * B + b - 1u;
    const bool active = valid && b != 0;
    const u64 pos = wave_counter_add<u64>(cursor, key, active);
    if (active) rec[pos] = msm_record(key, (u32)i, d < 0);
  }
}

// ---- 4. bucket accumulation: fixed-size slices of the sorted records, then of the partials ----------------------------------------
__global__ void __launch_bounds__(MSM_BLOCK) bjj_k_msm_slices(const u64* __restrict__ rec, const u64* __restrict__ total, u64 nslices, u32 S,
                                                             const u32* __restrict__ niels, u32* __restrict__ buckets, u32* __restrict__ out) {
  const u64 s = (u64)blockIdx.x * MSM_BLOCK + threadIdx.x;
  if (s >= nslices) return;
  msm_slice_records(rec, total[0], s, S, niels, buckets, out, c_K);
}
__global__ void __launch_bounds__(MSM_BLOCK) bjj_k_msm_level(const u32* __restrict__ in, u64 len, u64 nslices, u32* __restrict__ buckets,
                                                            u32* __restrict__ out) {
  const u64 s = (u64)blockIdx.x * MSM_BLOCK + threadIdx.x;
  if (s >= nslices) return;
  msm_slice_entries(in, len, s, MSM_LEVEL_SLICE, buckets, out, c_K);
}

// ---- 5. buckets -> window sums ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MSM_BLOCK) bjj_k_msm_windows(const u32* __restrict__ buckets, const u32* __restrict__ counts, int c, u32 G,
                                                              u64 nseg, u32* __restrict__ out) {
  const u64 t = (u64)blockIdx.x * MSM_BLOCK + threadIdx.x;
  if (t >= nseg) return;
  const Ext v = msm_window_segment(buckets, counts, (int)(t / G), (u32)(t % G), c, c_K);
  msm_store_ext(out + (size_t)t * MSM_ENTRY_WORDS, v);
}
__global__ void __launch_bounds__(MSM_BLOCK) bjj_k_msm_group(const u32* __restrict__ in, u64 nout, u32 F, u32* __restrict__ out) {
  const u64 i = (u64)blockIdx.x * MSM_BLOCK + threadIdx.x;
  if (i >= nout) return;
  msm_store_ext(out + (size_t)i * MSM_ENTRY_WORDS, msm_group_sum(in, i, F, c_K));
}

// ---- 6. Horner over the windows, affine, canonical bytes (one lane) --------------------------------------------------------------
__global__ void __launch_bounds__(64) bjj_k_msm_finish(const u32* __restrict__ wsum, int W, int c, const unsigned long long* __restrict__ status,
                                                      uint8_t* __restrict__ out) {
  if (threadIdx.x != 0) return;
  msm_finish(wsum, W, c, status[0] != ~0ull, out, c_K);
}

namespace bjjk {
static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
static unsigned blocks(u64 items, int block = MSM_BLOCK) { return (unsigned)((items + block - 1) / block); }
// Slice of the record level: the records of a call are n W at most; slices of 8 .. 64 records, as long as that leaves about 2^18
// slices (one lane each) -- a longer serial chain per lane where there are lanes to spare would only add latency.
static u32 slice_records(u64 records) {
  u32 S = 8;
  while (S < 64 && records / S > ((u64)1 << 18)) S <<= 1;
  return S;
}
// one layout for both forms: m segments (bjj_msm: 1) share the item arrays; every per-window array holds m W windows
static MsmLayout layout(size_t n, size_t m, int c) {
  MsmLayout L = {};
  L.c = c; L.W = msm_windows(c);
  L.m = m; L.nwin = (u64)m * L.W;
  const u64 B = msm_buckets(c), M = L.nwin * B;
  L.keys = M;
  L.records = (u64)n * L.W;
  L.S1 = slice_records(L.records);
  L.slices1 = msm_div_up(L.records ? L.records : 1, L.S1);
  L.levels = msm_level_count(L.records, L.S1);
  L.G = (u32)(B / MSM_SEG);
  const u64 len2 = 2 * L.slices1, slices2 = msm_div_up(len2, MSM_LEVEL_SLICE);
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += up256(bytes ? bytes : 1); return o; };
  L.o_niels = take(n * 128);
  L.o_red = take(n * 32);
  L.o_counts = take(M * 4);
  L.o_cursor = take(M * 8);
  L.nb = msm_div_up(M, MSM_SCAN_TILE);
  L.o_bsum = take(L.nb * 8);
  L.o_total = take(8);
  L.o_status = take(m * 8);
  L.o_out = take(m * 64);
  L.o_rec = take(L.records * 8);
  L.o_e0 = take(len2 * MSM_ENTRY_WORDS * 4);
  L.o_e1 = take(2 * slices2 * MSM_ENTRY_WORDS * 4);
  L.o_buckets = take(M * MSM_ENTRY_WORDS * 4);
  L.o_w0 = take(L.nwin * L.G * MSM_ENTRY_WORDS * 4);
  L.o_w1 = take(L.nwin * msm_div_up(L.G, MSM_GROUP) * MSM_ENTRY_WORDS * 4);
  L.o_offsets = take((m + 1) * 8);
  L.o_flag = take(8);
  L.o_seg = take(n * 4);
  L.bytes = off;
  return L;
}
MsmLayout msm_layout(size_t n, int c) { return layout(n, 1, c); }
MsmLayout msm_batch_layout(size_t n, size_t m, int c) { return layout(n, m ? m : 1, c); }

#define MSM_CK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)
// 2. the histogram in `counts` -> scatter cursors and the record total
hipError_t msm_scan(hipStream_t st, const MsmLayout& L, uint8_t* scratch) {
  u32* counts = (u32*)(scratch + L.o_counts);
  u64* cursor = (u64*)(scratch + L.o_cursor);
  u64* bsum = (u64*)(scratch + L.o_bsum);
  u64* total = (u64*)(scratch + L.o_total);
  BJJ_LAUNCH(bjj_k_msm_scan_tiles, dim3((unsigned)L.nb), dim3(MSM_BLOCK), 0, st, (const u32*)counts, (size_t)L.keys, bsum);
  MSM_CK(hipGetLastError());
  BJJ_LAUNCH(bjj_k_msm_scan_top, dim3(1), dim3(MSM_TOP_BLOCK), 0, st, bsum, (size_t)L.nb, total);
  MSM_CK(hipGetLastError());
  BJJ_LAUNCH(bjj_k_msm_scan_apply, dim3((unsigned)L.nb), dim3(MSM_BLOCK), 0, st, (const u32*)counts, (size_t)L.keys, (const u64*)bsum, cursor);
  return hipGetLastError();
}
// 4. + 5. the sorted records -> buckets -> one sum per window; *wsum: the L.nwin window sums (entry stride)
hipError_t msm_reduce(hipStream_t st, const MsmLayout& L, uint8_t* scratch, const uint32_t** wsum) {
  u32* niels = (u32*)(scratch + L.o_niels);
  u32* counts = (u32*)(scratch + L.o_counts);
  u64* total = (u64*)(scratch + L.o_total);
  u64* rec = (u64*)(scratch + L.o_rec);
  u32* e[2] = {(u32*)(scratch + L.o_e0), (u32*)(scratch + L.o_e1)};
  u32* buckets = (u32*)(scratch + L.o_buckets);
  u32* w[2] = {(u32*)(scratch + L.o_w0), (u32*)(scratch + L.o_w1)};
  BJJ_LAUNCH(bjj_k_msm_slices, dim3(blocks(L.slices1)), dim3(MSM_BLOCK), 0, st, (const u64*)rec, (const u64*)total, L.slices1, L.S1,
             (const u32*)niels, buckets, e[0]);
  MSM_CK(hipGetLastError());
  u64 len = 2 * L.slices1;
  for (int l = 0; l < L.levels; l++) {   // ping-pong: level l reads e[l & 1], writes e[(l + 1) & 1] (every later list is shorter)
    const u64 ns = msm_div_up(len, MSM_LEVEL_SLICE);
    BJJ_LAUNCH(bjj_k_msm_level, dim3(blocks(ns)), dim3(MSM_BLOCK), 0, st, (const u32*)e[l & 1], len, ns, buckets, e[(l + 1) & 1]);
    MSM_CK(hipGetLastError());
    len = 2 * ns;
  }
  const u64 nseg = L.nwin * L.G;
  BJJ_LAUNCH(bjj_k_msm_windows, dim3(blocks(nseg)), dim3(MSM_BLOCK), 0, st, (const u32*)buckets, (const u32*)counts, L.c, L.G, nseg, w[0]);
  MSM_CK(hipGetLastError());
  int cur = 0;
  for (u32 g = L.G; g > 1;) {   // G is a power of two: groups never straddle two windows
    const u32 F = g < (u32)MSM_GROUP ? g : (u32)MSM_GROUP;
    g /= F;
    const u64 nout = L.nwin * g;
    BJJ_LAUNCH(bjj_k_msm_group, dim3(blocks(nout)), dim3(MSM_BLOCK), 0, st, (const u32*)w[cur], nout, F, w[cur ^ 1]);
    MSM_CK(hipGetLastError());
    cur ^= 1;
  }
  *wsum = w[cur];
  return hipSuccess;
}
hipError_t msm(hipStream_t st, const MsmLayout& L, const uint8_t* pts, const uint8_t* scalars, size_t n, uint8_t* scratch, uint8_t* out,
               unsigned long long* status) {
  u32* niels = (u32*)(scratch + L.o_niels);
  u32* red = (u32*)(scratch + L.o_red);
  u32* counts = (u32*)(scratch + L.o_counts);
  u64* cursor = (u64*)(scratch + L.o_cursor);
  u64* rec = (u64*)(scratch + L.o_rec);
  MSM_CK(hipMemsetAsync(status, 0xff, sizeof(unsigned long long), st));
  if (n == 0) {   // the identity (0, 1): Horner over no windows
    BJJ_LAUNCH(bjj_k_msm_finish, dim3(1), dim3(64), 0, st, (const u32*)(scratch + L.o_w0), 0, L.c, (const unsigned long long*)status, out);
    return hipGetLastError();
  }
  MSM_CK(hipMemsetAsync(counts, 0, L.keys * 4, st));
  BJJ_LAUNCH(bjj_k_msm_prepare, dim3(blocks(n)), dim3(MSM_BLOCK), 0, st, pts, scalars, n, L.c, niels, red, counts, status);
  MSM_CK(hipGetLastError());
  MSM_CK(msm_scan(st, L, scratch));
  BJJ_LAUNCH(bjj_k_msm_scatter, dim3(blocks(n)), dim3(MSM_BLOCK), 0, st, (const u32*)red, n, L.c, cursor, rec);
  MSM_CK(hipGetLastError());
  const u32* wsum = nullptr;
  MSM_CK(msm_reduce(st, L, scratch, &wsum));
  BJJ_LAUNCH(bjj_k_msm_finish, dim3(1), dim3(64), 0, st, wsum, L.W, L.c, (const unsigned long long*)status, out);
  return hipGetLastError();
}
}  // namespace bjjk
