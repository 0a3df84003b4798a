// TEST-ONLY library (not part of libbjj_hip.so): the two MSM kernel units csrc/k_msm.hip and csrc/k_msm_batch.hip as they ship --
// their kernels, their launchers, the product's flags -- run ONE STAGE PER CALL on a scratch block the caller owns, so that
// tests/test_gpu_msm_stages.py can read every intermediate array (red, niels, counts, cursor, rec, buckets, window sums) between
// the stages and hold it against the plain-integer model of tests/msm_ref.py.  Nothing of the product is restated here: the calls
// below only compute the product's MsmLayout and hand scratch + offsets to the product's kernels and launchers.  One kernel stands
// BESIDE the product's: mt_counter_kernel, MSM_BLOCK lanes per workgroup, every lane calling wave_counter_add<T> once on a key and
// an active flag of the test's choice and storing what it returns.
// Scratch: mt_layout(...)[bytes] bytes of device memory, 256-byte aligned.  The item arrays (pts: n 64-byte records, scalars: n
// 32-byte records) are the caller's device memory.  Every call validates its arguments on the host and returns -1 without a launch
// when they fail; -3 is a launch error.  The S1 argument: 0 = the product's slice size, 16 / 32 / 64 = that slice size in the
// regions the product laid out for its own choice of 8 (a larger slice only shortens the lists).
#include "../../babyjubjub-rs_amd/csrc/k_msm.hip"
// the two units are separate translation units in the product and each has its own file-local bjjk::blocks and MSM_CK: in this one
// translation unit the second unit's copy goes by another name (the text of the unit is untouched)
#undef MSM_CK
#define blocks blocks_of_the_batch_unit
#include "../../babyjubjub-rs_amd/csrc/k_msm_batch.hip"
#undef blocks
using bjjk::MsmLayout;

#define MT_EXPORT extern "C" __attribute__((visibility("default")))
#define MT_FIELDS 26
#define MT_MAX_N ((size_t)1 << 20)
#define MT_MAX_M ((size_t)1 << 12)
#define MT_MAX_KEYS ((u64)1 << 25)

static int mt_rc(hipError_t e) { return e == hipSuccess ? 0 : -3; }

// the product's layout for (n, m, c), with the slice size overridden on request; false: arguments the harness refuses
static bool mt_make_layout(size_t n, size_t m, int c, unsigned S1, MsmLayout& L) {
  if (n < 1 || n > MT_MAX_N || m < 1 || m > MT_MAX_M || c < MSM_MIN_C || c > MSM_MAX_C) return false;
  if (S1 != 0 && S1 != 16 && S1 != 32 && S1 != 64) return false;
  L = m == 1 ? bjjk::msm_layout(n, c) : bjjk::msm_batch_layout(n, m, c);
  if (L.keys > MT_MAX_KEYS) return false;
  if (S1 != 0) {
    if (L.S1 != 8) return false;   // the regions are sized for the product's choice: only its smallest may be widened
    L.S1 = S1;
    L.slices1 = msm_div_up(L.records ? L.records : 1, L.S1);
    L.levels = msm_level_count(L.records, L.S1);
  }
  return true;
}
static bool mt_block_ok(const void* scratch, size_t scratch_bytes, const MsmLayout& L) {
  return scratch && ((uintptr_t)scratch & 255) == 0 && scratch_bytes >= L.bytes;
}

// out_fields: MT_FIELDS 64-bit words -- o_niels, o_red, o_counts, o_cursor, o_bsum, o_total, o_status, o_out, o_rec, o_e0, o_e1,
// o_buckets, o_w0, o_w1, o_offsets, o_flag, o_seg, bytes, W, G, keys, records, S1, slices1, levels, nb
MT_EXPORT int mt_layout(size_t n, size_t m, int c, unsigned S1, unsigned long long* out_fields) {
  MsmLayout L;
  if (!out_fields || !mt_make_layout(n, m, c, S1, L)) return -1;
  const unsigned long long f[MT_FIELDS] = {L.o_niels, L.o_red, L.o_counts, L.o_cursor, L.o_bsum, L.o_total, L.o_status, L.o_out, L.o_rec,
                                           L.o_e0, L.o_e1, L.o_buckets, L.o_w0, L.o_w1, L.o_offsets, L.o_flag, L.o_seg, L.bytes,
                                           (unsigned long long)L.W, L.G, L.keys, L.records, L.S1, L.slices1, (unsigned long long)L.levels, L.nb};
  for (int i = 0; i < MT_FIELDS; i++) out_fields[i] = f[i];
  return 0;
}
MT_EXPORT int mt_fields(void) { return MT_FIELDS; }
MT_EXPORT int mt_block(void) { return MSM_BLOCK; }
MT_EXPORT int mt_scan_tile(void) { return MSM_SCAN_TILE; }
MT_EXPORT int mt_top_block(void) { return MSM_TOP_BLOCK; }
MT_EXPORT int mt_entry_words(void) { return MSM_ENTRY_WORDS; }
MT_EXPORT int mt_level_count(unsigned long long records, unsigned S1) { return S1 ? msm_level_count(records, S1) : -1; }

// ---- 1. prepare, after the product's memsets of the status word(s) and of the histogram ------------------------------------------
MT_EXPORT int mt_prepare(uint8_t* scratch, size_t scratch_bytes, const uint8_t* pts, const uint8_t* scalars, size_t n, int c, void* stream) {
  MsmLayout L;
  if (!pts || !scalars || !mt_make_layout(n, 1, c, 0, L) || !mt_block_ok(scratch, scratch_bytes, L)) return -1;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* status = (unsigned long long*)(scratch + L.o_status);
  u32* counts = (u32*)(scratch + L.o_counts);
  if (hipMemsetAsync(status, 0xff, sizeof(unsigned long long), st) != hipSuccess) return -3;
  if (hipMemsetAsync(counts, 0, L.keys * 4, st) != hipSuccess) return -3;
  BJJ_LAUNCH(bjj_k_msm_prepare, dim3(bjjk::blocks(n)), dim3(MSM_BLOCK), 0, st, pts, scalars, n, L.c, (u32*)(scratch + L.o_niels),
             (u32*)(scratch + L.o_red), counts, status);
  return mt_rc(hipGetLastError());
}
// the m + 1 offsets are read from scratch + o_offsets (device memory, written by the caller): any content is safe for the kernels
MT_EXPORT int mt_batch_prepare(uint8_t* scratch, size_t scratch_bytes, const uint8_t* pts, const uint8_t* scalars, size_t n, size_t m, int c,
                               void* stream) {
  MsmLayout L;
  if (!pts || !scalars || !mt_make_layout(n, m, c, 0, L) || !mt_block_ok(scratch, scratch_bytes, L)) return -1;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* status = (unsigned long long*)(scratch + L.o_status);
  u32* counts = (u32*)(scratch + L.o_counts);
  u32* flag = (u32*)(scratch + L.o_flag);
  const u64* offsets = (const u64*)(scratch + L.o_offsets);
  if (hipMemsetAsync(status, 0xff, m * sizeof(unsigned long long), st) != hipSuccess) return -3;
  if (hipMemsetAsync(flag, 0, 8, st) != hipSuccess) return -3;
  BJJ_LAUNCH(bjj_k_msm_batch_check_offsets, dim3(bjjk::blocks((u64)m + 1)), dim3(MSM_BLOCK), 0, st, offsets, m, (u64)n, flag);
  if (hipGetLastError() != hipSuccess) return -3;
  if (hipMemsetAsync(counts, 0, L.keys * 4, st) != hipSuccess) return -3;
  BJJ_LAUNCH(bjj_k_msm_batch_prepare, dim3(bjjk::blocks(n)), dim3(MSM_BLOCK), 0, st, pts, scalars, n, offsets, m, L.c,
             (u32*)(scratch + L.o_niels), (u32*)(scratch + L.o_red), (u32*)(scratch + L.o_seg), counts, status);
  return mt_rc(hipGetLastError());
}

// ---- 2. scan ------------------------------------------------------------------------------------------------------------------
MT_EXPORT int mt_scan(uint8_t* scratch, size_t scratch_bytes, size_t n, size_t m, int c, void* stream) {
  MsmLayout L;
  if (!mt_make_layout(n, m, c, 0, L) || !mt_block_ok(scratch, scratch_bytes, L)) return -1;
  return mt_rc(bjjk::msm_scan((hipStream_t)stream, L, scratch));
}
// bjjk::msm_scan over a histogram of any length M: counts (M u32), cursor (M u64), bsum (ceil(M / MSM_SCAN_TILE) u64), total (1 u64)
// are four device arrays of the caller; the layout holds only keys, nb and their four offsets from the lowest of the addresses
MT_EXPORT int mt_scan_only(const uint32_t* counts, size_t M, unsigned long long* cursor, unsigned long long* bsum, unsigned long long* total,
                           void* stream) {
  if (!counts || !cursor || !bsum || !total || M < 1 || M > MT_MAX_KEYS) return -1;
  if (((uintptr_t)counts & 3) || ((uintptr_t)cursor & 7) || ((uintptr_t)bsum & 7) || ((uintptr_t)total & 7)) return -1;
  uintptr_t base = (uintptr_t)counts;
  for (uintptr_t p : {(uintptr_t)cursor, (uintptr_t)bsum, (uintptr_t)total}) base = p < base ? p : base;
  MsmLayout L = {};
  L.keys = M;
  L.nb = msm_div_up(M, MSM_SCAN_TILE);
  L.o_counts = (uintptr_t)counts - base;
  L.o_cursor = (uintptr_t)cursor - base;
  L.o_bsum = (uintptr_t)bsum - base;
  L.o_total = (uintptr_t)total - base;
  return mt_rc(bjjk::msm_scan((hipStream_t)stream, L, (uint8_t*)base));
}

// ---- 3. scatter ---------------------------------------------------------------------------------------------------------------
MT_EXPORT int mt_scatter(uint8_t* scratch, size_t scratch_bytes, size_t n, int c, void* stream) {
  MsmLayout L;
  if (!mt_make_layout(n, 1, c, 0, L) || !mt_block_ok(scratch, scratch_bytes, L)) return -1;
  BJJ_LAUNCH(bjj_k_msm_scatter, dim3(bjjk::blocks(n)), dim3(MSM_BLOCK), 0, (hipStream_t)stream, (const u32*)(scratch + L.o_red), n, L.c,
             (u64*)(scratch + L.o_cursor), (u64*)(scratch + L.o_rec));
  return mt_rc(hipGetLastError());
}
MT_EXPORT int mt_batch_scatter(uint8_t* scratch, size_t scratch_bytes, size_t n, size_t m, int c, void* stream) {
  MsmLayout L;
  if (!mt_make_layout(n, m, c, 0, L) || !mt_block_ok(scratch, scratch_bytes, L)) return -1;
  BJJ_LAUNCH(bjj_k_msm_batch_scatter, dim3(bjjk::blocks(n)), dim3(MSM_BLOCK), 0, (hipStream_t)stream, (const u32*)(scratch + L.o_red),
             (const u32*)(scratch + L.o_seg), n, L.c, (u64*)(scratch + L.o_cursor), (u64*)(scratch + L.o_rec));
  return mt_rc(hipGetLastError());
}

// ---- 4. + 5. slices, levels, window and group sums: returns 0 / 1 = the window sums are in w0 / w1 ----------------------------------
MT_EXPORT int mt_reduce(uint8_t* scratch, size_t scratch_bytes, size_t n, size_t m, int c, unsigned S1, void* stream) {
  MsmLayout L;
  if (!mt_make_layout(n, m, c, S1, L) || !mt_block_ok(scratch, scratch_bytes, L)) return -1;
  const uint32_t* wsum = nullptr;
  if (bjjk::msm_reduce((hipStream_t)stream, L, scratch, &wsum) != hipSuccess) return -3;
  if (wsum == (const uint32_t*)(scratch + L.o_w0)) return 0;
  return wsum == (const uint32_t*)(scratch + L.o_w1) ? 1 : -3;
}

// ---- 6. finish: `which` is what mt_reduce returned; the 64 result bytes per segment go to scratch + o_out ------------------------------
MT_EXPORT int mt_finish(uint8_t* scratch, size_t scratch_bytes, size_t n, int c, int which, void* stream) {
  MsmLayout L;
  if ((which != 0 && which != 1) || !mt_make_layout(n, 1, c, 0, L) || !mt_block_ok(scratch, scratch_bytes, L)) return -1;
  BJJ_LAUNCH(bjj_k_msm_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, (const u32*)(scratch + (which ? L.o_w1 : L.o_w0)), L.W, L.c,
             (const unsigned long long*)(scratch + L.o_status), scratch + L.o_out);
  return mt_rc(hipGetLastError());
}
MT_EXPORT int mt_batch_finish(uint8_t* scratch, size_t scratch_bytes, size_t n, size_t m, int c, int which, void* stream) {
  MsmLayout L;
  if ((which != 0 && which != 1) || !mt_make_layout(n, m, c, 0, L) || !mt_block_ok(scratch, scratch_bytes, L)) return -1;
  BJJ_LAUNCH(bjj_k_msm_batch_finish, dim3(bjjk::blocks(m, MSM_FINISH_BLOCK)), dim3(MSM_FINISH_BLOCK), 0, (hipStream_t)stream,
             (const u32*)(scratch + (which ? L.o_w1 : L.o_w0)), m, L.W, L.c, (unsigned long long*)(scratch + L.o_status),
             (const u32*)(scratch + L.o_flag), scratch + L.o_out);
  return mt_rc(hipGetLastError());
}

// ---- the counters: one call of wave_counter_add<T> per lane ----------------------------------------------------------------------
// lanes behind n, and lanes whose key does not name a counter, call with active = false (all 64 lanes of a wave must call)
template <typename T>
__global__ void __launch_bounds__(MSM_BLOCK) mt_counter_kernel(T* __restrict__ arr, u32 arr_len, const u32* __restrict__ key,
                                                              const uint8_t* __restrict__ active, T* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * MSM_BLOCK + threadIdx.x;
  u32 k = 0;
  bool on = false;
  if (i < n) { k = key[i]; on = active[i] != 0 && k < arr_len; }
  if (!on) k = 0;
  const T pos = wave_counter_add<T>(arr, k, on);
  if (i < n) out[i] = pos;
}
template <typename T>
static int mt_counter(T* arr, unsigned arr_len, const uint32_t* key, const uint8_t* active, T* out, size_t n, void* stream) {
  if (!arr || !key || !active || !out || arr_len < 1 || arr_len > (1u << 24) || n < 1 || n > MT_MAX_N) return -1;
  BJJ_LAUNCH(mt_counter_kernel<T>, dim3(bjjk::blocks(n)), dim3(MSM_BLOCK), 0, (hipStream_t)stream, arr, (u32)arr_len, key, active, out, n);
  return mt_rc(hipGetLastError());
}
MT_EXPORT int mt_counter_u32(uint32_t* arr, unsigned arr_len, const uint32_t* key, const uint8_t* active, uint32_t* out, size_t n, void* stream) {
  return mt_counter<u32>(arr, arr_len, key, active, out, n, stream);
}
MT_EXPORT int mt_counter_u64(uint64_t* arr, unsigned arr_len, const uint32_t* key, const uint8_t* active, uint64_t* out, size_t n, void* stream) {
  return mt_counter<u64>(arr, arr_len, key, active, out, n, stream);
}
