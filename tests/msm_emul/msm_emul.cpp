// DEBUG HARNESS (tests only): runs the bucket pipeline of bjj_msm (csrc/msm.hpp, the bodies k_msm.hip launches) on the CPU with
// limb / value-bound assertions, one "thread" after the other.  The counting sort -- wave-aggregated atomics and a three-pass scan
// on the device -- is restated here as the serial histogram / prefix / scatter it computes.  Not linked into libbjj_hip.so.
#define BJJ_DEBUG_BOUNDS 1
#include <string.h>
#include <vector>
#include "../../babyjubjub-rs_amd/csrc/msm.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
#include "../emul_support.hpp"

extern "C" {
// signed digits of one 32-byte scalar after the reduction mod 8l: W = ceil(255 / c) values into digits[]; returns W
int msm_emul_digits(const uint8_t* scalar32, int c, int* digits) {
  alignas(16) u32 w[8], k[8];
  memcpy(w, scalar32, 32);
  msm_reduce_scalar(w, k, K);
  u32 carry = 0;
  const int W = msm_windows(c);
  for (int j = 0; j < W; j++) digits[j] = msm_digit(k, j, c, carry);
  return W;
}
// the whole pipeline; out: 64 bytes; *status = -1 or the smallest index of an off-curve point
int msm_emul_run(const uint8_t* pts, const uint8_t* scalars, size_t n, int c, uint8_t* out, long long* status) {
  if (c < MSM_MIN_C || c > MSM_MAX_C) return -1;
  const int W = msm_windows(c);
  const u32 B = msm_buckets(c);
  const size_t M = (size_t)W * B;
  Aligned<uint8_t> in_pts(n * 64 + 1), in_sc(n * 32 + 1), res(64);
  memcpy(in_pts.p(), pts, n * 64);
  memcpy(in_sc.p(), scalars, n * 32);
  Aligned<u32> niels(n * NIELS_WORDS + 1), red(n * 8 + 1);
  std::vector<u32> counts(M, 0);
  long long st = -1;
  // 1. prepare
  for (size_t i = 0; i < n; i++) {
    const bool on = msm_prepare_point(in_pts.p() + i * 64, niels.p() + i * NIELS_WORDS, K);
    if (!on && st < 0) st = (long long)i;
    msm_prepare_scalar(in_sc.p() + i * 32, on, red.p() + i * 8, K);
    u32 carry = 0;
    for (int j = 0; j < W; j++) {
      const int d = msm_digit(red.p() + i * 8, j, c, carry);
      if (d) counts[(size_t)j * B + (d < 0 ? -d : d) - 1]++;
    }
  }
  // 2. + 3. counting sort
  std::vector<u64> cursor(M);
  u64 T = 0;
  for (size_t k = 0; k < M; k++) { cursor[k] = T; T += counts[k]; }
  std::vector<u64> rec(T ? T : 1);
  for (size_t i = 0; i < n; i++) {
    u32 carry = 0;
    for (int j = 0; j < W; j++) {
      const int d = msm_digit(red.p() + i * 8, j, c, carry);
      if (!d) continue;
      const u32 key = (u32)j * B + (d < 0 ? -d : d) - 1;
      rec[cursor[key]++] = msm_record(key, (u32)i, d < 0);
    }
  }
  // 4. slices: the records, then the levels of partials (the same schedule as the device)
  const u64 records = (u64)n * W;
  u32 S1 = 8;   // small inputs: exercise several levels on purpose
  if (records > 4096) S1 = 32;
  const u64 slices1 = msm_div_up(records ? records : 1, S1);
  const int levels = msm_level_count(records, S1);
  std::vector<u32> buckets(M * MSM_ENTRY_WORDS, 0xdeadbeefu);
  std::vector<u32> e0(2 * slices1 * MSM_ENTRY_WORDS), e1(2 * slices1 * MSM_ENTRY_WORDS);
  for (u64 s = 0; s < slices1; s++) msm_slice_records(rec.data(), T, s, S1, niels.p(), buckets.data(), e0.data(), K);
  u64 len = 2 * slices1;
  std::vector<u32>* e[2] = {&e0, &e1};
  for (int l = 0; l < levels; l++) {
    const u64 ns = msm_div_up(len, MSM_LEVEL_SLICE);
    for (u64 s = 0; s < ns; s++) msm_slice_entries(e[l & 1]->data(), len, s, MSM_LEVEL_SLICE, buckets.data(), e[(l + 1) & 1]->data(), K);
    len = 2 * ns;
  }
  // 5. window sums
  const u32 G = B / MSM_SEG;
  std::vector<u32> w0((size_t)W * G * MSM_ENTRY_WORDS), w1((size_t)W * G * MSM_ENTRY_WORDS);
  for (u64 t = 0; t < (u64)W * G; t++) msm_store_ext(w0.data() + t * MSM_ENTRY_WORDS, msm_window_segment(buckets.data(), counts.data(), (int)(t / G), (u32)(t % G), c, K));
  std::vector<u32>* w[2] = {&w0, &w1};
  int cur = 0;
  for (u32 g = G; g > 1;) {
    const u32 F = g < (u32)MSM_GROUP ? g : (u32)MSM_GROUP;
    g /= F;
    for (u64 i = 0; i < (u64)W * g; i++) msm_store_ext(w[cur ^ 1]->data() + i * MSM_ENTRY_WORDS, msm_group_sum(w[cur]->data(), i, F, K));
    cur ^= 1;
  }
  // 6. finish
  msm_finish(w[cur]->data(), n ? W : 0, c, st >= 0, res.p(), K);
  memcpy(out, res.p(), 64);
  *status = st;
  return 0;
}
}
