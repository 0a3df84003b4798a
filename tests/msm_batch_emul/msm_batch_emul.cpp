// DEBUG HARNESS (tests only): runs the batched bucket pipeline of bjj_msm_batch (csrc/msm.hpp, the bodies k_msm.hip and
// k_msm_batch.hip launch) on the CPU with limb / value-bound assertions, one "thread" after the other, as tests/msm_emul does
// for bjj_msm.  Every index the device code would form is checked against the size of its array.  Not linked into libbjj_hip.so.
#define BJJ_DEBUG_BOUNDS 1
#include <string.h>
#include <vector>
#include "../../babyjubjub-rs_amd/csrc/msm.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
#include "../emul_support.hpp"
#define EMUL_CHECK(cond) do { if (!(cond)) return -2; } while (0)   // an index the device would form lies outside its array

extern "C" {
// the segment the device assigns to item i (any offsets content)
unsigned msm_batch_emul_segment(const unsigned long long* offsets, size_t m, unsigned long long i) {
  return msm_find_segment((const u64*)offsets, m, i);
}
// The whole pipeline as the DEVICE form runs it: the offsets are data.  out: m * 64 bytes; status: m words (-1, the smallest
// off-curve index of the segment, or -2 everywhere for bad offsets).  Returns 0, -1 for bad arguments, -2 for an index out of range.
int msm_batch_emul_run(const uint8_t* pts, const uint8_t* scalars, size_t n, const unsigned long long* offsets_in, size_t m, int c,
                       uint8_t* out, long long* status_out) {
  if (c < MSM_MIN_C || c > MSM_MAX_C || m == 0) return -1;
  const int W = msm_windows(c);
  const u32 B = msm_buckets(c);
  const u64 nwin = (u64)m * W;
  if (nwin * B >= ((u64)1 << 31)) return -1;
  const size_t M = (size_t)(nwin * B);
  const u64* offsets = (const u64*)offsets_in;
  Aligned<uint8_t> in_pts(n * 64 + 1), in_sc(n * 32 + 1), res(m * 64);
  memcpy(in_pts.p(), pts, n * 64);
  memcpy(in_sc.p(), scalars, n * 32);
  Aligned<u32> niels(n * NIELS_WORDS + 1), red(n * 8 + 1);
  std::vector<u32> counts(M, 0), seg(n ? n : 1);
  std::vector<unsigned long long> st(m, ~0ull);
  // 0. offsets contract
  bool bad_offsets = false;
  for (size_t k = 0; k <= m; k++) bad_offsets = bad_offsets || !msm_offset_ok(offsets, m, n, k);
  // 1. prepare
  for (size_t i = 0; i < n; i++) {
    const u32 s = msm_find_segment(offsets, m, i);
    EMUL_CHECK(s < m);
    seg[i] = s;
    const bool on = msm_prepare_point(in_pts.p() + i * 64, niels.p() + i * NIELS_WORDS, K);
    if (!on && (unsigned long long)i < st[s]) st[s] = i;
    msm_prepare_scalar(in_sc.p() + i * 32, on, red.p() + i * 8, K);
    u32 carry = 0;
    for (int j = 0; j < W; j++) {
      const int d = msm_digit(red.p() + i * 8, j, c, carry);
      if (!d) continue;
      const u32 key = msm_batch_key(s, W, j, B, (u32)(d < 0 ? -d : d));
      EMUL_CHECK(key < M);
      counts[key]++;
    }
  }
  // 2. + 3. counting sort
  std::vector<u64> cursor(M);
  u64 T = 0;
  for (size_t k = 0; k < M; k++) { cursor[k] = T; T += counts[k]; }
  const u64 records = (u64)n * W;
  EMUL_CHECK(T <= records);
  std::vector<u64> rec(T ? T : 1);
  for (size_t i = 0; i < n; i++) {
    u32 carry = 0;
    for (int j = 0; j < W; j++) {
      const int d = msm_digit(red.p() + i * 8, j, c, carry);
      if (!d) continue;
      const u32 key = msm_batch_key(seg[i], W, j, B, (u32)(d < 0 ? -d : d));
      EMUL_CHECK(cursor[key] < T);
      rec[cursor[key]++] = msm_record(key, (u32)i, d < 0);
    }
  }
  for (u64 t = 1; t < T; t++) EMUL_CHECK(msm_record_key(rec[t - 1]) <= msm_record_key(rec[t]));
  // 4. slices: the records, then the levels of partials (the same schedule as the device)
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
  // 5. window sums over the m W "windows"
  const u32 G = B / MSM_SEG;
  std::vector<u32> w0((size_t)nwin * G * MSM_ENTRY_WORDS), w1((size_t)nwin * G * MSM_ENTRY_WORDS);
  for (u64 t = 0; t < nwin * G; t++) msm_store_ext(w0.data() + t * MSM_ENTRY_WORDS, msm_window_segment(buckets.data(), counts.data(), (int)(t / G), (u32)(t % G), c, K));
  std::vector<u32>* w[2] = {&w0, &w1};
  int cur = 0;
  for (u32 g = G; g > 1;) {
    const u32 F = g < (u32)MSM_GROUP ? g : (u32)MSM_GROUP;
    g /= F;
    for (u64 i = 0; i < nwin * g; i++) msm_store_ext(w[cur ^ 1]->data() + i * MSM_ENTRY_WORDS, msm_group_sum(w[cur]->data(), i, F, K));
    cur ^= 1;
  }
  // 6. finish, one "lane" per segment
  for (size_t s = 0; s < m; s++) msm_batch_finish(w[cur]->data(), s, n ? W : 0, c, st.data(), bad_offsets, res.p(), K);
  memcpy(out, res.p(), m * 64);
  for (size_t s = 0; s < m; s++) status_out[s] = (long long)st[s];
  return 0;
}
}
