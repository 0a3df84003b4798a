// Variable-base multi-scalar multiplication Q = sum k_i * P_i (bjj_msm, k_msm.hip): the per-thread bodies of Pippenger's bucket
// method.  __host__ __device__ like bjj_device.hpp, so that tests/msm_emul runs exactly this code on the CPU with bound assertions.
//
// Reference semantics: k_i * P_i is Point::mul_scalar (src/lib.rs:149-164), the sum PointProjective::add (src/lib.rs:88-131) folded
// from (0, 1, 1), then .affine() (src/lib.rs:70-85).  For on-curve points the addition law is complete (A a square, D a non-square),
// the group has order 8l and canonical affine coordinates are unique: ANY correct evaluation order gives the reference's bytes.
// The device works on the a' = -1 curve (curve.hpp) in extended coordinates.
//
// Pipeline (one kernel per step, k_msm.hip; W = ceil(255 / c) windows, B = 2^(c-1) buckets per window, M = W * B keys):
//   1. prepare   per item: on-curve check (a failing index -> atomicMin on the status word), affine-Niels point at a 128-B stride,
//                scalar mod 8l, signed c-bit digits, histogram of key = j * B + |d| - 1
//   2. scan      exclusive prefix of the histogram -> per-key offsets and cursors
//   3. scatter   records (key << 33 | item << 1 | sign) into key order
//   4. slices    segmented reduction over FIXED-SIZE slices of the sorted records (mixed additions): a key that starts and ends
//                inside a slice is written to its bucket; a key cut by a slice boundary leaves a partial (head / tail entry of
//                the slice).  The partials are reduced the same way, slice after slice, until one slice holds them all.  No lane
//                ever owns a whole bucket, so "every digit in one bucket" costs what a random input costs plus a few levels.
//   5. windows   per window, segments of MSM_SEG buckets: running sums give A_g = sum (b - g L) B_b and R_g = sum B_b; the
//                segment's share of sum b * B_b is A_g + (g L) R_g (a small scalar multiplication); then group sums per window
//   6. finish    Horner over the windows (c doublings each), one inversion, reference coordinates, canonical bytes; (0, 0) when
//                the status word names an off-curve point
#pragma once
#include "bjj_device.hpp"

namespace bjj {

constexpr int MSM_MIN_C = 4, MSM_MAX_C = 20;
constexpr int MSM_ENTRY_WORDS = 40;           // Ext limbs (36 words) + key + live flag, 160 B
constexpr u32 MSM_NO_KEY = 0xffffffffu;       // past the last record: sorts behind every real key, never live
constexpr int MSM_SEG = 8;                    // buckets per segment of the window sums (B >= 8 for c >= 4)
constexpr int MSM_LEVEL_SLICE = 8;            // entries per slice of the partial-reduction levels
constexpr int MSM_GROUP = 8;                  // values per group of the window group sums

BJJ_HD int msm_windows(int c) { return (255 + c - 1) / c; }
BJJ_HD u32 msm_buckets(int c) { return 1u << (c - 1); }

// ---- scalars -------------------------------------------------------------------------------------------------------------
// k mod 8l (< 2^254) of a 256-bit scalar: exact for an on-curve point (the group order is 8l).
BJJ_HD void msm_reduce_scalar(const u32 w[8], u32 out[8], const Consts& K) { scalar_mod_order(w, out, K); }
// Signed digit j (call j = 0 .. W-1 in order; carry starts at 0): d in [-2^(c-1), 2^(c-1)], sum d_j 2^(c j) == k exactly,
// because k < 2^254 leaves the top window at most 2^(c-1) when c W >= 255: no carry out of the last window.
BJJ_HD int msm_digit(const u32 k[8], int j, int c, u32& carry) {
  const u32 v = scalar_window(k, j, c) + carry;
  if (v > (1u << (c - 1))) { carry = 1; return (int)v - (int)(1u << c); }
  carry = 0;
  return (int)v;
}
BJJ_HD u64 msm_record(u32 key, u32 item, bool neg) { return ((u64)key << 33) | ((u64)item << 1) | (neg ? 1u : 0u); }
BJJ_HD u32 msm_record_key(u64 r) { return (u32)(r >> 33); }

// ---- points --------------------------------------------------------------------------------------------------------------
// (x, y) records -> affine Niels entry of (F x, y) on the a' = -1 curve (128 B); returns whether the point is on the curve.
// An off-curve point's entry is never read: its scalar is replaced by 0 (no digits, no records).
BJJ_HD bool msm_prepare_point(const uint8_t* xy, u32* niels, const Consts& K) {
  u32 w[8];
  load_w8(xy, w);      const Fr x = fr_to_mont_words(w);
  load_w8(xy + 32, w); const Fr y = fr_to_mont_words(w);
  const bool on = ref_on_curve(x, y, K);
  store_niels(niels, niels_from_affine(fr_mul(x, K.F), y, K, false));
  return on;
}
// the reduced scalar the later passes recode (zero for an off-curve point)
BJJ_HD void msm_prepare_scalar(const uint8_t* sc, bool on, u32 red[8], const Consts& K) {
  u32 w[8];
  load_w8(sc, w);
  msm_reduce_scalar(w, red, K);
  if (!on)
    for (int i = 0; i < 8; i++) red[i] = 0;
}

// ---- extended points in memory (raw limbs) and the general addition --------------------------------------------------------
BJJ_HD void msm_store_ext(u32* p, const Ext& e) {
  for (int i = 0; i < NL; i++) { p[i] = e.X.v[i]; p[NL + i] = e.Y.v[i]; p[2 * NL + i] = e.Z.v[i]; p[3 * NL + i] = e.T.v[i]; }
}
BJJ_HD Ext msm_load_ext(const u32* p) {
  Ext e;
  for (int i = 0; i < NL; i++) { e.X.v[i] = p[i]; e.Y.v[i] = p[NL + i]; e.Z.v[i] = p[2 * NL + i]; e.T.v[i] = p[3 * NL + i]; }
  return e;
}
BJJ_HD Ext msm_add(const Ext& a, const Ext& b, const Consts& K) { return ext_add_pn(a, ext_to_pniels(b, K), true); }
BJJ_HD void msm_store_entry(u32* e, u32 key, bool live, const Ext& v) {
  if (live) msm_store_ext(e, v);
  e[36] = key;
  e[37] = live ? 1u : 0u;
}

// ---- 4. segmented reduction over fixed-size slices -------------------------------------------------------------------------
// One segment = the run of one key inside a slice.  started: the key does not continue from before the slice; ended: it does
// not continue past it.  Complete (both) -> its bucket; else the slice's head (first segment, or a segment spanning the whole
// slice) or tail entry.  Entries that do not carry a partial keep their key with live = 0 (value = identity, not stored), so
// the entry list stays sorted and the next level never writes a key twice: a key is written exactly once, by the level at which
// its segment is complete and holds a live value.
struct MsmSeg {
  u32* buckets;
  u32* head;
  u32* tail;
  BJJ_HD void flush(u32 key, const Ext& acc, bool live, bool started, bool ended) const {
    if (!live) return;
    if (started && ended) msm_store_ext(buckets + (size_t)key * MSM_ENTRY_WORDS, acc);
    else msm_store_entry(started ? tail : head, key, true, acc);
  }
};
// level 1: records rec[lo, hi) of the T sorted records; slice s writes its head / tail entries to out + 2 s entries
BJJ_HD void msm_slice_records(const u64* rec, u64 T, u64 s, u32 S, const u32* niels, u32* buckets, u32* out, const Consts& K) {
  u32* head = out + (size_t)(2 * s) * MSM_ENTRY_WORDS;
  u32* tail = head + MSM_ENTRY_WORDS;
  const u64 lo = s * S;
  if (lo >= T) { head[36] = tail[36] = MSM_NO_KEY; head[37] = tail[37] = 0u; return; }
  const u64 hi = lo + S < T ? lo + S : T;
  const u32 before = lo > 0 ? msm_record_key(rec[lo - 1]) : MSM_NO_KEY;
  const u32 after = hi < T ? msm_record_key(rec[hi]) : MSM_NO_KEY;
  head[36] = msm_record_key(rec[lo]); head[37] = 0u;
  tail[36] = msm_record_key(rec[hi - 1]); tail[37] = 0u;
  const MsmSeg seg{buckets, head, tail};
  u32 cur = msm_record_key(rec[lo]);
  bool first = true;
  Ext acc = ext_identity();
#pragma unroll 1
  for (u64 i = lo; i < hi; i++) {
    const u64 r = rec[i];
    const u32 key = msm_record_key(r);
    if (key != cur) {
      seg.flush(cur, acc, true, !(first && cur == before), true);
      first = false; cur = key; acc = ext_identity();
    }
    const u32 item = (u32)(r >> 1) & 0xffffffffu;
    acc = ext_madd(acc, niels_cneg_lazy(load_niels(niels + (size_t)item * NIELS_WORDS), (r & 1u) != 0));
  }
  seg.flush(cur, acc, true, !(first && cur == before), cur != after);
}
// levels 2, 3, ...: entries in[lo, hi) of len, same rules (the last level is one slice: every segment is complete there)
BJJ_HD void msm_slice_entries(const u32* in, u64 len, u64 s, u32 S, u32* buckets, u32* out, const Consts& K) {
  u32* head = out + (size_t)(2 * s) * MSM_ENTRY_WORDS;
  u32* tail = head + MSM_ENTRY_WORDS;
  const u64 lo = s * S;
  if (lo >= len) { head[36] = tail[36] = MSM_NO_KEY; head[37] = tail[37] = 0u; return; }
  const u64 hi = lo + S < len ? lo + S : len;
  const u32 before = lo > 0 ? in[(size_t)(lo - 1) * MSM_ENTRY_WORDS + 36] : MSM_NO_KEY;
  const u32 after = hi < len ? in[(size_t)hi * MSM_ENTRY_WORDS + 36] : MSM_NO_KEY;
  head[36] = in[(size_t)lo * MSM_ENTRY_WORDS + 36]; head[37] = 0u;
  tail[36] = in[(size_t)(hi - 1) * MSM_ENTRY_WORDS + 36]; tail[37] = 0u;
  const MsmSeg seg{buckets, head, tail};
  u32 cur = head[36];
  bool first = true, live = false;
  Ext acc = ext_identity();
#pragma unroll 1
  for (u64 i = lo; i < hi; i++) {
    const u32* e = in + (size_t)i * MSM_ENTRY_WORDS;
    const u32 key = e[36];
    if (key != cur) {
      seg.flush(cur, acc, live, !(first && cur == before), true);
      first = false; cur = key; acc = ext_identity(); live = false;
    }
    if (e[37]) {
      acc = live ? msm_add(acc, msm_load_ext(e), K) : msm_load_ext(e);
      live = true;
    }
  }
  seg.flush(cur, acc, live, !(first && cur == before), cur != after);
}
// Level schedule: slice sizes and list lengths are bounds fixed by n and c (the host launches every level; slices past the
// actual data emit MSM_NO_KEY entries).  Returns the number of levels after the record level; len[l] = entries of level l + 1.
BJJ_HD u64 msm_div_up(u64 a, u64 b) { return (a + b - 1) / b; }
BJJ_HD int msm_level_count(u64 records, u32 S1) {
  u64 slices = msm_div_up(records ? records : 1, S1);
  int levels = 0;
  while (slices > 1) {
    const u64 len = 2 * slices;
    slices = msm_div_up(len, MSM_LEVEL_SLICE);
    levels++;
  }
  return levels;
}

// ---- 5. buckets -> window sums ----------------------------------------------------------------------------------------------
// Segment g of window j: buckets b = g L + 1 .. (g + 1) L.  Returns A_g + (g L) R_g; summed over g this is sum_b b * B_b.
// counts[key] == 0: the bucket was never written (identity).
BJJ_HD Ext msm_window_segment(const u32* buckets, const u32* counts, int j, u32 g, int c, const Consts& K) {
  const u32 B = msm_buckets(c);
  Ext run = ext_identity(), sum = ext_identity();
#pragma unroll 1
  for (u32 b = (g + 1) * MSM_SEG; b > g * MSM_SEG; b--) {
    const size_t key = (size_t)j * B + (b - 1);
    if (counts[key]) run = msm_add(run, msm_load_ext(buckets + key * MSM_ENTRY_WORDS), K);
    sum = msm_add(sum, run, K);
  }
  // (g L) * run, MSB first over the c - 1 bits of a value < B (select, not branch: the lanes of a wave hold different g)
  const u32 m = g * MSM_SEG;
  const PNiels rp = ext_to_pniels(run, K);
  Ext acc = ext_identity();
#pragma unroll 1
  for (int bit = c - 2; bit >= 0; bit--) {
    acc = ext_dbl<true>(acc);
    const Ext t = ext_add_pn(acc, rp, true);
    const bool on = (m >> bit) & 1u;
    acc.X = fr_select(on, t.X, acc.X); acc.Y = fr_select(on, t.Y, acc.Y);
    acc.Z = fr_select(on, t.Z, acc.Z); acc.T = fr_select(on, t.T, acc.T);
  }
  return msm_add(sum, acc, K);
}
// out[i] = in[i F] + ... + in[i F + F - 1]
BJJ_HD Ext msm_group_sum(const u32* in, u64 i, u32 F, const Consts& K) {
  Ext acc = msm_load_ext(in + (size_t)(i * F) * MSM_ENTRY_WORDS);
#pragma unroll 1
  for (u32 f = 1; f < F; f++) acc = msm_add(acc, msm_load_ext(in + (size_t)(i * F + f) * MSM_ENTRY_WORDS), K);
  return acc;
}

// ---- 6. windows -> Q ----------------------------------------------------------------------------------------------------------
// wsum: the W window sums (entry stride).  out: 64 bytes, reference (x, y) canonical; (0, 0) when `bad`.  W = 0: identity (0, 1).
BJJ_HD void msm_finish(const u32* wsum, int W, int c, bool bad, uint8_t* out, const Consts& K) {
  Ext acc = W > 0 ? msm_load_ext(wsum + (size_t)(W - 1) * MSM_ENTRY_WORDS) : ext_identity();
#pragma unroll 1
  for (int j = W - 2; j >= 0; j--) {
#pragma unroll 1
    for (int t = 1; t < c; t++) acc = ext_dbl<false>(acc);   // a doubling does not read T: only the last one before the addition needs it
    acc = ext_dbl<true>(acc);
    acc = msm_add(acc, msm_load_ext(wsum + (size_t)j * MSM_ENTRY_WORDS), K);
  }
  const Fr zi = fr_inv(acc.Z);                       // Z != 0: the law is complete on the curve
  u32 w[8];
  fr_from_mont_words(fr_mul(fr_mul(acc.X, zi), K.FINV), w);   // x = x' / F
  if (bad) for (int i = 0; i < 8; i++) w[i] = 0;
  store_w8(out, w);
  fr_from_mont_words(fr_mul(acc.Y, zi), w);
  if (bad) for (int i = 0; i < 8; i++) w[i] = 0;
  store_w8(out + 32, w);
}

// ---- batched form (bjj_msm_batch, k_msm_batch.hip): m independent sums over CSR segments of one point / scalar array ----------
// Segment s = items [offsets[s], offsets[s + 1]).  The sort key carries the segment: key = (s W + j) B + |d| - 1 < m W B, so the
// scan, the slices, the levels, the window sums and the group sums above run unchanged with "window" s W + j; only the two
// passes that form keys and the finish know about segments.
// The segment of item i: the last s in [0, m - 1] with offsets[s] <= i (m >= 1).  For valid offsets that is the s with
// offsets[s] <= i < offsets[s + 1]; for ANY content of offsets[] the loop reads only offsets[1 .. m - 1] and returns a value in
// [0, m - 1].  Neighbouring items probe the same words (one line per step and wave almost everywhere).
BJJ_HD u32 msm_find_segment(const u64* offsets, size_t m, u64 i) {
  size_t lo = 0, hi = m;
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (offsets[mid] <= i) lo = mid; else hi = mid;
  }
  return (u32)lo;
}
BJJ_HD u32 msm_batch_key(u32 s, int W, int j, u32 B, u32 b) { return (s * (u32)W + (u32)j) * B + b - 1u; }
// condition k (k = 0 .. m) of the offsets contract: offsets[0] == 0, non-decreasing, offsets[m] == n
BJJ_HD bool msm_offset_ok(const u64* offsets, size_t m, u64 n, size_t k) {
  bool ok = true;
  if (k == 0) ok = ok && offsets[0] == 0;
  if (k == m) ok = ok && offsets[m] == n;
  if (k < m) ok = ok && offsets[k] <= offsets[k + 1];
  return ok;
}
// Segment s of the batch: Horner over its W window sums.  status: the segment's word (-1, or the smallest off-curve index of the
// whole array inside the segment); offsets_bad: the offsets contract is broken -> every result (0, 0), every status word -2.
BJJ_HD void msm_batch_finish(const u32* wsum, size_t s, int W, int c, unsigned long long* status, bool offsets_bad, uint8_t* out,
                             const Consts& K) {
  if (offsets_bad) {
    const u32 z[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    store_w8(out + s * 64, z);
    store_w8(out + s * 64 + 32, z);
    status[s] = ~1ull;   // -2
    return;
  }
  msm_finish(wsum + s * (size_t)W * MSM_ENTRY_WORDS, W, c, status[s] != ~0ull, out + s * 64, K);
}

}  // namespace bjj
