// Signed point sums over CSR segments (bjj_point_sum, k_point_sum.hip): Q_s = sum_{i in [offsets[s], offsets[s + 1])} +-P_i.  The
// per-lane bodies of a segmented reduction whose element is an extended point; __host__ __device__ like msm.hpp, so that
// tests/point_sum_emul runs exactly this code on the CPU with bound assertions.
//
// Reference semantics: the fold of PointProjective::add (src/lib.rs:88-131) from (0, 1, 1) over +-P_i, -(x, y) = (-x, y), then
// .affine() (src/lib.rs:70-85).  The addition law is complete on the curve and canonical affine coordinates are unique, so ANY
// association order gives the reference's bytes -- which are also bjj_msm_batch's for the scalars 1 and 8l - 1.
//
// One launch per level (k_point_sum.hip).  A workgroup of PSUM_TILE lanes takes PSUM_TILE consecutive items, ONE per lane:
//   level 0     items are the caller's 64-byte records: on-curve check (a failing index -> atomicMin on the segment's status word,
//               the point is replaced by the identity), conditional negation, the segment number by msm_find_segment
//   level >= 1  items are the entries the level before left: two per tile (head, tail), projective, with their segment numbers
//   scan        inclusive segmented scan over the tile through an exchange area of 144 B per lane (log2 PSUM_TILE steps, one
//               general addition each for the lanes that have a live partner in their own segment)
//   results     the last lane of every run holds the run's sum.  A run that neither continues from before the tile nor past it
//               is a whole segment: its Z goes through the workgroup-wide simultaneous inversion (every other lane feeds 1) and
//               its canonical bytes to out[s].  The run at the head of the tile, when it continues from before, and the run at its
//               tail, when it continues, leave a live entry for the next level; entries that carry nothing keep their segment
//               number with live = 0, so the entry list stays sorted and no segment is written twice.
// The levels end with the one that fits a single tile: every run is whole there.  No lane performs more than log2 PSUM_TILE
// additions per launch whatever the offsets; the levels number about log(n) / log(PSUM_TILE / 2).
// A last pass over the segments (psum_finish) writes what no run owns: (0, 1) for an empty segment, (0, 0) for a spoiled one, and
// for offsets that break their contract (0, 0) and status -2 everywhere -- the levels do not run at all then.
#pragma once
#include "msm.hpp"

#define PSUM_TILE 256   // points per workgroup and pass == lanes per workgroup

namespace bjj {

constexpr u32 PSUM_NO_SEG = 0xffffffffu;   // beyond either end of the item list: no segment has this number (s <= m - 1 < 2^32 - 1)
constexpr int PSUM_EXT_WORDS = 4 * NL;     // one extended point of the exchange area

struct PsumLane { Ext v; u32 seg; bool live; };   // live = 0: v is not meaningful (stands for the identity)

// ---- items -------------------------------------------------------------------------------------------------------------------
// level 0: point i of the caller's array.  *on: the point is on the curve (else the lane carries the identity and the caller
// reports i to the status word of the lane's segment).  neg == nullptr: every term is added.
BJJ_HD PsumLane psum_load_point(const uint8_t* pts, const uint8_t* neg, size_t i, const u64* offsets, size_t m, bool* on, const Consts& K) {
  PsumLane a;
  a.seg = msm_find_segment(offsets, m, (u64)i);   // in [0, m - 1] whatever offsets[] holds
  a.live = true;
  u32 w[8];
  load_w8(pts + i * 64, w);      const Fr x = fr_to_mont_words(w);
  load_w8(pts + i * 64 + 32, w); const Fr y = fr_to_mont_words(w);
  *on = ref_on_curve(x, y, K);   // the test of msm_prepare_point, on the same values
  const bool minus = neg != nullptr && neg[i] != 0;
  a.v = ext_from_ref_affine(fr_select(minus, fr_neg(x), x), y, K);
  if (!*on) a.v = ext_identity();
  return a;
}
// level >= 1: entry i of the list the level before wrote
BJJ_HD PsumLane psum_load_entry(const u32* in, size_t i) {
  const u32* e = in + i * MSM_ENTRY_WORDS;
  PsumLane a;
  a.seg = e[36];
  a.live = e[37] != 0u;
  a.v = a.live ? msm_load_ext(e) : ext_identity();
  return a;
}
// the segments of the items next to the tile [lo, hi) of a list of len items
BJJ_HD u32 psum_point_neighbour(const u64* offsets, size_t m, u64 len, u64 lo, u64 hi, bool after) {
  if (after) return hi < len ? msm_find_segment(offsets, m, hi) : PSUM_NO_SEG;
  return lo > 0 ? msm_find_segment(offsets, m, lo - 1) : PSUM_NO_SEG;
}
BJJ_HD u32 psum_entry_neighbour(const u32* in, u64 len, u64 lo, u64 hi, bool after) {
  if (after) return hi < len ? in[(size_t)hi * MSM_ENTRY_WORDS + 36] : PSUM_NO_SEG;
  return lo > 0 ? in[(size_t)(lo - 1) * MSM_ENTRY_WORDS + 36] : PSUM_NO_SEG;
}

// ---- the exchange area of a tile: T lanes, limb-major (word k of lane t at val[k T + t]: neighbouring lanes, neighbouring banks) --
struct PsumXch {
  u32* val;    // PSUM_EXT_WORDS * T
  u32* seg;    // T
  u32* live;   // T
  int T;
};
BJJ_HD void psum_xch_put_value(const PsumXch& x, int t, const PsumLane& a) {
  for (int k = 0; k < NL; k++) {
    x.val[(0 * NL + k) * x.T + t] = a.v.X.v[k]; x.val[(1 * NL + k) * x.T + t] = a.v.Y.v[k];
    x.val[(2 * NL + k) * x.T + t] = a.v.Z.v[k]; x.val[(3 * NL + k) * x.T + t] = a.v.T.v[k];
  }
  x.live[t] = a.live ? 1u : 0u;
}
BJJ_HD void psum_xch_put(const PsumXch& x, int t, const PsumLane& a) {
  x.seg[t] = a.seg;
  psum_xch_put_value(x, t, a);
}
BJJ_HD Ext psum_xch_get(const PsumXch& x, int t) {
  Ext e;
  for (int k = 0; k < NL; k++) {
    e.X.v[k] = x.val[(0 * NL + k) * x.T + t]; e.Y.v[k] = x.val[(1 * NL + k) * x.T + t];
    e.Z.v[k] = x.val[(2 * NL + k) * x.T + t]; e.T.v[k] = x.val[(3 * NL + k) * x.T + t];
  }
  return e;
}
// Step d = 1, 2, 4, ... of the scan, lane t of cnt, in two halves with a barrier between them and one after: the read half takes
// the sum that ends d lanes before, when that lane lies in the same run and carries anything; the write half publishes the
// lane's new sum.  Before the step lane t holds the sum over the last min(d, position in run + 1) items up to its own.
BJJ_HD bool psum_scan_read(const PsumXch& x, int t, int d, const PsumLane& a, Ext& other) {
  if (t < d || x.seg[t - d] != a.seg || x.live[t - d] == 0u) return false;
  other = psum_xch_get(x, t - d);
  return true;
}
BJJ_HD void psum_scan_write(const PsumXch& x, int t, PsumLane& a, const Ext& other, const Consts& K) {
  a.v = a.live ? msm_add(other, a.v, K) : other;
  a.live = true;
  psum_xch_put_value(x, t, a);
}

// ---- what the lane's sum is, after the scan --------------------------------------------------------------------------------------
enum : u32 { PSUM_WHOLE = 1u, PSUM_HEAD = 2u, PSUM_TAIL = 4u };
// PSUM_WHOLE: the lane ends a run that is a whole segment and carries a value -> the result of segment a.seg.
// PSUM_HEAD:  the lane ends the first run of the tile -> it writes the tile's head entry (live when the run continues from before).
// PSUM_TAIL:  the lane is the last of the tile -> it writes the tile's tail entry (live when its run started here and continues).
// before / after: the segments of the items next to the tile (PSUM_NO_SEG at the ends of the list, and at the last level).
BJJ_HD u32 psum_classify(const PsumXch& x, int t, int cnt, const PsumLane& a, u32 before, u32 after, bool* head_live, bool* tail_live) {
  *head_live = *tail_live = false;
  const bool last = t == cnt - 1;
  if (!last && x.seg[t + 1] == a.seg) return 0u;
  const bool first_run = x.seg[0] == a.seg;
  const bool started = !(first_run && before == a.seg);
  const bool ended = !(last && after == a.seg);
  u32 r = 0u;
  if (started && ended && a.live) r |= PSUM_WHOLE;
  if (first_run) { r |= PSUM_HEAD; *head_live = !started && a.live; }
  if (last) { r |= PSUM_TAIL; *tail_live = started && !ended && a.live; }
  return r;
}
BJJ_HD void psum_store_entries(u32* out, u64 tile, u32 what, const PsumLane& a, bool head_live, bool tail_live) {
  u32* head = out + (size_t)(2 * tile) * MSM_ENTRY_WORDS;
  if (what & PSUM_HEAD) msm_store_entry(head, a.seg, head_live, a.v);
  if (what & PSUM_TAIL) msm_store_entry(head + MSM_ENTRY_WORDS, a.seg, tail_live, a.v);
}
// reference coordinates, canonical bytes: msm_finish's last lines with the inverse handed in (zi = 1 / Z, Montgomery)
BJJ_HD void psum_store_result(uint8_t* out, const Ext& v, const Fr& zi, const Consts& K) {
  u32 w[8];
  fr_from_mont_words(fr_mul(fr_mul(v.X, zi), K.FINV), w);   // x = x' / F
  store_w8(out, w);
  fr_from_mont_words(fr_mul(v.Y, zi), w);
  store_w8(out + 32, w);
}

// ---- the schedule: items per level (the host launches every level; every tile of every level holds at least one item) -------------
BJJ_HD u64 psum_tiles(u64 items, u32 T) { return (items + T - 1) / T; }
BJJ_HD int psum_level_count(u64 n, u32 T) {   // launches for n >= 1 points
  int levels = 1;
  for (u64 tiles = psum_tiles(n, T); tiles > 1; tiles = psum_tiles(2 * tiles, T)) levels++;
  return levels;
}

// ---- the segments nobody's run owns --------------------------------------------------------------------------------------------
// status: the segment's word (~0, or the smallest off-curve index the level-0 lanes left).  offsets_bad: every result (0, 0), every
// status word -2.  Reads offsets[s] and offsets[s + 1] only.
BJJ_HD void psum_finish(const u64* offsets, size_t s, unsigned long long* status, bool offsets_bad, uint8_t* out) {
  u32 z[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (offsets_bad) {
    store_w8(out + s * 64, z);
    store_w8(out + s * 64 + 32, z);
    status[s] = ~1ull;   // -2
    return;
  }
  if (offsets[s] == offsets[s + 1]) {   // empty: the identity (0, 1)
    store_w8(out + s * 64, z);
    z[0] = 1u;
    store_w8(out + s * 64 + 32, z);
  } else if (status[s] != ~0ull) {
    store_w8(out + s * 64, z);
    store_w8(out + s * 64 + 32, z);
  }
}

}  // namespace bjj
