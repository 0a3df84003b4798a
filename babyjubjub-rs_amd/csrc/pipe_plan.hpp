// pipe_plan.hpp -- what a super-batch of the host-pointer pipeline (host_pipe.inc: run_pipelined) does before it touches the device:
// the chunk schedule, the lane parity, where every array lies in the device staging and in the pinned rings, and how many items
// fit into one super-batch.  Pure functions of plain values: no HIP, no getenv (the callers read the knobs, when they always did,
// and hand the strings or their values in).  Also built for the CPU under AddressSanitizer / UBSan by tests/test_pipe_plan.py
// (tests/emul/emul_pipe_plan.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <vector>

static inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// A knob that counts items (BJJ_PIPE_CHUNK, BJJ_PIPE_FIRST_CHUNK): 64 .. 2^24, rounded up to a multiple of 64; unset, empty or
// out of range = dflt
static inline size_t pipe_parse_items(const char* e, size_t dflt) {
  if (!e || !*e) return dflt;
  const unsigned long long v = strtoull(e, nullptr, 0);
  return v >= 64 && v <= ((size_t)1 << 24) ? ((size_t)v + 63) & ~(size_t)63 : dflt;
}
// developer: BJJ_PIPE_SCHEDULE="a,b,c,..." = the chunk sizes themselves (items, rounded DOWN to a multiple of 64, entries below 64
// dropped; the last one repeats, and what remains at the end is a short last chunk of its own).  Unset or empty = no override.
static inline std::vector<size_t> pipe_parse_schedule(const char* e) {
  std::vector<size_t> v;
  for (const char* p = e; p && *p;) {
    char* q = nullptr;
    const unsigned long long x = strtoull(p, &q, 0);
    if (q == p) break;
    if (x >= 64) v.push_back((size_t)x & ~(size_t)63);
    p = *q ? q + 1 : q;
  }
  return v;
}
// Items per super-batch: what fits into `budget` bytes of device staging at per_item bytes each, in whole pipe_chunks, at least one
static inline size_t pipe_super_batch_cap(size_t budget, size_t per_item, size_t pipe_chunk) {
  const size_t cap = budget / per_item;
  return cap > pipe_chunk ? cap / pipe_chunk * pipe_chunk : pipe_chunk;
}

struct PipePlanIn {
  size_t n;                                      // items of the super-batch
  int n_in, n_out;                               // PipeSpec: the arrays, their strides (n_in / n_out entries) ...
  const size_t *in_stride, *out_stride;
  const bool *in_direct, *out_direct;            // pinned arrays: copied from / to directly, no ring space
  size_t extra_dev_per_item;
  size_t first_chunk, max_chunk, tail_chunk;     // ... and the entry point's schedule (0 = the context's)
  bool last_on_priority_lane, out_at_end;
  size_t pipe_first, pipe_chunk;                 // the context's schedule
  bool pipe_env_schedule;                        // ... which came from the environment: the entry point's own is ignored
  const std::vector<size_t>* forced;             // BJJ_PIPE_SCHEDULE as parsed (null or empty = no override)
  int parity;                                    // BJJ_PIPE_LANE_PARITY: 0 / 1, -1 = no override
};
struct PipePlan {
  std::vector<size_t> lo_of;     // chunk ch = items lo_of[ch] .. lo_of[ch + 1]
  size_t lane_flip = 0;          // chunk ch runs on lane (ch + lane_flip) & 1; lane 1 = stream2
  size_t max_chunk = 0;
  // device staging: array i of the whole super-batch at d_*_off[i]; pinned ring slots: the staged arrays of ONE chunk
  size_t d_in_off[4] = {}, d_out_off[4] = {}, d_extra_off = 0, dev_tot = 0;
  size_t r_in_off[4] = {}, r_out_off[4] = {}, in_ring = 0, out_ring = 0;
  size_t nchunks() const { return lo_of.size() - 1; }
  size_t cnt_of(size_t ch) const { return lo_of[ch + 1] - lo_of[ch]; }
};

static inline PipePlan pipe_plan(const PipePlanIn& q) {
  PipePlan p;
  const size_t n = q.n;
  // ---- chunk schedule: first, 2 first, 4 first ... capped at pipe_chunk; a remainder below half a chunk joins the last chunk
  if (q.forced && !q.forced->empty()) {
    const std::vector<size_t>& f = *q.forced;
    for (size_t at = 0, k = 0; at < n; k++) { p.lo_of.push_back(at); at += f[k < f.size() ? k : f.size() - 1]; }
  } else {
    const size_t sz_max = (q.max_chunk && !q.pipe_env_schedule) ? q.max_chunk : q.pipe_chunk;
    size_t lo = 0, sz = (q.first_chunk && !q.pipe_env_schedule) ? q.first_chunk : q.pipe_first;
    if (sz > sz_max) sz = sz_max;
    // a separate small last chunk only when there is a schedule to speak of in front of it
    const size_t tail = (q.tail_chunk && !q.pipe_env_schedule && n >= 4 * q.tail_chunk) ? q.tail_chunk : 0;
    const size_t body_n = n - tail;
    while (lo < body_n) {
      size_t take = sz < body_n - lo ? sz : body_n - lo;
      if (body_n - lo - take < sz / 2) take = body_n - lo;          // what would be left is small: take it along
      p.lo_of.push_back(lo);
      lo += take;
      if (sz < sz_max) sz = sz * 2 < sz_max ? sz * 2 : sz_max;
    }
    if (tail) p.lo_of.push_back(body_n);
  }
  p.lo_of.push_back(n);
  const size_t nchunks = p.nchunks();
  p.lane_flip = q.parity >= 0 ? (size_t)q.parity : (q.last_on_priority_lane ? ((nchunks - 1) & 1) ^ 1 : 0);
  for (size_t ch = 0; ch < nchunks; ch++) if (p.cnt_of(ch) > p.max_chunk) p.max_chunk = p.cnt_of(ch);
  for (int i = 0; i < q.n_in; i++) { p.d_in_off[i] = p.dev_tot; p.dev_tot += up256(n * q.in_stride[i]); }
  for (int i = 0; i < q.n_out; i++) { p.d_out_off[i] = p.dev_tot; p.dev_tot += up256(n * q.out_stride[i]); }
  p.d_extra_off = p.dev_tot;
  p.dev_tot += up256(n * q.extra_dev_per_item);
  for (int i = 0; i < q.n_in; i++) if (!q.in_direct[i]) { p.r_in_off[i] = p.in_ring; p.in_ring += up16(p.max_chunk * q.in_stride[i]); }
  // outputs that leave at the end go through ONE ring slot that holds the whole array
  for (int i = 0; i < q.n_out; i++) if (!q.out_direct[i]) { p.r_out_off[i] = p.out_ring; p.out_ring += up16((q.out_at_end ? n : p.max_chunk) * q.out_stride[i]); }
  return p;
}
