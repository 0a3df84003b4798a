// DEBUG HARNESS (tests only): runs a whole call of bjj_point_sum_dev (csrc/point_sum.hpp, the bodies k_point_sum.hip launches) on
// the CPU with limb / value-bound assertions, one "lane" after the other and one barrier interval after the other, with the tile
// as a run-time parameter: a tile of 8 or 16 items crosses every boundary with a few hundred points.  Every index the device code
// would form is checked against the size of its array, and no result is written twice.  Not linked into libbjj_hip.so.
#define BJJ_DEBUG_BOUNDS 1
#include <string.h>
#include <vector>
#include "../../babyjubjub-rs_amd/csrc/point_sum.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
#include "../emul_support.hpp"
#define EMUL_CHECK(cond) do { if (!(cond)) return -2; } while (0)   // an index the device would form lies outside its array

struct Call {
  const uint8_t* pts; const uint8_t* neg; size_t n;
  const u64* offsets; size_t m;
  uint8_t* out; std::vector<unsigned long long>* st; std::vector<int>* written;
};

// One level: the tiles one after the other, every barrier interval of a tile for all its lanes before the next one.
// in == nullptr: the points; entries == nullptr: the last level.
static int run_level(const Call& c, const std::vector<u32>* in, u64 len, int T, std::vector<u32>* entries) {
  const u64 tiles = psum_tiles(len, (u32)T);
  for (u64 tile = 0; tile < tiles; tile++) {
    const u64 lo = tile * T, hi = lo + T < len ? lo + T : len;
    const int cnt = (int)(hi - lo);
    EMUL_CHECK(cnt >= 1 && cnt <= T);
    std::vector<u32> val((size_t)PSUM_EXT_WORDS * T, 0xdeadbeefu), seg(T, 0xdeadbeefu), live(T, 0xdeadbeefu);
    const PsumXch x{val.data(), seg.data(), live.data(), T};
    std::vector<PsumLane> a(cnt);
    for (int t = 0; t < cnt; t++) {
      if (!in) {
        EMUL_CHECK(lo + t < c.n);
        bool on = false;
        a[t] = psum_load_point(c.pts, c.neg, (size_t)(lo + t), c.offsets, c.m, &on, K);
        EMUL_CHECK(a[t].seg < c.m);
        if (!on && (unsigned long long)(lo + t) < (*c.st)[a[t].seg]) (*c.st)[a[t].seg] = lo + t;   // atomicMin
      } else {
        EMUL_CHECK((lo + t + 1) * MSM_ENTRY_WORDS <= in->size());
        a[t] = psum_load_entry(in->data(), (size_t)(lo + t));
        EMUL_CHECK(a[t].seg < c.m);
      }
      psum_xch_put(x, t, a[t]);
    }
    u32 before = PSUM_NO_SEG, after = PSUM_NO_SEG;
    if (entries) {
      EMUL_CHECK(in || hi <= c.n);
      EMUL_CHECK(!in || hi * MSM_ENTRY_WORDS <= in->size());
      before = in ? psum_entry_neighbour(in->data(), len, lo, hi, false) : psum_point_neighbour(c.offsets, c.m, len, lo, hi, false);
      after = in ? psum_entry_neighbour(in->data(), len, lo, hi, true) : psum_point_neighbour(c.offsets, c.m, len, lo, hi, true);
    }
    int adds = 0;
    for (int d = 1; d < cnt; d <<= 1) {
      std::vector<Ext> other(cnt);
      std::vector<char> take(cnt, 0);
      for (int t = 0; t < cnt; t++) take[t] = psum_scan_read(x, t, d, a[t], other[t]) ? 1 : 0;   // barrier
      for (int t = 0; t < cnt; t++) if (take[t]) psum_scan_write(x, t, a[t], other[t], K);        // barrier
      adds++;
    }
    EMUL_CHECK(adds <= 32);   // log2 of the tile: the bound on a lane's work per launch
    for (int t = 0; t < cnt; t++) {
      bool head_live = false, tail_live = false;
      const u32 what = psum_classify(x, t, cnt, a[t], before, after, &head_live, &tail_live);
      if (entries && what) {
        EMUL_CHECK((2 * tile + 2) * MSM_ENTRY_WORDS <= entries->size());
        psum_store_entries(entries->data(), tile, what, a[t], head_live, tail_live);
      }
      if (what & PSUM_WHOLE) {
        EMUL_CHECK(a[t].seg < c.m);
        EMUL_CHECK((*c.written)[a[t].seg]++ == 0);
        EMUL_CHECK(!fr_is_zero(a[t].v.Z));
        psum_store_result(c.out + (size_t)a[t].seg * 64, a[t].v, fr_inv(a[t].v.Z), K);   // the device: block_invert
      }
    }
  }
  return 0;
}

extern "C" {
// the segment the device assigns to item i (any offsets content)
unsigned point_sum_emul_segment(const unsigned long long* offsets, size_t m, unsigned long long i) {
  return msm_find_segment((const u64*)offsets, m, i);
}
int point_sum_emul_levels(unsigned long long n, int T) { return psum_level_count(n, (u32)T); }
// The whole call as the DEVICE form runs it: the offsets are data.  neg: n bytes or NULL.  T: the tile (>= 4).  out: m * 64 bytes;
// status: m words (-1, the smallest off-curve index of the segment, or -2 everywhere for bad offsets).  Returns 0, -1 for bad
// arguments, -2 for an index out of range or a result written twice.
int point_sum_emul_run(const uint8_t* pts, const uint8_t* neg, size_t n, const unsigned long long* offsets_in, size_t m, int T,
                       uint8_t* out, long long* status_out) {
  if (T < 4 || m == 0) return -1;
  const u64* offsets = (const u64*)offsets_in;
  Aligned<uint8_t> in_pts(n * 64 + 1), res(m * 64);
  if (n) memcpy(in_pts.p(), pts, n * 64);
  memset(res.p(), 0xAB, m * 64);
  std::vector<unsigned long long> st(m, ~0ull);
  std::vector<int> written(m, 0);
  bool bad_offsets = false;
  for (size_t k = 0; k <= m; k++) bad_offsets = bad_offsets || !msm_offset_ok(offsets, m, n, k);
  if (!bad_offsets && n) {   // the level kernels leave at once when the flag is set
    const Call c{in_pts.p(), neg, n, offsets, m, res.p(), &st, &written};
    const int levels = psum_level_count(n, (u32)T);
    const u64 tiles0 = psum_tiles(n, (u32)T), tiles1 = tiles0 > 1 ? psum_tiles(2 * tiles0, (u32)T) : 0;
    std::vector<u32> e0((size_t)(tiles0 > 1 ? 2 * tiles0 : 0) * MSM_ENTRY_WORDS, 0xdeadbeefu);
    std::vector<u32> e1((size_t)(tiles1 > 1 ? 2 * tiles1 : 0) * MSM_ENTRY_WORDS, 0xdeadbeefu);
    std::vector<u32>* e[2] = {&e0, &e1};
    u64 len = n;
    for (int l = 0; l < levels; l++) {
      const u64 tiles = psum_tiles(len, (u32)T);
      EMUL_CHECK((tiles == 1) == (l == levels - 1));
      const int rc = run_level(c, l ? e[(l - 1) & 1] : nullptr, len, T, tiles > 1 ? e[l & 1] : nullptr);
      if (rc) return rc;
      len = 2 * tiles;
    }
  }
  for (size_t s = 0; s < m; s++) {
    if (!bad_offsets) EMUL_CHECK(written[s] == (offsets[s] < offsets[s + 1] ? 1 : 0));   // every non-empty segment exactly once
    psum_finish(offsets, s, st.data(), bad_offsets, res.p());
  }
  memcpy(out, res.p(), m * 64);
  for (size_t s = 0; s < m; s++) status_out[s] = (long long)st[s];
  return 0;
}
}
