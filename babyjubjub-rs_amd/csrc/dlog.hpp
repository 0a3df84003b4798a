// Batched small-range discrete logarithms, m from P = m * G with 0 <= m < 2^range_bits (include/bjj_hip_dlog.h): the per-lane
// bodies of the build, check and search kernels of k_dlog.hip.  __host__ __device__ like bases.hpp, so that tests/dlog_emul runs
// exactly this code on the CPU.
//
// Baby steps.  An open-addressed table of 2^(b+2) slots of 8 bytes holds j * G for j = 0 .. 2^b (b = baby_bits): 2^b + 1 entries,
// a quarter full.  The key is the canonical y of j * G as a 256-bit integer (dlog_canon_y): slot index = its low b + 2 bits (word 0),
// tag = word 1 -- disjoint bits -- and the slot is {tag, j + 1}, 0 = empty, linear probing.  -(x, y) = (-x, y) on this curve, so y alone
// identifies +-j * G: one lookup answers for the 2^(b+1) + 1 values -2^b .. 2^b, and the sign is found by comparing x when the hit
// is confirmed.  Two different j in 0 .. 2^b never share y: G has order >= l > 2^250 (dlog_setup refuses 8 G = identity).
// Giant steps.  Q_i = P - (2^b + i * 2^(b+1)) * G for i = 0, 1, ...: window i answers for m in [i * 2^(b+1), (i + 1) * 2^(b+1)].
// Q_0 is one mixed addition of -2^b G, every further Q one of -2^(b+1) G (7 multiplications); the y of a step needs 1 / Z, which
// the kernel takes from a workgroup-wide simultaneous inversion and the CPU program from fr_inv.
// Confirmation.  A tag hit is a candidate only.  The lane keeps Q_i and waits; when no lane of the workgroup searches any more,
// every waiting lane recomputes j * G by double-and-add and compares it with its Q_i in full-width x and y, projectively.  Equal:
// m = c_i + j; equal with x negated: m = c_i - j; neither: the lane goes on probing behind the false hit.  No m is reported
// without this comparison.
#pragma once
#include "bjj_device.hpp"

#define BJJ_DLOG_GIANT_BITS 16          // BJJ_DLOG_MAX_GIANT_BITS of include/bjj_hip_dlog.h
#define BJJ_DLOG_MIN_BABY_BITS 4
#define BJJ_DLOG_MAX_BABY_BITS 28

namespace bjj {

// what dlog_setup leaves for the kernels, in words from the start of the block (each Niels entry NIELS_WORDS words)
constexpr int DLOG_P_G = 0;             // Niels(G)
constexpr int DLOG_P_NEG_HALF = 32;     // Niels(-2^b G): P -> Q_0
constexpr int DLOG_P_NEG_STRIDE = 64;   // Niels(-2^(b+1) G): Q_i -> Q_(i+1)
constexpr int DLOG_P_XY = 96;           // x, y of G, canonical, 2 x 8 words
constexpr int DLOG_P_SMALL = 112;       // 1 when 8 G = identity
constexpr int DLOG_PARAM_WORDS = 128;

BJJ_HD u64 dlog_entries(int b) { return ((u64)1 << b) + 1; }
BJJ_HD u64 dlog_slots(int b) { return (u64)1 << (b + 2); }
BJJ_HD int dlog_max_range_bits(int b) { return b + 1 + BJJ_DLOG_GIANT_BITS; }
// giant steps a search over [0, 2^range_bits) takes at most
BJJ_HD u32 dlog_steps(int b, int range_bits) { return range_bits <= b + 1 ? 1u : (u32)1 << (range_bits - b - 1); }

// k * g, k < 2^nbits, MSB first; the addition is computed unconditionally and selected (uniform control flow)
BJJ_HD Ext dlog_mul_small(const Niels& g, u64 k, int nbits) {
  Ext acc = ext_identity();
#pragma unroll 1
  for (int i = nbits - 1; i >= 0; i--) {
    acc = ext_dbl<true>(acc);
    const Ext sum = ext_madd(acc, g);
    const bool bit = (k >> i) & 1;
    acc.X = fr_select(bit, sum.X, acc.X); acc.Y = fr_select(bit, sum.Y, acc.Y);
    acc.Z = fr_select(bit, sum.Z, acc.Z); acc.T = fr_select(bit, sum.T, acc.T);
  }
  return acc;
}
BJJ_HD Niels dlog_niels_neg(const Niels& n) { return Niels{n.ypx, n.ymx, fr_canon(fr_neg(n.t2d))}; }
BJJ_HD Niels dlog_affine_niels(const Ext& p, const Consts& K) {
  const Fr zi = fr_inv(p.Z);
  return niels_from_affine(fr_mul(p.X, zi), fr_mul(p.Y, zi), K, false);
}

// One thread, once per table: the three fixed points of the search, the base point's canonical record and the order test.
// (bx, by): the base point in Montgomery form (a record's coordinates >= r are reduced by the conversion), ON the curve.
BJJ_HD void dlog_setup(u32* params, const Fr& bx, const Fr& by, int b, const Consts& K) {
  const Ext G = ext_from_ref_affine(bx, by, K);
  store_niels(params + DLOG_P_G, niels_from_affine(G.X, G.Y, K, false));
  const Ext G8 = ext_dbl<false>(ext_dbl<false>(ext_dbl<false>(G)));
  params[DLOG_P_SMALL] = (fr_is_zero(G8.X) && fr_eq(G8.Y, G8.Z)) ? 1u : 0u;   // the eight points of order <= 8
  Ext H = G;
#pragma unroll 1
  for (int i = 0; i < b; i++) H = ext_dbl<false>(H);
  store_niels(params + DLOG_P_NEG_HALF, dlog_niels_neg(dlog_affine_niels(H, K)));
  store_niels(params + DLOG_P_NEG_STRIDE, dlog_niels_neg(dlog_affine_niels(ext_dbl<false>(H), K)));
  fr_from_mont_words(bx, params + DLOG_P_XY);
  fr_from_mont_words(by, params + DLOG_P_XY + 8);
  for (int i = DLOG_P_SMALL + 1; i < DLOG_PARAM_WORDS; i++) params[i] = 0;
}

// ---- the table ------------------------------------------------------------------------------------------------------------------
// the key of p: y = Y / Z as its canonical representative IN MONTGOMERY FORM (y * 2^261 mod r, below r), 8 words; zinv = 1 / p.Z in
// Montgomery form.  The form is a bijection of the field, so it identifies y as well as the plain integer does and its bits are as
// uniform; leaving it saves every giant step the multiplication that would take it out.
BJJ_HD void dlog_canon_y(const Ext& p, const Fr& zinv, u32 yw[8]) {
  fr_to_words(fr_canon(fr_mul(p.Y, zinv)), yw);
}
BJJ_HD u32 dlog_index(const u32 yw[8], u32 mask) { return yw[0] & mask; }
template <int TAG_BITS>
BJJ_HD u32 dlog_tag(const u32 yw[8]) { return TAG_BITS >= 32 ? yw[1] : yw[1] & (((u32)1 << (TAG_BITS & 31)) - 1u); }
BJJ_HD u64 dlog_slot_value(u32 tag, u32 j) { return ((u64)tag << 32) | (u64)(j + 1); }

// Slots: a policy with load(i) and cas(i, v) (v into slot i if that is empty; true when it went in) -- the kernels' reads and
// 64-bit atomics on global memory, the CPU program's bounded array.
// Walks the probe sequence of (idx, tag) from offset `probe`, whose slot `s` is already loaded: j + 1 of the first slot with this
// tag (probe = its offset), or 0 when an empty slot ends the run.
template <class Slots>
BJJ_HD u32 dlog_walk(const Slots& S, u32 mask, u32 idx, u32 tag, u32& probe, u64 s) {
  for (;;) {
    if (s == 0) return 0;
    if ((u32)(s >> 32) == tag) return (u32)s;
    if (probe >= mask) return 0;
    probe++;
    s = S.load((idx + probe) & mask);
  }
}
// build: entry j with the point acc = j * G and zinv = 1 / acc.Z.  The slot an entry lands in depends on who came first; no
// lookup result does.  False only for a table without a free slot, which a quarter-full table never is.
template <int TAG_BITS, class Slots>
BJJ_HD bool dlog_insert(const Slots& S, u32 mask, u32 j, const Ext& acc, const Fr& zinv) {
  u32 yw[8];
  dlog_canon_y(acc, zinv, yw);
  const u32 idx = dlog_index(yw, mask);
  const u64 v = dlog_slot_value(dlog_tag<TAG_BITS>(yw), j);
  for (u32 p = 0;; p++) {
    if (S.cas((idx + p) & mask, v)) return true;
    if (p >= mask) return false;
  }
}
// check: j * G by a route that shares nothing with the build chain -- projective double-and-add from the affine base point, its
// own inversion -- must be found under its own y with exactly j.  Returns the number of violated conditions (0 or 1).
template <int TAG_BITS, class Slots>
BJJ_HD int dlog_check_entry(const Slots& S, u32 mask, const u32* params, u32 j, int b, const Consts& K) {
  const Ext base = ext_from_ref_affine(fr_to_mont_words(params + DLOG_P_XY), fr_to_mont_words(params + DLOG_P_XY + 8), K);
  const PNiels bn = ext_to_pniels(base, K), idn = pniels_identity();
  Ext acc = ext_identity();
#pragma unroll 1
  for (int i = b; i >= 0; i--) {
    acc = ext_dbl<true>(acc);
    const bool bit = (j >> i) & 1;
    PNiels sel;
    sel.ymx = fr_select(bit, bn.ymx, idn.ymx); sel.ypx = fr_select(bit, bn.ypx, idn.ypx);
    sel.t2d = fr_select(bit, bn.t2d, idn.t2d); sel.z2 = fr_select(bit, bn.z2, idn.z2);
    acc = ext_add_pn(acc, sel);
  }
  u32 yw[8];
  dlog_canon_y(acc, fr_inv(acc.Z), yw);
  const u32 idx = dlog_index(yw, mask), tag = dlog_tag<TAG_BITS>(yw);
  u32 probe = 0;
  for (;;) {
    const u32 hit = dlog_walk(S, mask, idx, tag, probe, S.load((idx + probe) & mask));
    if (hit == 0) return 1;
    if (hit == j + 1) return 0;
    if (probe >= mask) return 1;
    probe++;
  }
}
// check: one slot.  occupied counts towards the total that must equal the number of entries; a value outside 1 .. 2^b + 1 is a
// violated condition of its own.
BJJ_HD int dlog_check_slot(u64 s, int b, u32& occupied) {
  occupied = s != 0;
  return s != 0 && ((u32)s == 0 || (u64)(u32)s > dlog_entries(b));
}

// ---- one item -----------------------------------------------------------------------------------------------------------------
enum : int { DL_SEARCH = 0, DL_PENDING = 1, DL_DONE = 2, DL_EXHAUSTED = 3, DL_SKIP = 4 };
struct DlogLane {
  Ext Q;        // P - c_i G while searching or waiting for confirmation; the identity for a lane without an item
  u64 m;        // the answer, UINT64_MAX until one is confirmed in range
  u32 i;        // giant step
  u32 probe;    // offset in the probe sequence of Q's y to go on from
  u32 cand;     // j + 1 of the tag hit that waits for confirmation
  int st, ok;
};
// ok[i] between the launches of a cut call: an item whose walk is not over yet carries this value, which no result has; the launch
// that holds the call's last step writes 0 in its place.  A decided item -- found, off the curve, or confirmed at or beyond
// 2^range_bits -- keeps its result and is passed by.
#define BJJ_DLOG_IN_FLIGHT 0xFF
BJJ_HD bool dlog_resumes(u32 s0, u32 ok_byte) { return s0 == 0 || ok_byte == BJJ_DLOG_IN_FLIGHT; }
BJJ_HD void dlog_idle(DlogLane& L) {
  L.Q = ext_identity(); L.m = ~(u64)0; L.i = 0; L.probe = 0; L.cand = 0; L.st = DL_SKIP; L.ok = 0;
}
// The item's record -> the lane at giant step s0 (the first step of this launch).  A record off the curve is finished here:
// the addition law is complete only on the curve.
BJJ_HD void dlog_start(DlogLane& L, const void* rec, const u32* params, u32 s0, const Consts& K) {
  u32 w[8];
  load_w8(rec, w);                   const Fr x = fr_to_mont_words(w);
  load_w8((const char*)rec + 32, w); const Fr y = fr_to_mont_words(w);
  dlog_idle(L);
  L.i = s0;
  if (!ref_on_curve(x, y, K)) { L.st = DL_DONE; L.ok = 2; return; }
  Ext Q = ext_madd(ext_from_ref_affine(x, y, K), load_niels(params + DLOG_P_NEG_HALF));
  if (s0 != 0) {   // a later launch of a call that was cut: s0 giant strides at once, s0 < 2^BJJ_DLOG_GIANT_BITS
    const Ext A = dlog_mul_small(load_niels(params + DLOG_P_NEG_STRIDE), s0, BJJ_DLOG_GIANT_BITS);
    Q = ext_add_pn(A, ext_to_pniels(Q, K));
  }
  L.Q = Q;
  L.st = DL_SEARCH;
}
// One giant step of a searching lane: y of Q, the slot it names, Q's successor while that read is in flight, then the walk.
template <int TAG_BITS, class Slots>
BJJ_HD void dlog_step(DlogLane& L, const Fr& zinv, const Niels& neg_stride, const Slots& S, u32 mask, u32 s1) {
  if (L.st != DL_SEARCH) return;
  u32 yw[8];
  dlog_canon_y(L.Q, zinv, yw);
  const u32 idx = dlog_index(yw, mask), tag = dlog_tag<TAG_BITS>(yw);
  const u64 first = S.load((idx + L.probe) & mask);
  const Ext next = ext_madd(L.Q, neg_stride);
  u32 probe = L.probe;
  const u32 hit = dlog_walk(S, mask, idx, tag, probe, first);
  if (hit != 0) { L.cand = hit; L.probe = probe; L.st = DL_PENDING; return; }
  L.Q = next; L.probe = 0; L.i++;
  if (L.i >= s1) L.st = DL_EXHAUSTED;
}
// what a launch leaves in ok[i] for its lane; last: the launch holds the call's last giant step
BJJ_HD u32 dlog_ok_byte(const DlogLane& L, bool last) { return (L.st == DL_EXHAUSTED && !last) ? (u32)BJJ_DLOG_IN_FLIGHT : (u32)L.ok; }
// Every lane runs the ladder (uniform trip count); only a waiting lane acts on it.  True when the hit was a false one.
BJJ_HD bool dlog_confirm(DlogLane& L, const Niels& g, int b, int range_bits) {
  const bool waiting = L.st == DL_PENDING;
  const u32 j = waiting ? L.cand - 1u : 0u;
  const Ext J = dlog_mul_small(g, j, b + 1);
  if (!waiting) return false;
  const bool same_y = fr_eq(fr_mul(J.Y, L.Q.Z), fr_mul(L.Q.Y, J.Z));
  const Fr a = fr_mul(J.X, L.Q.Z), c = fr_mul(L.Q.X, J.Z);
  const bool plus = fr_eq(a, c), minus = fr_is_zero(fr_add(a, c));
  if (j <= ((u32)1 << b) && same_y && (plus || minus)) {
    const u64 centre = ((u64)1 << b) + (u64)L.i * ((u64)2 << b);
    const u64 m = plus ? centre + j : centre - j;
    const bool in = m < ((u64)1 << range_bits);   // m is the only logarithm below the order: outside the range, nothing is inside
    L.ok = in ? 1 : 0;
    L.m = in ? m : ~(u64)0;
    L.st = DL_DONE;
    return false;
  }
  L.st = DL_SEARCH;
  L.probe++;
  return true;
}

}  // namespace bjj
