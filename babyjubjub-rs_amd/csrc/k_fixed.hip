// libbjj_hip.so, kernel unit 1: the fixed-base table (build / check) and K1, B8.mul_scalar(n)
// (src/lib.rs:149-164 with self = B8, src/lib.rs:37-46; the engine of PrivateKey::public, :304-306).
#include "k_common.hpp"

// workgroup size / resident workgroups per CU / staging areas per wave of K1 (A/B knobs; default: one 512-lane workgroup
// per CU = 2 waves per SIMD, two 8 KB staging areas per wave)
#ifndef BJJ_K1_BLOCK
#define BJJ_K1_BLOCK BJJ_EPI_BLOCK
#endif
#ifndef BJJ_K1_MIN_BLOCKS
#define BJJ_K1_MIN_BLOCKS 1
#endif
#ifndef BJJ_K1_NBUF
#define BJJ_K1_NBUF 2
#endif
// the inversion core of K1's epilogue (A/B knob; default: the division-step core, fr.hpp: fr_inv_k1)
#ifndef BJJ_K1_INV_CORE
#define BJJ_K1_INV_CORE INV_K1
#endif
// The overlap form (bjj_k_mul_fixed_base_2x256[_c32]) may start work ahead of need; each part has its own A/B knob
// (profiles/r10_ab_k1_item_pipeline.txt):
//   BJJ_K1_PIPE_ITEM    the next item's scalar, digits and first two gathers before the current item's last addition: on,
//                       +1.8 ... 2.1 % on two streams
//   BJJ_K1_PIPE_RECORD  phase 2 loads the record of item m-1 before the five multiplications of item m: off, -0.3 ... -0.8 %
//   BJJ_K1_EARLY_RECORD phase 2's first record is requested before the workgroup inversion, not after its last barrier: off,
//                       -0.4 ... -0.7 %
#ifndef BJJ_K1_PIPE_ITEM
#define BJJ_K1_PIPE_ITEM 1
#endif
#ifndef BJJ_K1_PIPE_RECORD
#define BJJ_K1_PIPE_RECORD 0
#endif
#ifndef BJJ_K1_EARLY_RECORD
#define BJJ_K1_EARLY_RECORD 0
#endif
// What the overlap form's item boundary (BJJ_K1_PIPE_ITEM) no longer waits for or computes twice; each part has its own A/B
// knob (profiles/r11_ab_k1_item_boundary.txt):
//   BJJ_K1_LATE_SCALAR  the next scalar's load and the stash stores of the item before are issued BEHIND the two waits that
//                       open an item, so that those wait for the two gathers alone
//   BJJ_K1_FOLD_LIFT    the first addition takes Y - X, Y + X, 2Z straight from window 0's entry (twice y - x', twice y + x',
//                       the constant 4): no lift to an extended point that the addition then takes apart again
//   BJJ_K1_WEAK_MOD_L   the scalar is reduced without the last conditional subtraction (bjj_device.hpp: scalar_mod_l_weak)
//   BJJ_K1_SLOT_STRIP   a gather's slot numbers go through a wave-private LDS strip (k_common.hpp: GatherCoopLds<2, true>)
// All four on: +2.0 ... 2.2 % on two streams in four interleaved rounds; none loses alone (fold is the largest at about +1 %),
// and the build is not faster without any of them.
#ifndef BJJ_K1_LATE_SCALAR
#define BJJ_K1_LATE_SCALAR 1
#endif
#ifndef BJJ_K1_FOLD_LIFT
#define BJJ_K1_FOLD_LIFT 1
#endif
#ifndef BJJ_K1_WEAK_MOD_L
#define BJJ_K1_WEAK_MOD_L 1
#endif
#ifndef BJJ_K1_SLOT_STRIP
#define BJJ_K1_SLOT_STRIP 1
#endif
// Glue instructions of the overlap form that the result does not need; each part has its own A/B knob (DESIGN.md section 6,
// profiles/r12_ab_k1_glue.txt):
//   BJJ_K1_SIGN_CARRY   the accumulator carries the sign of the current digit, so a table entry is used as it leaves LDS: no
//                       swap of y - x' / y + x' and no negated 2D'x'y per window (the comment above K1Acc); needs BJJ_K1_FOLD_LIFT
//   BJJ_K1_REG_RECORDS  phase 2 has its own loop (k1_epilogue_run) and takes the four values of a record apart, and its results
//                       together, in registers: through an array of eight words the compiler routes them through LDS
//   BJJ_K1_ADDR_MAD     k_common.hpp: one multiply-add per address of the gather
#ifndef BJJ_K1_SIGN_CARRY
#define BJJ_K1_SIGN_CARRY 1
#endif
#ifndef BJJ_K1_REG_RECORDS
#define BJJ_K1_REG_RECORDS 1
#endif
//   BJJ_K1_UNIFORM_STAGE the wave's staging area is addressed from the wave index as a scalar (one v_readfirstlane_b32 per launch):
//                       the LDS base of each of a gather's eight loads, which goes to M0, was a vector add and a
//                       v_readfirstlane_b32 per load
//   BJJ_K1_ALIGN_DIGITS the digit stream moves down by one v_alignbit_b32 per word (k1_digit_next); for a run-time width the
//                       compiler forms digit_next's funnel shift from a shift and a shift-or
#ifndef BJJ_K1_UNIFORM_STAGE
#define BJJ_K1_UNIFORM_STAGE 1
#endif
#ifndef BJJ_K1_ALIGN_DIGITS
#define BJJ_K1_ALIGN_DIGITS 1
#endif
#define K1_SIGN_CARRY (BJJ_K1_SIGN_CARRY && BJJ_K1_FOLD_LIFT)   // it works on the folded state: off without it

// ---------------------------------------------------------------------------
// init: fixed-base table (layout and recoding: bjj_device.hpp "fixed base").
//   bases:  one thread per window j -> P_j = 2^(W j) * B8 (ladder + inversion; nwin threads)
//   build:  one thread per chain of `chain` consecutive digits of one window (fixed_table_chain)
//   check:  one thread per entry, link conditions of fixed_table_check_slot (bjj_check_table)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64) bjj_k_fixed_window_bases(u32* bases, int W, int nwin) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nwin) return;
  store_niels(bases + (size_t)j * NIELS_WORDS, fixed_table_entry(1u, j, W, c_K));
}
__global__ void __launch_bounds__(BJJ_BLOCK) bjj_k_build_fixed_table(u32* table, const u32* __restrict__ bases, int W, int nwin,
                                                                 u32 chain) {
  const size_t stride = fixed_stride(W);
  const size_t cpw = (stride + chain - 1) / chain;  // chains per window
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cpw * (size_t)nwin) return;
  const int j = (int)(t / cpw);
  const size_t k0 = (t % cpw) * chain;
  const u32 cnt = (u32)(stride - k0 < chain ? stride - k0 : chain);
  fixed_table_chain(table, load_niels(bases + (size_t)j * NIELS_WORDS), (size_t)j * stride + k0, (u32)k0, cnt, W, c_K);
}
__global__ void __launch_bounds__(BJJ_BLOCK) bjj_k_check_fixed_table(const u32* __restrict__ table, const u32* __restrict__ bases,
                                                                 int W, int nwin, unsigned long long* bad) {
  const size_t stride = fixed_stride(W);
  const size_t total = stride * (size_t)nwin, nthreads = (size_t)gridDim.x * blockDim.x;
  unsigned long long mine = 0;
#pragma unroll 1
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += nthreads)
    mine += (unsigned long long)fixed_table_check_slot(table, bases, (int)(e / stride), (u32)(e % stride), W, nwin, c_K);
  if (mine) atomicAdd(bad, mine);
}


// ---- the overlap form's split of fixed_base_mul (bjj_device.hpp) and of the epilogue (k_common.hpp) ----------------------
// fixed_base_mul in two halves, so that K1's loop can begin item k+1 while item k still has its last addition to do: `begin`
// reduces the scalar (loaded one item earlier still), opens the digit stream and issues the gathers of windows 0 and 1 (both
// staging areas: they are free once the item before has its last entry in registers); `windows` completes them and runs every
// addition but the last, whose entry it returns.  The digits, the order of the additions and so the result are fixed_base_mul's.
struct K1Item {
  DigitStream ds;
  bool neg0, neg1;
};
// fr_from_words on the two loaded vectors, word by word from registers.  Through an array of eight words the compiler fetches
// the word pairs that straddle a limb as vectors at odd offsets, keeps the array in scratch for that, and every item began
// with a store to scratch, a load back and a wait for it.
__device__ __forceinline__ u32 k1_limb(u32 lo, u32 hi, int sh) { return ((lo >> sh) | (hi << (32 - sh))) & MASK29; }
__device__ __forceinline__ Fr k1_scalar_limbs(const U4 (&v)[2]) {
  Fr s;
  s.v[0] = v[0].x & MASK29;
  s.v[1] = k1_limb(v[0].x, v[0].y, 29); s.v[2] = k1_limb(v[0].y, v[0].z, 26); s.v[3] = k1_limb(v[0].z, v[0].w, 23);
  s.v[4] = k1_limb(v[0].w, v[1].x, 20); s.v[5] = k1_limb(v[1].x, v[1].y, 17); s.v[6] = k1_limb(v[1].y, v[1].z, 14);
  s.v[7] = k1_limb(v[1].z, v[1].w, 11);
  s.v[8] = v[1].w >> 8;
  return s;
}
// digit_next (bjj_device.hpp) with the shift register moved by funnel shifts: the same digits, slots and carries
__device__ __forceinline__ size_t k1_digit_next(DigitStream& d, bool& neg) {
  if (!BJJ_K1_ALIGN_DIGITS) return digit_next(d, neg);
  const u32 u = (d.w[0] & d.mask) + d.carry;
  neg = u > d.half;
  d.carry = neg ? 1u : 0u;
  const u32 dig = neg ? (d.mask + 1u) - u : u;
  const size_t slot = d.base + dig;
  d.base += d.stride;
#pragma unroll
  for (int i = 0; i < 7; i++) d.w[i] = __builtin_amdgcn_alignbit(d.w[i + 1], d.w[i], (u32)d.W);   // 4 <= W <= 28
  d.w[7] >>= d.W;
  return slot;
}
template <class G>
__device__ __forceinline__ K1Item k1_item_begin(const G& g, int W, const U4 (&scalar)[2]) {
  u32 sc[8];
  Fr s = scalar_mod_l_weak_limbs(k1_scalar_limbs(scalar), scalar[1].w >> 24, c_K);
  if (!BJJ_K1_WEAK_MOD_L) s = fr_cond_sub_kr(s, c_K.L.v);   // scalar_mod_l
  fr_to_words(s, sc);
  K1Item it;
  it.ds = digit_stream(sc, W);
  typename G::Pending p;
  g.issue(k1_digit_next(it.ds, it.neg0), p, 0);
  g.issue(k1_digit_next(it.ds, it.neg1), p, 1);
  return it;
}
#if BJJ_K1_FOLD_LIFT
// The accumulator between two additions as ext_madd first forms it: Y - X, Y + X and 2Z (lazy) and T.  Kept in this shape the
// window loop stays rolled, does per trip exactly what ext_madd does, and window 0's entry (x', y) -- in T form -- IS a
// state: Y - X = 2(y - x'), Y + X = 2(y + x'), 2Z = 4, T = 2x'y of the point (2x' : 2y : 2 : 2x'y) that fixed_base_mul lifts it to.
//
// BJJ_K1_SIGN_CARRY.  Let eps_j = +-1 be the sign of window j's digit, Q_j its entry as stored, S_j = sum_{i <= j} eps_i Q_i the
// partial sum fixed_base_mul holds after window j.  The loop holds R_j = eps_j S_j instead:
//     R_0 = Q_0,      R_j = (eps_j eps_{j-1}) R_{j-1} + Q_j,      result S_last = eps_last R_last = R_last,
// so an addition takes its entry exactly as the gather returns it, and what is negated -- when two neighbouring digits differ in
// sign -- is the accumulator.  That costs nothing where the accumulator is made: -(X, Y, Z, T) = (-X, Y, Z, -T), and in the
// addition X = e f and T = e h share the factor e = b - a, so addition j-1 forms e as b - a or a - b by ONE select on
// eps_j eps_{j-1} (`flip`; the digit of window j is drawn before addition j-1 runs, for its gather).  The last addition does not
// flip: eps_last = +1 always, because the reduced scalar is not negative -- a negative top digit would leave a carry behind the
// top window, which scalar_mod_l_weak's contract excludes for every width (bjj_device.hpp; tests/test_k1_weak_mod_l_host.py) --
// so R_last is S itself.  Window 0 has no addition before it: its state swaps Y - X / Y + X and
// negates T (lazily) by eps_0 eps_1, which are the selects and the negation it had for eps_0 and for window 1's t2d.
// Bounds: a and b are N-form products < 2r, and fr_sub_lazy is the same function of either order, so e keeps < 6r with limbs
// < 1.5 * 2^30 and every other operand is untouched; the entry's t2d is now always N-form < 2r, and the one lazy negation left,
// window 0's T (limbs < 2^30, < 4r), meets that N-form t2d in c = T * t2d, the mirror image of the pair it replaces.
// Per window: 18 selects and 9 subtractions plus 9 selects on the entry go, 9 subtractions and 9 selects on e come.
// The functions are curve.hpp's (MaddState), which the host model tests/emul/k1_sign_carry_main.cpp runs as well.
typedef MaddState K1Acc;
// ext_madd on that state.  Operand bounds as in curve.hpp: ym < 6r with limbs < 1.5 * 2^30, yp < 4r and d < 4r with limbs
// < 2^30, T N-form; the entry N-form < 2r but for t2d, which may be a lazy negation (limbs < 2^30, < 4r).
template <bool NEED_T = true>
__device__ __forceinline__ Ext k1_madd(const K1Acc& s, const Niels& q, bool flip = false) {
  return ext_madd_state<NEED_T>(s, q, K1_SIGN_CARRY && flip);
}
__device__ __forceinline__ K1Acc k1_forms(const Ext& p) { return ext_madd_forms(p); }
#else
typedef Ext K1Acc;
template <bool NEED_T = true>
__device__ __forceinline__ Ext k1_madd(const K1Acc& s, const Niels& q, bool = false) { return ext_madd<NEED_T>(s, q); }
__device__ __forceinline__ K1Acc k1_forms(const Ext& p) { return p; }
#endif
// the entry of a window as the additions take it: as stored, or negated by its digit's sign
__device__ __forceinline__ Niels k1_entry(const Niels& e, bool neg) { return K1_SIGN_CARRY ? e : niels_cneg_lazy(e, neg); }
// `mid` runs once both staged entries are in registers: the place for memory traffic that the two waits must not cover.
template <class G, class MID>
__device__ __forceinline__ void k1_item_windows(const G& g, int nwin, K1Item& it, K1Acc& acc, Niels& cur, const MID& mid) {
  typename G::Pending p;
  bool neg, last = false;   // BJJ_K1_SIGN_CARRY: the sign of the digit before
#if K1_SIGN_CARRY
  acc = niels_tform_state(g.finish(p, 0), it.neg0 != it.neg1, it.neg0 != it.neg1);   // (eps_0 eps_1) Q_0
  BJJ_SCHED_FENCE();
  cur = g.finish(p, 1);
  last = it.neg1;
#elif BJJ_K1_FOLD_LIFT
  const Niels e0 = g.finish(p, 0);
  const Fr ymx0 = fr_select(it.neg0, e0.ypx, e0.ymx), ypx0 = fr_select(it.neg0, e0.ymx, e0.ypx);
  acc.ym = fr_add_lazy(ymx0, ymx0);              // twice an N-form entry < 2r: lazy sums, limbs < 2^30, < 4r
  acc.yp = fr_add_lazy(ypx0, ypx0);
  acc.d = fr_add(fr_add(fr_one(), fr_one()), fr_add(fr_one(), fr_one()));   // the constant 4: N-form, < 4r
  acc.T = e0.t2d;                                // N-form as stored; window 0's sign goes to window 1's t2d: C = T * t2d
  BJJ_SCHED_FENCE();
  const Niels e1 = g.finish(p, 1);
  cur = niels_cneg_lazy(e1, it.neg1);
  cur.t2d = fr_select(it.neg0 != it.neg1, fr_sub_lazy(fr_zero(), e1.t2d), e1.t2d);
#else
  const Niels n0 = niels_cneg_lazy(g.finish(p, 0), it.neg0);
  acc.X = fr_reduce_weak(fr_sub(n0.ypx, n0.ymx));  // window 0 lifted to (2x' : 2y : 2 : 2x'y), as fixed_base_mul
  acc.Y = fr_add(n0.ypx, n0.ymx);
  acc.Z = fr_add(fr_one(), fr_one()); acc.T = fr_add(n0.t2d, fr_zero());
  BJJ_SCHED_FENCE();
  cur = niels_cneg_lazy(g.finish(p, 1), it.neg1);
#endif
  mid();
#pragma unroll 1
  for (int j = 1; j + 1 < nwin; j++) {
    g.issue(k1_digit_next(it.ds, neg), p, (j + 1) & 1);
    acc = k1_forms(k1_madd(acc, cur, neg != last));   // window j's addition, negated where window j + 1 changes the sign
    if (K1_SIGN_CARRY) last = neg;
    BJJ_SCHED_FENCE();
    cur = k1_entry(g.finish(p, (j + 1) & 1), neg);
  }
}
// epilogue_stash (k_common.hpp) in two halves: the four packed values of an item wait in registers until its stores may go.
struct K1Stash { U4 x[2], y[2], z[2], p[2]; };
// BJJ_K1_REG_RECORDS: fr_to_words into two vectors, word by word from the limbs (word j starts 32 j - 29 floor(32 j / 29) bits into
// limb floor(32 j / 29) and ends in the next one), as k1_scalar_limbs does the other way: no array of eight words.
__device__ __forceinline__ void k1_words(U4 (&v)[2], const Fr& f) {
  const u32* a = f.v;
  v[0] = U4{a[0] | (a[1] << 29), (a[1] >> 3) | (a[2] << 26), (a[2] >> 6) | (a[3] << 23), (a[3] >> 9) | (a[4] << 20)};
  v[1] = U4{(a[4] >> 12) | (a[5] << 17), (a[5] >> 15) | (a[6] << 14), (a[6] >> 18) | (a[7] << 11), (a[7] >> 21) | (a[8] << 8)};
}
__device__ __forceinline__ void k1_stash_words(U4 (&v)[2], const Fr& f) {
  if (BJJ_K1_REG_RECORDS) { k1_words(v, f); return; }
  u32 w[8];
  fr_to_words(f, w);
  v[0] = U4{w[0], w[1], w[2], w[3]}; v[1] = U4{w[4], w[5], w[6], w[7]};
}
__device__ __forceinline__ void k1_stash_pack(K1Stash& s, const Ext& p, Fr& run) {
  k1_stash_words(s.x, p.X); k1_stash_words(s.y, p.Y); k1_stash_words(s.z, p.Z); k1_stash_words(s.p, run);
  run = fr_mul(run, p.Z);
}
__device__ __forceinline__ void k1_stash_store(const K1Stash& s, uint8_t* xy_item, u32* scr_item) {
  U4 *q = (U4*)xy_item, *r = (U4*)scr_item;
  q[0] = s.x[0]; q[1] = s.x[1]; q[2] = s.y[0]; q[3] = s.y[1];
  r[0] = s.z[0]; r[1] = s.z[1]; r[2] = s.p[0]; r[3] = s.p[1];
}
// An item's phase-1 record in registers, and epilogue_finish's arithmetic on it: loading and finishing apart, so that the
// loads of one record run under the multiplications of another.
struct K1Record {
  U4 z[2], p[2], x[2], y[2];   // as loaded: nothing waits for a record before k1_record_finish reads it
};
__device__ __forceinline__ void k1_record_load(K1Record& r, const uint8_t* xy_item, const u32* scr_item) {
  const U4 *s = (const U4*)scr_item, *q = (const U4*)xy_item;
  r.z[0] = s[0]; r.z[1] = s[1]; r.p[0] = s[2]; r.p[1] = s[3];
  r.x[0] = q[0]; r.x[1] = q[1]; r.y[0] = q[2]; r.y[1] = q[3];
}
__device__ __forceinline__ Fr k1_record_fr(const U4 (&v)[2]) {
  if (BJJ_K1_REG_RECORDS) return k1_scalar_limbs(v);
  const u32 w[8] = {v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y, v[1].z, v[1].w};
  return fr_from_words(w);
}
template <unsigned FORM>
__device__ __forceinline__ void k1_record_finish(Fr& inv, uint8_t* out_item, const K1Record& r) {
  constexpr u32 R1[NL] = {BJJ_N0, BJJ_N1, BJJ_N2, BJJ_N3, BJJ_N4, BJJ_N5, BJJ_N6, BJJ_N7, BJJ_N8};
  const Fr Z = k1_record_fr(r.z), P = k1_record_fr(r.p), X = k1_record_fr(r.x), Y = k1_record_fr(r.y);
  Fr zinv = fr_mul(inv, P);               // plain 1/Z
  inv = fr_mul(inv, Z);
  Fr c2 = fr_mul(zinv, c_K.FINV);         // plain 1/(Z F)
  Fr x = fr_cond_sub_kr(fr_mul(X, c2), R1);
  Fr y = fr_cond_sub_kr(fr_mul(Y, zinv), R1);
  if (BJJ_K1_REG_RECORDS) {
    U4 *const o = (U4*)out_item, v[2];
    if (FORM & EPI_COMPRESS) {
      k1_words(v, y);
      if (plain_gt_halfq(x, c_K)) v[1].w |= 0x80000000u;
      o[0] = v[0]; o[1] = v[1];
    } else {
      k1_words(v, x); o[0] = v[0]; o[1] = v[1];
      k1_words(v, y); o[2] = v[0]; o[3] = v[1];
    }
    return;
  }
  u32 w[8];
  if (FORM & EPI_COMPRESS) {
    fr_to_words(y, w);
    if (plain_gt_halfq(x, c_K)) w[7] |= 0x80000000u;
    store_w8(out_item, w);
  } else {
    fr_to_words(x, w); store_w8(out_item, w);
    fr_to_words(y, w); store_w8(out_item + 32, w);
  }
}
// epilogue_run for the overlap form.  A lane's items are finished last to first; `stash` is where phase 1 put X, Y (the output
// itself for the affine form).  The first record is the one this lane stored last in phase 1: with BJJ_K1_EARLY_RECORD its loads
// are issued behind a wait for those stores and complete under the inversion.
template <int BLOCK, unsigned FORM>
__device__ __forceinline__ void k1_epilogue_run(Fr run, size_t n, size_t tid, size_t nthreads, uint8_t* out, const uint8_t* stash,
                                                const u32* scratch, u32* lds) {
  constexpr size_t OUT_BYTES = (FORM & EPI_COMPRESS) ? 32 : 64;
  const size_t cnt = tid < n ? (n - tid + nthreads - 1) / nthreads : 0;
  K1Record cur;
  if (BJJ_K1_EARLY_RECORD && cnt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this lane's phase-1 stores of the same addresses
    const size_t i = tid + (cnt - 1) * nthreads;
    k1_record_load(cur, stash + i * 64, scratch + i * 16);
  }
  Fr inv = fr_mul(block_invert<BLOCK, BJJ_K1_INV_CORE>(run, lds), fr_one_plain());  // out of Montgomery form once per lane
  if (!cnt) return;
  if (!BJJ_K1_EARLY_RECORD) {
    const size_t i = tid + (cnt - 1) * nthreads;
    k1_record_load(cur, stash + i * 64, scratch + i * 16);
  }
#pragma unroll 1
  for (size_t m = cnt; m-- > 0;) {
    const size_t i = tid + m * nthreads;
    if (BJJ_K1_PIPE_RECORD) {
      K1Record nxt = cur;
      if (m) k1_record_load(nxt, stash + (i - nthreads) * 64, scratch + (i - nthreads) * 16);
      k1_record_finish<FORM>(inv, out + i * OUT_BYTES, cur);
      cur = nxt;
    } else {
      k1_record_finish<FORM>(inv, out + i * OUT_BYTES, cur);
      if (m) k1_record_load(cur, stash + (i - nthreads) * 64, scratch + (i - nthreads) * 16);
    }
  }
}

// FORM = EPI_AFFINE: out holds 64-byte points and doubles as the phase-1 stash (xy == out); EPI_COMPRESS: out holds 32-byte
// Point::compress records (src/lib.rs:166-178) and the stash is the scratch set's XY area.
// AHEAD: the overlap form, which starts the next item and the next phase-2 record ahead of need (the knobs above).
template <int BLOCK, int NBUF, unsigned FORM = EPI_AFFINE, bool AHEAD = false>
__device__ __forceinline__ void mul_fixed_base_body(const u32* __restrict__ table, int W, int nwin, const uint8_t* __restrict__ scalars,
                                                    size_t n, uint8_t* __restrict__ out, u32* __restrict__ scratch,
                                                    uint8_t* __restrict__ xy = nullptr) {
  __shared__ u32 lds[NL * 64];
  constexpr bool STRIP = AHEAD && BJJ_K1_PIPE_ITEM && BJJ_K1_SLOT_STRIP;   // the overlap form's gather: k_common.hpp
  constexpr int WAVE_WORDS = NBUF * FB_STAGE_WORDS + (STRIP ? FB_STRIP_WORDS : 0);
  __shared__ __attribute__((aligned(16))) u32 stage[(BLOCK / 64) * WAVE_WORDS];
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nthreads = (size_t)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  // the wave index as the compiler can see it is uniform (BJJ_K1_UNIFORM_STAGE; the overlap form only)
  const int wave = AHEAD && BJJ_K1_UNIFORM_STAGE ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : (int)(threadIdx.x >> 6);
  const GatherCoopLds<NBUF, STRIP> fb = {table, stage + wave * WAVE_WORDS, lane};
  uint8_t* const stash = (FORM & EPI_COMPRESS) ? xy : out;
  Fr run = fr_one();
  if (AHEAD && BJJ_K1_PIPE_ITEM) {
    static_assert(!AHEAD || NBUF >= 2, "both gathers of the next item are issued at once");
    size_t i = tid;
    if (i - lane < n) {  // wave-uniform, as every branch of this loop: the gathers are cooperative
      const U4* const sc4 = (const U4*)scalars;
      U4 raw[2] = {sc4[2 * (i < n ? i : n - 1)], sc4[2 * (i < n ? i : n - 1) + 1]};
      K1Item it = k1_item_begin(fb, W, raw);
      // BJJ_K1_LATE_SCALAR: an item opens with two waits for ALL of the wave's memory traffic (one counter), meant for its two
      // gathers, which were issued an addition earlier.  So nothing else is in flight then: the stash of the item before
      // waits packed in `held` (32 registers, over a span without a multiplication) and is stored behind those waits, where
      // the next scalar is requested as well; the first wait to cover either is the one that ends the first window trip.
      K1Stash held = {};
      bool pending = false;   // wave-uniform
      size_t iheld = 0;
#pragma unroll 1
      for (;;) {
        const size_t inext = i + nthreads, iload = inext < n ? inext : n - 1;   // a lane without a next item clamps
        const bool more = inext - lane < n;
        if (!BJJ_K1_LATE_SCALAR && more) { raw[0] = sc4[2 * iload]; raw[1] = sc4[2 * iload + 1]; }
        K1Acc acc;
        Niels cur;
        k1_item_windows(fb, nwin, it, acc, cur, [&]() {
          if (!BJJ_K1_LATE_SCALAR) return;
          if (pending) k1_stash_store(held, stash + iheld * 64, scratch + iheld * 16);
          if (more) { raw[0] = sc4[2 * iload]; raw[1] = sc4[2 * iload + 1]; }  // the next scalar: in flight under this item's windows
        });
        if (more) it = k1_item_begin(fb, W, raw);                               // its first two gathers: under the last addition
        BJJ_SCHED_FENCE();
        const Ext p = k1_madd<false>(acc, cur);   // the last window's addition, T not needed by the epilogue
        // a wave with a next item has this one in every lane (inext - lane < n and lane < nthreads give i < n): its stash is held
        // back; a lane's last item has no wait behind it to hide under and is stored at once
        pending = BJJ_K1_LATE_SCALAR && more;
        if (pending) { k1_stash_pack(held, p, run); iheld = i; }
        else if (i < n) {
          if (BJJ_K1_REG_RECORDS) { k1_stash_pack(held, p, run); k1_stash_store(held, stash + i * 64, scratch + i * 16); }
          else epilogue_stash(p, run, stash + i * 64, scratch + i * 16);
        }
        if (!more) break;
        i = inext;
      }
    }
  } else {
#pragma unroll 1
    for (size_t i = tid; i - lane < n; i += nthreads) {  // wave-uniform trip count: the gathers are cooperative
      const bool valid = i < n;
      u32 sc[8];
      load_w8(scalars + (valid ? i : n - 1) * 32, sc);
      Ext p = fixed_base_mul(fb, W, nwin, sc, c_K);
      if (valid) epilogue_stash(p, run, stash + i * 64, scratch + i * 16);
    }
  }
  if (AHEAD && (BJJ_K1_REG_RECORDS || BJJ_K1_PIPE_RECORD || BJJ_K1_EARLY_RECORD))
    k1_epilogue_run<BLOCK, FORM>(run, n, tid, nthreads, out, stash, scratch, lds);
  else
    epilogue_run<BLOCK, FORM, BJJ_K1_INV_CORE>(run, n, tid, nthreads, out, scratch, lds, xy);
}
// Two shapes of the same kernel:
//  * bjj_k_mul_fixed_base: ONE workgroup of BJJ_K1_BLOCK = 512 lanes per CU (2 waves per SIMD, two staging areas per wave,
//    150 KB of LDS): one workgroup-wide inversion per CU and launch.  Best when launches run one after the other.
//  * bjj_k_mul_fixed_base_2x256: TWO workgroups of 256 lanes per CU (the same 2 waves per SIMD).  Alone it is ~2 % slower (two
//    inversions per CU); but a launch only ever needs ONE of the two workgroup slots of a CU, so when a second launch of
//    the context is in flight (another stream, the other scratch set) the hardware gives each launch one slot per CU, the
//    two run half a period out of phase, and one launch's serial section -- the inversion by one wave while the other waves of
//    its workgroup wait, then the epilogue -- is covered by the other launch's main loop: 1.84 vs 1.75 G mults/s on two streams
//    (profiles/r03_ab_k1_2x256_two_streams.txt).  The host picks the shape per call (bjj_hip.hip: fixed_base_variant).
//    Its grid is ONE workgroup per CU (bjj_hip.hip: fixed_base_lanes): the launch asks only for the slot it would get anyway, so a
//    lane keeps its slot for all of its items -- 16 at 2^20 items on 256 CUs -- and a slot runs one ramp, one running product
//    and one inversion per launch instead of two: +2.3 ... 2.5 % on two streams over the grid of two workgroups per CU, whose
//    second workgroup on every slot repeated all three (profiles/r09_ab_k1_long_lanes.txt; BJJ_K1_OVERLAP_SLOTS=2 gives that
//    grid back).  The kernel is grid-strided and its stash is indexed by item, so the grid is the host's business alone.
__global__ void __launch_bounds__(BJJ_K1_BLOCK, BJJ_K1_MIN_BLOCKS) bjj_k_mul_fixed_base(const u32* __restrict__ table, int W, int nwin,
                                                                  const uint8_t* __restrict__ scalars, size_t n,
                                                                  uint8_t* __restrict__ out, u32* __restrict__ scratch) {
  mul_fixed_base_body<BJJ_K1_BLOCK, BJJ_K1_NBUF>(table, W, nwin, scalars, n, out, scratch);
}
// The signer's constant-time option (bjj_set_signer_constant_time; PrivateKey::public, src/lib.rs:304-306): the multiplication
// through the scanning policy over the context's small 4-bit table -- no address depends on a digit of the scalar.
template <unsigned FORM>
__device__ __forceinline__ void mul_fixed_base_scan_body(const u32* __restrict__ table, int W, const uint8_t* __restrict__ scalars, size_t n,
                                                         uint8_t* __restrict__ out, u32* __restrict__ scratch, uint8_t* __restrict__ xy, int nwin) {
  __shared__ u32 lds[NL * 64];
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nthreads = (size_t)gridDim.x * blockDim.x;
  const GatherScan fb = {table, (u32)fixed_stride(W)};
  Fr run = fr_one();
#pragma unroll 1
  for (size_t i = tid; i < n; i += nthreads) {
    u32 sc[8];
    load_w8(scalars + i * 32, sc);
    Ext p = fixed_base_mul(fb, W, nwin, sc, c_K);
    epilogue_stash(p, run, ((FORM & EPI_COMPRESS) ? xy : out) + i * 64, scratch + i * 16);
  }
  epilogue_run<BJJ_EPI_BLOCK, FORM, BJJ_K1_INV_CORE>(run, n, tid, nthreads, out, scratch, lds, xy);
}
__global__ void __launch_bounds__(BJJ_EPI_BLOCK, 1) bjj_k_mul_fixed_base_scan(const u32* __restrict__ table, int W, int nwin,
                                                                        const uint8_t* __restrict__ scalars, size_t n,
                                                                        uint8_t* __restrict__ out, u32* __restrict__ scratch) {
  mul_fixed_base_scan_body<EPI_AFFINE>(table, W, scalars, n, out, scratch, nullptr, nwin);
}
__global__ void __launch_bounds__(256, 2) bjj_k_mul_fixed_base_2x256(const u32* __restrict__ table, int W, int nwin,
                                                                    const uint8_t* __restrict__ scalars, size_t n,
                                                                    uint8_t* __restrict__ out, u32* __restrict__ scratch) {
  mul_fixed_base_body<256, 2, EPI_AFFINE, true>(table, W, nwin, scalars, n, out, scratch);
}
// ---- the same three kernels with Point::compress fused into the epilogue (src/lib.rs:166-178): 32 bytes per result instead of 64.
// `sk.public().compress()` is what a key server ships, and the host-pointer form of K1 is bound by the copy-out (64 MB of
// affine points per 2^20 items = 1.2 ms of PCIe against 0.6 ms of kernel): half the bytes, and no second pass over the points.
__global__ void __launch_bounds__(BJJ_K1_BLOCK, BJJ_K1_MIN_BLOCKS) bjj_k_mul_fixed_base_c32(const u32* __restrict__ table, int W, int nwin,
                                                                      const uint8_t* __restrict__ scalars, size_t n,
                                                                      uint8_t* __restrict__ out32, u32* __restrict__ scratch,
                                                                      uint8_t* __restrict__ xy) {
  mul_fixed_base_body<BJJ_K1_BLOCK, BJJ_K1_NBUF, EPI_COMPRESS>(table, W, nwin, scalars, n, out32, scratch, xy);
}
__global__ void __launch_bounds__(256, 2) bjj_k_mul_fixed_base_2x256_c32(const u32* __restrict__ table, int W, int nwin,
                                                                        const uint8_t* __restrict__ scalars, size_t n,
                                                                        uint8_t* __restrict__ out32, u32* __restrict__ scratch,
                                                                        uint8_t* __restrict__ xy) {
  mul_fixed_base_body<256, 2, EPI_COMPRESS, true>(table, W, nwin, scalars, n, out32, scratch, xy);
}
__global__ void __launch_bounds__(BJJ_EPI_BLOCK, 1) bjj_k_mul_fixed_base_scan_c32(const u32* __restrict__ table, int W, int nwin,
                                                                            const uint8_t* __restrict__ scalars, size_t n,
                                                                            uint8_t* __restrict__ out32, u32* __restrict__ scratch,
                                                                            uint8_t* __restrict__ xy) {
  mul_fixed_base_scan_body<EPI_COMPRESS>(table, W, scalars, n, out32, scratch, xy, nwin);
}

// ---- launchers (declared in bjj_launch.hpp) ------------------------------------------------------------
namespace bjjk {
int fixed_base_lanes_per_cu(int variant) {   // one grid size serves the affine and the compressed form: the lesser of the two
  return variant ? lanes_for_both(bjj_k_mul_fixed_base_2x256, bjj_k_mul_fixed_base_2x256_c32, 256)
                 : lanes_for_both(bjj_k_mul_fixed_base, bjj_k_mul_fixed_base_c32, BJJ_K1_BLOCK);
}
hipError_t fill_fixed_table(hipStream_t st, u32* table, const u32* bases, int W, int nwin) {
  const size_t entries = fixed_stride(W) * (size_t)nwin;
  // chain length: long enough to amortise the start ladder and the inversion, short enough to fill the GPU
  size_t chain = entries >> 18;
  chain = chain < 4 ? 4 : (chain > 256 ? 256 : chain);
  const size_t chains = ((fixed_stride(W) + chain - 1) / chain) * (size_t)nwin;
  BJJ_LAUNCH(bjj_k_build_fixed_table, dim3((unsigned)((chains + BJJ_BLOCK - 1) / BJJ_BLOCK)), dim3(BJJ_BLOCK), 0, st,
                     table, bases, W, nwin, (u32)chain);
  return hipGetLastError();
}
hipError_t build_fixed_table(hipStream_t st, u32* table, u32* bases, int W, int nwin) {
  BJJ_LAUNCH(bjj_k_fixed_window_bases, dim3((nwin + 63) / 64), dim3(64), 0, st, bases, W, nwin);
  return fill_fixed_table(st, table, bases, W, nwin);
}
hipError_t check_fixed_table(hipStream_t st, int grid, const u32* table, const u32* bases, int W, int nwin,
                             unsigned long long* d_bad) {
  BJJ_LAUNCH(bjj_k_check_fixed_table, dim3((unsigned)grid), dim3(BJJ_BLOCK), 0, st, table, bases, W, nwin, d_bad);
  return hipGetLastError();
}
// xy != nullptr: the compressed form (out = 32-byte records, xy = the 64-byte-per-item stash)
hipError_t mul_fixed_base_scan(hipStream_t st, int cus, const u32* table, int W, int nwin, const uint8_t* scalars, size_t n,
                               uint8_t* out, u32* scratch, uint8_t* xy) {
  const int occ = xy ? occupancy_of(bjj_k_mul_fixed_base_scan_c32, BJJ_EPI_BLOCK) : occupancy_of(bjj_k_mul_fixed_base_scan, BJJ_EPI_BLOCK);
  const int grid = capped_grid(n, BJJ_EPI_BLOCK, (size_t)cus * (size_t)occ);
  if (xy)
    BJJ_LAUNCH(bjj_k_mul_fixed_base_scan_c32, dim3(grid), dim3(BJJ_EPI_BLOCK), 0, st, table, W, nwin, scalars, n, out, scratch, xy);
  else
    BJJ_LAUNCH(bjj_k_mul_fixed_base_scan, dim3(grid), dim3(BJJ_EPI_BLOCK), 0, st, table, W, nwin, scalars, n, out, scratch);
  return hipGetLastError();
}
hipError_t mul_fixed_base(hipStream_t st, int cus, int lanes_per_cu, int variant, const u32* table, int W, int nwin, const uint8_t* scalars,
                          size_t n, uint8_t* out, u32* scratch, uint8_t* xy) {
  const int block = variant ? 256 : BJJ_K1_BLOCK;
  const int grid = capped_grid(n, block, (size_t)cus * (size_t)(lanes_per_cu / block));
  if (xy) {
    if (variant)
      BJJ_LAUNCH(bjj_k_mul_fixed_base_2x256_c32, dim3(grid), dim3(256), 0, st, table, W, nwin, scalars, n, out, scratch, xy);
    else
      BJJ_LAUNCH(bjj_k_mul_fixed_base_c32, dim3(grid), dim3(BJJ_K1_BLOCK), 0, st, table, W, nwin, scalars, n, out, scratch, xy);
  } else if (variant)
    BJJ_LAUNCH(bjj_k_mul_fixed_base_2x256, dim3(grid), dim3(256), 0, st, table, W, nwin, scalars, n, out, scratch);
  else
    BJJ_LAUNCH(bjj_k_mul_fixed_base, dim3(grid), dim3(BJJ_K1_BLOCK), 0, st, table, W, nwin, scalars, n, out, scratch);
  return hipGetLastError();
}
}  // namespace bjjk
