// Device-side code shared by the kernel translation units (k_*.hip): the constant block, the
// workgroup-wide simultaneous inversion + affine epilogue (K5), and the wave-cooperative gather
// policy of the fixed-base table.  The library is split into one translation unit per kernel
// family so that the ~140 s single-file device compile runs in parallel; every unit carries its
// own (internal-linkage) copy of the 63 KB constant block.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "sign.hpp"
#include "bjj_constants.inc"
#include "bjj_launch.hpp"

using namespace bjj;

// Every launcher returns hipGetLastError() right after its launch.  That call reports the thread's LAST error, which may be a
// stale, harmless one (hipErrorNotReady of an event query): the slate is wiped before the launch so that the
// status a launcher returns is the status of its own launch.
#define BJJ_LAUNCH(...) do { (void)hipGetLastError(); hipLaunchKernelGGL(__VA_ARGS__); } while (0)

static __constant__ Consts c_K = BJJ_CONSTS_INIT;

// ---------------------------------------------------------------------------
// workgroup-wide simultaneous inversion: every thread passes x (Montgomery, != 0,
// < 2r) and receives 1/x.  The workgroup is cut into 64 groups of G = BJJ_EPI_BLOCK/64
// consecutive lanes: prefix and suffix products inside a group by cross-lane shuffles
// (log2 G steps each, no barrier), the 64 group products go through LDS to ONE wave
// whose 64 lanes invert one group product each (binary GCD), and every thread
// finishes with 1/x = (1/group product) * (product of the lanes before it) * (after it).
// CORE selects what the one wave runs: INV_GCD = fr_inv (everyone's default, and their machine code), INV_K1 = fr_inv_k1, the
// shorter division-step core, which K1 (k_fixed.hip) passes through epilogue_run.
// ---------------------------------------------------------------------------
enum : int { INV_GCD = 0, INV_K1 = 1 };
template <int GROUP>
__device__ __forceinline__ Fr fr_shfl_up(const Fr& f, int d) {
  Fr r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.v[i] = __shfl_up(f.v[i], d, GROUP);
  return r;
}
template <int GROUP>
__device__ __forceinline__ Fr fr_shfl_down(const Fr& f, int d) {
  Fr r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.v[i] = __shfl_down(f.v[i], d, GROUP);
  return r;
}
template <int BLOCK, int CORE = INV_GCD>
__device__ Fr block_invert(const Fr& x, u32* lds /* NL * 64 words */) {
  constexpr int GROUP = BLOCK / 64;
  const int t = threadIdx.x, gl = t & (GROUP - 1), grp = t / GROUP;
  Fr pre = x, suf = x;
#pragma unroll 1
  for (int d = 1; d < GROUP; d <<= 1) {  // inclusive prefix / suffix products inside the group
    Fr yp = fr_shfl_up<GROUP>(pre, d), ys = fr_shfl_down<GROUP>(suf, d);
    pre = fr_mul(pre, fr_select(gl >= d, yp, fr_one()));
    suf = fr_mul(suf, fr_select(gl + d < GROUP, ys, fr_one()));
  }
  Fr epre = fr_select(gl > 0, fr_shfl_up<GROUP>(pre, 1), fr_one());                    // exclusive versions
  Fr esuf = fr_select(gl + 1 < GROUP, fr_shfl_down<GROUP>(suf, 1), fr_one());
  if (gl == GROUP - 1) {
#pragma unroll
    for (int i = 0; i < NL; i++) lds[i * 64 + grp] = pre.v[i];  // limb-major: conflict-free
  }
  __syncthreads();
  // the inverting wave rotates with the workgroup index so that co-resident workgroups do not queue on one SIMD
  if ((t >> 6) == (int)((blockIdx.x + (blockIdx.x >> 8)) % (BLOCK / 64))) {
    const int l = t & 63;
    Fr tot;
#pragma unroll
    for (int i = 0; i < NL; i++) tot.v[i] = lds[i * 64 + l];
    Fr inv = CORE == INV_K1 ? fr_inv_k1(tot) : fr_inv(tot);
#pragma unroll
    for (int i = 0; i < NL; i++) lds[i * 64 + l] = inv.v[i];
  }
  __syncthreads();
  Fr ginv;
#pragma unroll
  for (int i = 0; i < NL; i++) ginv.v[i] = lds[i * 64 + grp];
  __syncthreads();
  return fr_mul(fr_mul(ginv, epre), esuf);
}

// Phase-1 record for the affine epilogue: X, Y (as 2 x 32-byte integers) go to `xy_item` -- the item's final output slot when the
// result is the 64-byte affine point, a slot of the scratch set's XY area when the result is the 32-byte compressed point
// (EPI_COMPRESS) -- Z and the lane's running prefix product go to scratch.
__device__ __forceinline__ void epilogue_stash(const Ext& p, Fr& run, uint8_t* xy_item, u32* scr_item) {
  u32 w[8];
  fr_to_words(p.X, w); store_w8(xy_item, w);
  fr_to_words(p.Y, w); store_w8(xy_item + 32, w);
  fr_to_words(p.Z, w); store_w8(scr_item, w);
  fr_to_words(run, w); store_w8(scr_item + 8, w);
  run = fr_mul(run, p.Z);
}
// An item this launch does NOT finish (EPI_SKIPPABLE kernels; K2: the point is off the curve, the exact kernel K6 owns the item's
// output slot and may be writing it while this launch runs): Z = 0 marks it -- the Z of a computed point is never 0 -- and the
// running product passes it by.  Nothing is written to the output slot, neither here nor in phase 2.
__device__ __forceinline__ void epilogue_stash_skipped(u32* scr_item) {
  const u32 z[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  store_w8(scr_item, z);
}
// Epilogue forms (template flags; the default -- affine output, no skipped items -- is what K1 and the signer use, and its code
// does not change when the other forms are instantiated next to it)
//   EPI_STASH_APART: the affine form with the phase-1 stash in `xy` when that is given (run time) instead of in the output slots -- for
//   an output array that must be written exactly once and never read: the caller's pinned HOST memory behind its device mapping
enum : unsigned { EPI_AFFINE = 0u, EPI_COMPRESS = 1u, EPI_SKIPPABLE = 2u, EPI_STASH_APART = 4u };
// Phase-2: given inv = 1 / (product of this lane's Z_0..Z_i) as a PLAIN (non-Montgomery) integer, finish item i
// and step inv down to 1 / (Z_0..Z_{i-1}).  A Montgomery product of a plain and a Montgomery operand is the plain
// product, so Y * (1/Z) lands directly on the canonical output integer.  Output: reference-curve (x, y), or with EPI_COMPRESS
// Point::compress of it (src/lib.rs:166-178: y as 32 little-endian bytes, bit 255 set when x > Q >> 1) -- x is canonical right
// here, so the sign costs one comparison instead of a second pass over 64-byte points.
template <unsigned FORM = EPI_AFFINE>
__device__ __forceinline__ void epilogue_finish(Fr& inv, uint8_t* out_item, uint8_t* xy_item, const u32* scr_item) {
  constexpr u32 R1[NL] = {BJJ_N0, BJJ_N1, BJJ_N2, BJJ_N3, BJJ_N4, BJJ_N5, BJJ_N6, BJJ_N7, BJJ_N8};
  u32 w[8];
  load_w8(scr_item, w);
  if (FORM & EPI_SKIPPABLE) {
    if ((w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) == 0u) return;
  }
  Fr Z = fr_from_words(w);
  load_w8(scr_item + 8, w); Fr P = fr_from_words(w);
  load_w8(xy_item, w);      Fr X = fr_from_words(w);
  load_w8(xy_item + 32, w); Fr Y = fr_from_words(w);
  Fr zinv = fr_mul(inv, P);               // plain 1/Z
  inv = fr_mul(inv, Z);
  Fr c2 = fr_mul(zinv, c_K.FINV);         // plain 1/(Z F): maps x' back to the reference curve
  Fr x = fr_cond_sub_kr(fr_mul(X, c2), R1);
  Fr y = fr_cond_sub_kr(fr_mul(Y, zinv), R1);
  if (FORM & EPI_COMPRESS) {
    fr_to_words(y, w);
    if (plain_gt_halfq(x, c_K)) w[7] |= 0x80000000u;
    store_w8(out_item, w);
  } else {
    fr_to_words(x, w); store_w8(out_item, w);
    fr_to_words(y, w); store_w8(out_item + 32, w);
  }
}
// out: 64 bytes per item (32 with EPI_COMPRESS); xy: where phase 1 stashed X, Y, 64 bytes per item (== out for the affine form)
template <int BLOCK = BJJ_EPI_BLOCK, unsigned FORM = EPI_AFFINE, int CORE = INV_GCD>
__device__ __forceinline__ void epilogue_run(Fr run, size_t n, size_t tid, size_t nthreads, uint8_t* out, u32* scratch,
                                             u32* lds, uint8_t* xy = nullptr) {
  Fr inv = fr_mul(block_invert<BLOCK, CORE>(run, lds), fr_one_plain());  // out of Montgomery form once per lane
  if (tid >= n) return;
  size_t cnt = (n - tid + nthreads - 1) / nthreads;
#pragma unroll 1
  for (size_t m = cnt; m-- > 0;) {
    size_t i = tid + m * nthreads;
    if (FORM & EPI_COMPRESS) epilogue_finish<FORM>(inv, out + i * 32, xy + i * 64, scratch + i * 16);
    else if (FORM & EPI_STASH_APART) epilogue_finish<FORM>(inv, out + i * 64, (xy ? xy : out) + i * 64, scratch + i * 16);
    else epilogue_finish<FORM>(inv, out + i * 64, out + i * 64, scratch + i * 16);
  }
}

// Wave-cooperative gather straight into LDS (policy interface: bjj_device.hpp "gather policies").
// A lane-private gather costs 7 load instructions x 64 lanes, every lane in its own 128-byte line and, for tables beyond
// the TLB reach, its own page: measured alone (tools/ubench/gather_bench.hip) that pattern sustains 12.7 G gathers/s on a
// 5.9 GB table and 10.8 G/s on 155 GB, the one used here 48 and 46 G/s.  Load instruction k of a wave fetches the 8 FULL
// lines of the entries owned by lanes 8k .. 8k+7: lane L moves one 16-byte chunk of the entry of lane e = 8k + L/8, whose slot
// number it obtains by a cross-lane read, with global_load_lds_dwordx4 (no VGPR staging; LDS address = M0 + 16 L), so an
// instruction touches 8 lines, each exactly once.  Chunk c of entry e lands at position c ^ ((e >> 1) & 7) of the entry's
// 128-byte LDS row, which makes the read-back of one's own entry (7 x ds_read_b128, lane stride 128 B) bank-conflict free.
// hipcc does not track LDS-DMA completion, hence the explicit s_waitcnt.  ALL 64 lanes of the wave must call issue/finish
// together (cross-lane reads).  NBUF = 2 staging areas per wave let two gathers be in flight (the start of a fresh
// multiplication in K1); with NBUF = 1 the loops still overlap gather j+1 with addition j, whose entry is in registers by then.
#define FB_STAGE_WORDS (64 * NIELS_WORDS)   // 8 KB: one staged entry per lane
// Cache policy of the gather's LDS-DMA loads: the cache-policy immediate of the builtin (gfx940+: sc0 = 1, nt = 2, sc1 = 16).
// A table line is read once per launch by construction.  K1 (NBUF = 2) loads it non-temporal: +1.4 ... 2.2 % on two streams, all
// of it sustained clock under the power cap; sc1 / sc0 sc1 add nothing (profiles/r07_ab_k1_gather_policy.txt).
// The NBUF = 1 users (verify, sign) have their own knob and keep the default policy: not measured with another one.
#ifndef BJJ_GATHER_AUX
#define BJJ_GATHER_AUX 2
#endif
#ifndef BJJ_GATHER_AUX_NBUF1
#define BJJ_GATHER_AUX_NBUF1 0
#endif
// STRIP (K1's overlap form only; every other user keeps its code): the eight slot numbers a lane needs per gather come from
// a 256-byte wave-private strip behind the wave's staging areas -- one ds_write_b32 and two ds_read_b128 -- instead of eight
// ds_bpermute_b32.  The slot of lane j sits at word (j & 7) * 8 + (j >> 3), so the slots of the entries 8k + L/8, k = 0 .. 7,
// of which lane L moves a chunk each, are the eight consecutive words from (L / 8) * 8.  The strip is rewritten by every
// gather; a wave's LDS operations complete in the order they were issued, so the reads of the gather before are done when
// the write lands, and the reads below follow the write: the compiler's own lgkmcnt waits order the rest.  No barrier.
// BJJ_K1_ADDR_MAD (the STRIP instantiation only): a load's address slot * 128 + (table + 16 c) is ONE v_mad_u64_u32 per load.
// The compiler forms it with a 64-bit shift and a 64-bit add, two quarter-rate instructions (a shift by 7 does not fit the
// fused shift-add).  The chunk c = (L & 7) ^ ((e >> 1) & 7) of entry e = 8k + L / 8 is (L & 7) ^ (L >> 4) for even k and that
// value ^ 4 for odd k ((e >> 1) & 7 = (4k + (L >> 4)) & 7 and L >> 4 < 4), so two per-lane 64-bit bases serve the eight loads.
// One asm statement: every statement costs a padding s_nop (fr.hpp).
#ifndef BJJ_K1_ADDR_MAD
#define BJJ_K1_ADDR_MAD 1
#endif
#define FB_STRIP_WORDS 64
template <int NBUF, bool STRIP = false>
struct GatherCoopLds {
  struct Pending {};
  static constexpr int kBuffers = NBUF;
  const u32* table;
  u32* wlds;   // this wave's staging area (STRIP: NBUF areas, then the slot strip)
  int lane;
  __device__ __forceinline__ void strip_slots(u32 slot, u32 (&s)[8]) const {
    u32* const strip = wlds + NBUF * FB_STAGE_WORDS;
    strip[(lane & 7) * 8 + (lane >> 3)] = slot;
    const U4 lo = ((const U4*)strip)[(lane >> 3) * 2], hi = ((const U4*)strip)[(lane >> 3) * 2 + 1];
    s[0] = lo.x; s[1] = lo.y; s[2] = lo.z; s[3] = lo.w; s[4] = hi.x; s[5] = hi.y; s[6] = hi.z; s[7] = hi.w;
  }
  // all 64 lanes run together under this policy: wave-wide maximum (butterfly over the lanes)
  static __device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
  }
  __device__ __forceinline__ void issue(size_t slot, Pending&, int buf) const {
    u32 ss[8];
    if (STRIP) strip_slots((u32)slot, ss);
#if BJJ_K1_ADDR_MAD
    if constexpr (STRIP) {
      const u32 c0 = (u32)((lane & 7) ^ (lane >> 4));
      const u64 b0 = (u64)(uintptr_t)table + c0 * 16u, b1 = (u64)(uintptr_t)table + (c0 ^ 4u) * 16u;
      u64 a[8];
      asm("v_mad_u64_u32 %0, vcc, %8, %16, %17\n\tv_mad_u64_u32 %1, vcc, %9, %16, %18\n\t"
          "v_mad_u64_u32 %2, vcc, %10, %16, %17\n\tv_mad_u64_u32 %3, vcc, %11, %16, %18\n\t"
          "v_mad_u64_u32 %4, vcc, %12, %16, %17\n\tv_mad_u64_u32 %5, vcc, %13, %16, %18\n\t"
          "v_mad_u64_u32 %6, vcc, %14, %16, %17\n\tv_mad_u64_u32 %7, vcc, %15, %16, %18"
          : "=&v"(a[0]), "=&v"(a[1]), "=&v"(a[2]), "=&v"(a[3]), "=&v"(a[4]), "=&v"(a[5]), "=&v"(a[6]), "=&v"(a[7])
          : "v"(ss[0]), "v"(ss[1]), "v"(ss[2]), "v"(ss[3]), "v"(ss[4]), "v"(ss[5]), "v"(ss[6]), "v"(ss[7]),
            "s"(NIELS_WORDS * 4u), "v"(b0), "v"(b1)
          : "vcc");
#pragma unroll
      for (int k = 0; k < 8; k++)
        __builtin_amdgcn_global_load_lds((const u32*)(uintptr_t)a[k],
                                         (__attribute__((address_space(3))) void*)(wlds + (NBUF > 1 ? buf : 0) * FB_STAGE_WORDS + k * (8 * NIELS_WORDS)),
                                         16, 0, NBUF > 1 ? BJJ_GATHER_AUX : BJJ_GATHER_AUX_NBUF1);
      return;
    }
#endif
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int e = 8 * k + (lane >> 3);
      const u32 s = STRIP ? ss[k] : (u32)__shfl((int)(u32)slot, e, 64);
      const int c = (lane & 7) ^ ((e >> 1) & 7);
      __builtin_amdgcn_global_load_lds(table + (size_t)s * NIELS_WORDS + c * 4,
                                       (__attribute__((address_space(3))) void*)(wlds + (NBUF > 1 ? buf : 0) * FB_STAGE_WORDS + k * (8 * NIELS_WORDS)),
                                       16, 0, NBUF > 1 ? BJJ_GATHER_AUX : BJJ_GATHER_AUX_NBUF1);
    }
  }
  __device__ __forceinline__ Niels finish(Pending&, int buf) const {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const U4* q = (const U4*)(wlds + (NBUF > 1 ? buf : 0) * FB_STAGE_WORDS + lane * NIELS_WORDS);
    const int x = (lane >> 1) & 7;
    const U4 a = q[0 ^ x], b = q[1 ^ x], c = q[2 ^ x], d = q[3 ^ x], e = q[4 ^ x], f = q[5 ^ x], h = q[6 ^ x];
    Niels n;
    n.ymx = Fr{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x}};
    n.ypx = Fr{{c.y, c.z, c.w, d.x, d.y, d.z, d.w, e.x, e.y}};
    n.t2d = Fr{{e.z, e.w, f.x, f.y, f.z, f.w, h.x, h.y, h.z}};
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the rows are free again before the next issue overwrites them
    return n;
  }
};

#include "slot_queue.hpp"   // per-XCD rings of free table slots (verify groups, K2 tiles)
