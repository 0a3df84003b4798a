// libbjj_hip.so, kernel unit 12: batched small-range discrete logarithms (include/bjj_hip_dlog.h; bodies: dlog.hpp).
//   bjj_k_dlog_setup: one thread -- Niels(G), Niels(-2^b G), Niels(-2^(b+1) G), the base's canonical record, the order test
//   bjj_k_dlog_build: the baby table, j * G for j = 0 .. 2^b: a lane walks a chain of `chain` consecutive j by mixed additions of
//   G, every step's 1 / Z from the workgroup inversion, and inserts {tag, j + 1} with a 64-bit atomicCAS on the slot
//   bjj_k_dlog_check_entries / bjj_k_dlog_check_slots: every j found again from an independent j * G; the occupied slots counted
//   bjj_k_dlog_search: one item per lane, giant steps s0 .. s1 - 1 of the call; a workgroup inversion per step
#include "k_common.hpp"
#include "dlog.hpp"

// One inversion (one wave) per step is shared by the whole workgroup, and the other waves wait for it: the largest workgroup wins.
// Measured at 2^20 items, 22 baby bits, 32-bit range, one uncut launch: 1024 lanes 115.0 ms, 512 lanes 159.9 ms, 256 lanes
// 169.7 ms -- although 1024 lanes cap the kernel at 128 VGPRs and cost it 100 bytes of scratch per lane.  A/B: EXTRA=-DBJJ_DLOG_BLOCK=...
#ifndef BJJ_DLOG_BLOCK
#define BJJ_DLOG_BLOCK 1024
#endif
// Tag width of a slot.  The library ships 32; tests/devfuzz/dlog.hip compiles this unit again with 3, where false tag hits are the
// rule and confirmation has something to refuse in every search.
#ifndef BJJ_DLOG_TAG_BITS
#define BJJ_DLOG_TAG_BITS 32
#endif

struct DlogSlotsRead {
  const unsigned long long* p;
  __device__ __forceinline__ u64 load(u32 i) const { return (u64)p[i]; }
};
struct DlogSlotsBuild {
  unsigned long long* p;
  __device__ __forceinline__ u64 load(u32 i) const { return (u64)p[i]; }
  __device__ __forceinline__ bool cas(u32 i, u64 v) const { return atomicCAS(p + i, 0ull, (unsigned long long)v) == 0ull; }
};
struct DlogPointArg { u32 xy[16]; };

// use_b8: the base is the generator B8 of the constant block, not the record
__global__ void __launch_bounds__(64) bjj_k_dlog_setup(u32* params, int b, DlogPointArg P, int use_b8) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const Fr bx = use_b8 ? c_K.B8X : fr_to_mont_words(P.xy), by = use_b8 ? c_K.B8Y : fr_to_mont_words(P.xy + 8);
  dlog_setup(params, bx, by, b, c_K);
}
// Thread t owns j = t * chain .. t * chain + chain - 1; a thread whose chain starts past 2^b walks the identity and inserts nothing
// (the workgroup inversion needs every lane at every step).
__global__ void __launch_bounds__(BJJ_DLOG_BLOCK) bjj_k_dlog_build(unsigned long long* slots, u32 mask, const u32* __restrict__ params, int b,
                                                                   u32 chain, unsigned long long* failed) {
  __shared__ u32 lds[NL * 64];
  const u64 entries = dlog_entries(b);
  const u64 j0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) * chain;
  const Niels g = load_niels(params + DLOG_P_G);
  const DlogSlotsBuild S = {slots};
  Ext acc = dlog_mul_small(g, j0 < entries ? j0 : 0, b + 1);
  unsigned long long lost = 0;
#pragma unroll 1
  for (u32 k = 0; k < chain; k++) {
    const Fr zinv = block_invert<BJJ_DLOG_BLOCK, INV_K1>(acc.Z, lds);
    if (j0 + k < entries) lost += dlog_insert<BJJ_DLOG_TAG_BITS>(S, mask, (u32)(j0 + k), acc, zinv) ? 0 : 1;
    acc = ext_madd(acc, g);
  }
  if (lost) atomicAdd(failed, lost);
}
__global__ void __launch_bounds__(BJJ_BLOCK) bjj_k_dlog_check_entries(const unsigned long long* __restrict__ slots, u32 mask,
                                                                      const u32* __restrict__ params, int b, unsigned long long* bad) {
  const u64 entries = dlog_entries(b), nthreads = (u64)gridDim.x * blockDim.x;
  const DlogSlotsRead S = {slots};
  unsigned long long mine = 0;
#pragma unroll 1
  for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < entries; j += nthreads)
    mine += (unsigned long long)dlog_check_entry<BJJ_DLOG_TAG_BITS>(S, mask, params, (u32)j, b, c_K);
  if (mine) atomicAdd(bad, mine);
}
// bad[0] += violated conditions, bad[1] += occupied slots
__global__ void __launch_bounds__(BJJ_BLOCK) bjj_k_dlog_check_slots(const unsigned long long* __restrict__ slots, u32 mask, int b,
                                                                    unsigned long long* bad) {
  const u64 nslots = (u64)mask + 1, nthreads = (u64)gridDim.x * blockDim.x;
  unsigned long long mine = 0, occ = 0;
#pragma unroll 1
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += nthreads) {
    u32 o;
    mine += (unsigned long long)dlog_check_slot((u64)slots[i], b, o);
    occ += o;
  }
  if (mine) atomicAdd(bad, mine);
  if (occ) atomicAdd(bad + 1, occ);
}

// Item i = the lane's global index.  Launches after the first of a cut call (s0 > 0) pass by every item that is decided (its ok is
// not BJJ_DLOG_IN_FLIGHT) and leave its result alone; `last` marks the launch with the call's last step, which turns the marker into 0.  The search loop and the confirmation round are workgroup-uniform: block_invert and the ladder of
// dlog_confirm need every lane.  A lane without work keeps Q = the identity (Z = 1) in the inversion.
__global__ void __launch_bounds__(BJJ_DLOG_BLOCK) bjj_k_dlog_search(const unsigned long long* __restrict__ slots, u32 mask,
                                                                    const u32* __restrict__ params, int b, const uint8_t* __restrict__ pts,
                                                                    size_t n, int range_bits, u32 s0, u32 s1, int last,
                                                                    unsigned long long* __restrict__ out_m, uint8_t* ok) {
  __shared__ u32 lds[NL * 64];
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const DlogSlotsRead S = {slots};
  DlogLane L;
  const bool mine = i < n && dlog_resumes(s0, s0 ? (u32)ok[i] : 0u);
  if (mine) dlog_start(L, pts + i * 64, params, s0, c_K); else dlog_idle(L);
  const Niels ns = load_niels(params + DLOG_P_NEG_STRIDE);
#pragma unroll 1
  for (;;) {
#pragma unroll 1
    while (__syncthreads_or(L.st == DL_SEARCH)) {
      const Fr zinv = block_invert<BJJ_DLOG_BLOCK, INV_K1>(L.Q.Z, lds);
      dlog_step<BJJ_DLOG_TAG_BITS>(L, zinv, ns, S, mask, s1);
    }
    if (!__syncthreads_or(L.st == DL_PENDING)) break;
    dlog_confirm(L, load_niels(params + DLOG_P_G), b, range_bits);
  }
  if (mine) {
    ok[i] = (uint8_t)dlog_ok_byte(L, last != 0);
    out_m[i] = (unsigned long long)L.m;
  }
}

// ---- launchers (declared in bjj_launch.hpp) ------------------------------------------------------------
namespace bjjk {
hipError_t dlog_setup_table(hipStream_t st, uint32_t* params, int b, const uint32_t* xy /* 16 words, NULL = B8 */) {
  DlogPointArg P;
  for (int i = 0; i < 16; i++) P.xy[i] = xy ? xy[i] : 0u;
  BJJ_LAUNCH(bjj_k_dlog_setup, dim3(1), dim3(64), 0, st, params, b, P, xy ? 0 : 1);
  return hipGetLastError();
}
// chain length: one entry per lane up to 2^10 entries, then longer chains, 16 at most (2^22 entries: 256 workgroups)
hipError_t dlog_build_table(hipStream_t st, unsigned long long* slots, const uint32_t* params, int b, unsigned long long* d_failed) {
  const uint64_t entries = dlog_entries(b);
  uint64_t chain = entries >> 10;
  chain = chain < 1 ? 1 : (chain > 16 ? 16 : chain);
  const uint64_t threads = (entries + chain - 1) / chain;
  BJJ_LAUNCH(bjj_k_dlog_build, dim3((unsigned)((threads + BJJ_DLOG_BLOCK - 1) / BJJ_DLOG_BLOCK)), dim3(BJJ_DLOG_BLOCK), 0, st, slots,
             (uint32_t)(dlog_slots(b) - 1), params, b, (uint32_t)chain, d_failed);
  return hipGetLastError();
}
hipError_t dlog_check_table(hipStream_t st, int grid, const unsigned long long* slots, const uint32_t* params, int b, unsigned long long* d_bad2) {
  const uint32_t mask = (uint32_t)(dlog_slots(b) - 1);
  BJJ_LAUNCH(bjj_k_dlog_check_entries, dim3((unsigned)grid), dim3(BJJ_BLOCK), 0, st, slots, mask, params, b, d_bad2);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  BJJ_LAUNCH(bjj_k_dlog_check_slots, dim3((unsigned)grid), dim3(BJJ_BLOCK), 0, st, slots, mask, b, d_bad2);
  return hipGetLastError();
}
hipError_t dlog_search(hipStream_t st, const unsigned long long* slots, const uint32_t* params, int b, const uint8_t* pts, size_t n,
                       int range_bits, uint32_t s0, uint32_t s1, bool last, unsigned long long* out_m, uint8_t* ok) {
  BJJ_LAUNCH(bjj_k_dlog_search, dim3((unsigned)((n + BJJ_DLOG_BLOCK - 1) / BJJ_DLOG_BLOCK)), dim3(BJJ_DLOG_BLOCK), 0, st, slots,
             (uint32_t)(dlog_slots(b) - 1), params, b, pts, n, range_bits, s0, s1, last ? 1 : 0, out_m, ok);
  return hipGetLastError();
}
}  // namespace bjjk
