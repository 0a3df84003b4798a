// libbjj_hip.so, kernel unit 14: one scalar, many points -- bjj_mul_common, bjj_in_subgroup, the first launch of bjj_elgamal_decrypt
// (bodies, the recoding and the form rule: common_scalar.hpp).  K2's tile shape: 256-lane workgroups, one item per lane, the
// workgroup-wide simultaneous inversion of k_common.hpp; the table form takes its per-lane tables from K2's slot queue.
// per-lane table entries of this unit: K2's packed layout (bjj_device.hpp "per-lane variable-base table")
#define BJJ_PNIELS_LAYOUT 1
#include "k_common.hpp"
#include "common_scalar.hpp"

// Workgroup size / resident workgroups per CU: K2's, whose slot queue holds one slot per workgroup K2 can have resident.
#define BJJ_CS_BLOCK 256
#define BJJ_CS_MIN_BLOCKS 3
static_assert(BJJ_CS_BLOCK == 256, "the slot of a tile is the tables of one 256-lane workgroup (bjjk::var_base_block)");

enum : int { CS_EPI_POINT = 0, CS_EPI_SUBGROUP = 1, CS_EPI_DECRYPT = 2 };

// One template for both forms and the three epilogues:
//   CS_EPI_POINT     out[i] = canonical affine bytes through epilogue_stash / epilogue_run, ok[i] = 1; an off-curve item writes (0, 0)
//                    and ok[i] = 2, and is passed by in the inversion (epilogue_stash_skipped: the running product never sees it)
//   CS_EPI_SUBGROUP  ok[i] = 1 when the product is the identity, projectively, 0 when it is not, 2 off the curve; no inversion, no out
//   CS_EPI_DECRYPT   the point epilogue without the ok store (the logarithm that follows reports (0, 0) itself)
// D travels by value in the kernel arguments.  Lanes past n take no item but reach every barrier, as in var_base_body.
template <bool TABLE, int EPI, bool ADD>
__global__ void __launch_bounds__(BJJ_CS_BLOCK, BJJ_CS_MIN_BLOCKS) bjj_k_mul_common(const CsDigits D, const uint8_t* __restrict__ pts,
    const uint8_t* __restrict__ add, size_t n, uint8_t* __restrict__ out, uint8_t* __restrict__ ok, u32* __restrict__ scratch,
    u32* __restrict__ vb_tables, u32* __restrict__ slotq, u32 cap_nx) {
  __shared__ u32 lds[NL * 64];
  __shared__ u32 sh_slot;
  u32* q = nullptr;
  u32* tbl = nullptr;
  u32 slot = 0;
  if (TABLE) {
    q = slot_queue_of_this_xcd(slotq, cap_nx);
    if (threadIdx.x == 0) sh_slot = slot_pop_one(q, cap_nx);
    __syncthreads();
    slot = sh_slot;
    tbl = vb_tables + ((size_t)slot * BJJ_CS_BLOCK + threadIdx.x) * VB_TABLE_WORDS;
  }
  const size_t base = (size_t)blockIdx.x * BJJ_CS_BLOCK;
  const size_t hi = base + BJJ_CS_BLOCK < n ? base + BJJ_CS_BLOCK : n;
  const size_t i = base + threadIdx.x;
  Fr run = fr_one();
  if (i < hi) {
    Ext p;
    const bool on = cs_item<TABLE, ADD>(pts, add, i, D, tbl, p, c_K);
    if (EPI == CS_EPI_SUBGROUP) {
      ok[i] = on ? (cs_is_identity(p) ? (uint8_t)1 : (uint8_t)0) : (uint8_t)2;
    } else if (on) {
      epilogue_stash(p, run, out + i * 64, scratch + i * 16);
      if (EPI == CS_EPI_POINT) ok[i] = 1;
    } else {
      const u32 z[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
      epilogue_stash_skipped(scratch + i * 16);
      store_w8(out + i * 64, z);
      store_w8(out + i * 64 + 32, z);
      if (EPI == CS_EPI_POINT) ok[i] = 2;
    }
  }
  if (TABLE) {   // the tables are done with: every wave's stores acknowledged before the barrier, the push behind it
    slot_release_wave();
    __syncthreads();
    if (threadIdx.x == 0) slot_push_one(q, cap_nx, slot);
  }
  if (EPI != CS_EPI_SUBGROUP) epilogue_run<BJJ_CS_BLOCK, EPI_SKIPPABLE>(run, hi, i, (size_t)BJJ_CS_BLOCK, out, scratch, lds);
}

namespace bjjk {
// resident workgroups per CU of the table form: the least over its instantiations (they share K2's slot queue)
int common_scalar_table_blocks_per_cu() {
  const int a = occupancy_of(bjj_k_mul_common<true, CS_EPI_POINT, false>, BJJ_CS_BLOCK), b = occupancy_of(bjj_k_mul_common<true, CS_EPI_POINT, true>, BJJ_CS_BLOCK),
            c = occupancy_of(bjj_k_mul_common<true, CS_EPI_SUBGROUP, false>, BJJ_CS_BLOCK), d = occupancy_of(bjj_k_mul_common<true, CS_EPI_DECRYPT, true>, BJJ_CS_BLOCK);
  const int ab = a > b ? a : b, cd = c > d ? c : d;
  return ab > cd ? ab : cd;   // the most any of them can have resident: what the queue must cover
}
template <bool TABLE, int EPI, bool ADD>
static hipError_t cs_launch(hipStream_t st, const CsDigits& D, const uint8_t* pts, const uint8_t* add, size_t n, uint8_t* out, uint8_t* ok,
                            u32* scratch, u32* vb_tables, u32* slotq, u32 slot_cap) {
  const size_t tiles = (n + BJJ_CS_BLOCK - 1) / BJJ_CS_BLOCK;
  BJJ_LAUNCH((bjj_k_mul_common<TABLE, EPI, ADD>), dim3((unsigned)(tiles ? tiles : 1)), dim3(BJJ_CS_BLOCK), 0, st, D, pts, add, n, out, ok, scratch,
             vb_tables, slotq, slot_cap);
  return hipGetLastError();
}
template <bool TABLE>
static hipError_t cs_launch_form(hipStream_t st, int epi, const CsDigits& D, const uint8_t* pts, const uint8_t* add, size_t n, uint8_t* out,
                                 uint8_t* ok, u32* scratch, u32* vb_tables, u32* slotq, u32 slot_cap) {
  if (epi == COMMON_SUBGROUP) return cs_launch<TABLE, CS_EPI_SUBGROUP, false>(st, D, pts, nullptr, n, nullptr, ok, nullptr, vb_tables, slotq, slot_cap);
  if (epi == COMMON_DECRYPT) {
    if (!add) return hipErrorInvalidValue;
    return cs_launch<TABLE, CS_EPI_DECRYPT, true>(st, D, pts, add, n, out, nullptr, scratch, vb_tables, slotq, slot_cap);
  }
  if (add) return cs_launch<TABLE, CS_EPI_POINT, true>(st, D, pts, add, n, out, ok, scratch, vb_tables, slotq, slot_cap);
  return cs_launch<TABLE, CS_EPI_POINT, false>(st, D, pts, nullptr, n, out, ok, scratch, vb_tables, slotq, slot_cap);
}
hipError_t mul_common(hipStream_t st, int form, int epi, const bjj::CsDigits& D, const uint8_t* pts, const uint8_t* add, size_t n, uint8_t* out,
                      uint8_t* ok, uint32_t* scratch, uint32_t* vb_tables, uint32_t* slotq, uint32_t slot_cap) {
  if (form == CS_FORM_TABLE) return cs_launch_form<true>(st, epi, D, pts, add, n, out, ok, scratch, vb_tables, slotq, slot_cap);
  return cs_launch_form<false>(st, epi, D, pts, add, n, out, ok, scratch, vb_tables, slotq, slot_cap);
}
}  // namespace bjjk
