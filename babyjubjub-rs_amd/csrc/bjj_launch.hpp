// Interface between the host side of libbjj_hip.so (bjj_hip.hip: contexts + the extern "C" boundary) and its kernel
// translation units (k_*.hip).  Plain pointers and sizes only; every launcher enqueues on `st` and returns the launch status.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define BJJ_BLOCK 256
// Workgroup size of the kernels that end in the shared-inversion epilogue: one binary-GCD
// inversion (executed by one wave) is amortised over the whole workgroup.
#define BJJ_EPI_BLOCK 512

// Workgroup size of the verify kernels.  Their waves never cooperate beyond the wave (per-wave staging rows, atomic work
// cursors), so a workgroup is ONE wave: a wave that runs out of work retires its slot at once instead of waiting for the
// slowest of four, which is what lets the head of the next launch (second scratch set, second stream) fill a tail round.
#ifndef BJJ_VERIFY_BLOCK
#define BJJ_VERIFY_BLOCK 64
#endif

namespace bjj { struct BasesArgs; }   // bases.hpp: the per-base descriptors of bjj_k_mul_bases
namespace bjj { struct SignerArgs; }  // signer.hpp: the two tables and the point of bjj_k_verify_signer
namespace bjj { struct SetArgs; }     // signer_set.hpp: the set's tables and keys, the B8 table (bjj_k_verify_set)
namespace bjj { struct ElgamalArgs; } // elgamal.hpp: the three chains and the input arrays of bjj_k_elgamal_encrypt
namespace bjj { struct CsDigits; }    // common_scalar.hpp: the recoded scalar of bjj_k_mul_common, by value in the kernel arguments
namespace bjj { struct PairArgs; struct DleqVerifyArgs; struct DleqRespondArgs; }   // dleq.hpp: the arrays and tables of the k_dleq.hip kernels

namespace bjjk {

template <typename K>
static inline int occupancy_of(K kernel, int block) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block, 0) != hipSuccess || nb < 1) nb = 1;
  return nb;
}
// resident lanes per CU that serve BOTH of two kernels of one workgroup size: one grid size is computed for the pair
template <typename Ka, typename Kb>
static inline int lanes_for_both(Ka a, Kb b, int block) {
  const int oa = occupancy_of(a, block), ob = occupancy_of(b, block);
  return (oa < ob ? oa : ob) * block;
}
// workgroups of a grid-strided launch over n items: one per `block` items, at least one (n = 0), at most the `cap` resident ones
static inline int capped_grid(size_t n, int block, size_t cap) {
  const size_t want = (n + block - 1) / block;
  return (int)(want < cap ? (want ? want : 1) : cap);
}

// resident workgroups per CU -- resident LANES per CU for K1 / K2 (queried on the current device)
int fixed_base_lanes_per_cu(int variant);   // variant 0: one 512-lane workgroup per CU, 1: two 256-lane workgroups
int var_base_lanes_per_cu();
int var_base_block();
int occ_point_add();
int occ_poseidon5();
int occ_decompress();
int occ_verify();           // resident verify WAVES per CU
int probe_xccs(hipStream_t st, uint32_t* d_word);   // number of XCDs of the current device (0 on error)
int occ_verify_scan();      // resident scan WAVES per CU
int verify_scan_block();
int occ_sign();
int occ_sign_schnorr();

// k_fixed.hip
hipError_t build_fixed_table(hipStream_t st, uint32_t* table, uint32_t* bases, int W, int nwin);
hipError_t check_fixed_table(hipStream_t st, int grid, const uint32_t* table, const uint32_t* bases, int W, int nwin,
                             unsigned long long* d_bad);
// the second half of build_fixed_table alone: every entry from the window bases P_j already in `bases` (any base point)
hipError_t fill_fixed_table(hipStream_t st, uint32_t* table, const uint32_t* bases, int W, int nwin);
// xy == nullptr: out = 64-byte affine points; xy != nullptr: out = 32-byte Point::compress records, xy = 64 B / item of stash
hipError_t mul_fixed_base(hipStream_t st, int cus, int lanes_per_cu, int variant, const uint32_t* table, int W, int nwin,
                          const uint8_t* scalars, size_t n, uint8_t* out, uint32_t* scratch, uint8_t* xy = nullptr);
hipError_t mul_fixed_base_scan(hipStream_t st, int cus, const uint32_t* table, int W, int nwin, const uint8_t* scalars, size_t n,
                               uint8_t* out, uint32_t* scratch, uint8_t* xy = nullptr);   // constant-time form over the small 4-bit table
// k_var.hip (sc_words: 32-bit words per scalar record, 8 for the 32-byte form)
// K2 (slow != nullptr: appends the off-curve items it skips; nullptr: they are on somebody else's list), the on-curve scan that makes
// such a list, and K6 over a list (patch: compact results beside the indices instead of the items' own slots; seen: host word <- count)
hipError_t mul_var_base_main(hipStream_t st, int cus, int lanes_per_cu, int variant, const uint8_t* pts, const uint8_t* scalars, int sc_words, size_t n,
                             uint8_t* out, uint32_t* scratch, uint32_t* vb_tables, uint32_t* slow, uint32_t* slotq, uint32_t slot_cap,
                             uint8_t* xy = nullptr);   // xy: phase-1 stash apart from `out` (which may then be mapped host memory)
hipError_t var_base_list_reset(hipStream_t st, uint32_t* list);
hipError_t var_base_scan(hipStream_t st, int grid, const uint8_t* pts, size_t first, size_t end, uint32_t* list);
hipError_t mul_var_base_exact(hipStream_t st, int grid_exact, const uint8_t* pts, const uint8_t* scalars, int sc_words, uint8_t* out,
                              const uint32_t* slow, uint8_t* patch, uint32_t* seen);
int occ_var_base_scan();
// k_small.hip: four lanes per item, for calls that do not fill the chip one item per lane (32-byte scalars); slow as for mul_var_base_main
// ... Poseidon with six lanes per hash, and the bulk of verify with eight lanes per signature (scan and exact launch: k_verify.hip)
hipError_t verify_small(hipStream_t st, bool schnorr, const uint32_t* table, int W, int nwin, const uint8_t* pk, const uint8_t* rb8, const uint8_t* s, const uint8_t* msg,
                        size_t n, uint8_t* ok);
hipError_t mul_fixed_base_quad(hipStream_t st, const uint32_t* table, int W, int nwin, const uint8_t* scalars, size_t n, uint8_t* out, bool compressed);   // B8.mul_scalar, four lanes per item
hipError_t sign_small(hipStream_t st, const uint32_t* table, int W, int nwin, const uint8_t* keys, const uint8_t* msgs, size_t n, uint8_t* out_r, uint8_t* out_s,
                      uint8_t* ok);   // PrivateKey::sign, eight lanes per signature (out_s == nullptr: compressed records)
hipError_t poseidon5_coop(hipStream_t st, const uint8_t* in, size_t n, uint8_t* out);
hipError_t mul_var_base_quad(hipStream_t st, const uint8_t* pts, const uint8_t* scalars, size_t n, uint8_t* out, uint32_t* slow);
hipError_t point_add(hipStream_t st, int grid, const uint8_t* p, const uint8_t* q, size_t n, uint8_t* out);
hipError_t proj_add(hipStream_t st, int grid, const uint8_t* p, const uint8_t* q, size_t n, uint8_t* out);
hipError_t proj_affine(hipStream_t st, int grid, const uint8_t* p, size_t n, uint8_t* out);
// k_hash_codec.hip
hipError_t poseidon5(hipStream_t st, int grid, const uint8_t* in, size_t n, uint8_t* out);
hipError_t compress_points(hipStream_t st, int grid, const uint8_t* in_xy, size_t n, uint8_t* out);
hipError_t decompress_points(hipStream_t st, int grid, const uint8_t* in, size_t stride, size_t n, uint8_t* out_xy, uint8_t* ok,
                             uint8_t* out_s);
hipError_t merge_codec_flags(hipStream_t st, int grid, uint8_t* ok, const uint8_t* f_pk, const uint8_t* f_r, size_t n);
hipError_t scalar_keys(hipStream_t st, int grid, const uint8_t* keys, size_t n, uint8_t* out);
// k_verify.hip
hipError_t verify_scan(hipStream_t st, int grid_scan, const uint8_t* pk, const uint8_t* rb8, const uint8_t* msg, size_t n, uint32_t* wl);
hipError_t verify_list_reset(hipStream_t st, uint32_t* wl);
hipError_t verify_scan_range(hipStream_t st, int grid_scan, const uint8_t* pk, const uint8_t* rb8, const uint8_t* msg, size_t first, size_t end,
                             uint32_t* wl);
enum { VERIFY_BOTH = 0, VERIFY_BULK = 1, VERIFY_EXACT = 2 };   // which workgroups of the one-group-per-workgroup form a launch holds
hipError_t verify_main(hipStream_t st, int mode, int grid, bool schnorr, const uint32_t* table, int W, int nwin, const uint8_t* pk,
                       const uint8_t* rb8, const uint8_t* s, const uint8_t* msg, size_t n, uint8_t* ok, uint32_t* vb_tables,
                       uint32_t* wl, uint32_t* slotq, uint32_t slot_cap, int part = VERIFY_BOTH);
// k_sign.hip
hipError_t sign(hipStream_t st, int grid, const uint32_t* table, int W, int nwin, const uint8_t* keys, const uint8_t* msgs, size_t n,
                uint8_t* out_r, uint8_t* out_s, uint8_t* ok);
hipError_t sign_schnorr(hipStream_t st, int grid, const uint32_t* table, int W, int nwin, const uint8_t* keys, const uint8_t* msgs,
                        const uint8_t* nonces, size_t n, uint8_t* out_r, uint8_t* out_s, uint8_t* ok);
// the same with the scanning (constant-time) gather policy over the small 4-bit table; ct = true in the occupancy queries
hipError_t sign_ct(hipStream_t st, int grid, const uint32_t* table, int W, int nwin, const uint8_t* keys, const uint8_t* msgs, size_t n,
                   uint8_t* out_r, uint8_t* out_s, uint8_t* ok);
hipError_t sign_schnorr_ct(hipStream_t st, int grid, const uint32_t* table, int W, int nwin, const uint8_t* keys, const uint8_t* msgs,
                           const uint8_t* nonces, size_t n, uint8_t* out_r, uint8_t* out_s, uint8_t* ok);
int occ_sign_ct();
int occ_sign_schnorr_ct();
// k_msm.hip: bjj_msm -- Q = sum k_i P_i (Pippenger, msm.hpp).  The scratch of one call is ONE device block laid out by msm_layout
// (byte offsets, 256-B aligned); `status` is the caller's int64 word (-1, or the smallest index of an off-curve point), `out` 64 bytes.
struct MsmLayout {
  int c, W, levels;
  uint32_t S1, G;
  uint64_t keys, records, slices1, nb;
  size_t o_niels, o_red, o_counts, o_cursor, o_bsum, o_total, o_status, o_out, o_rec, o_e0, o_e1, o_buckets, o_w0, o_w1, bytes;
  size_t m;               // segments (bjj_msm: 1)
  uint64_t nwin;          // m * W: the "windows" of the key space
  size_t o_offsets, o_flag, o_seg;   // batched form: the host form's copy of the offsets, the offsets-are-bad word, a segment word per item
};
MsmLayout msm_layout(size_t n, int c);
hipError_t msm(hipStream_t st, const MsmLayout& L, const uint8_t* pts, const uint8_t* scalars, size_t n, uint8_t* scratch, uint8_t* out,
               unsigned long long* status);
// the stages between the two key-forming passes and after them, shared with the batched form (they never look inside a key)
hipError_t msm_scan(hipStream_t st, const MsmLayout& L, uint8_t* scratch);
hipError_t msm_reduce(hipStream_t st, const MsmLayout& L, uint8_t* scratch, const uint32_t** wsum);
// k_msm_batch.hip: bjj_msm_batch -- m sums over the CSR segments offsets[0 .. m] of one point / scalar array; key = (s W + j) B + |d| - 1.
// `offsets`: m + 1 uint64 on the device; `out`: m * 64 bytes; `status`: m int64 words (-1, the smallest off-curve index of the
// segment as a position in the whole array, or -2 everywhere when the offsets break their contract).  m >= 1.
MsmLayout msm_batch_layout(size_t n, size_t m, int c);
hipError_t msm_batch(hipStream_t st, const MsmLayout& L, const uint8_t* pts, const uint8_t* scalars, size_t n, const uint64_t* offsets,
                     size_t m, uint8_t* scratch, uint8_t* out, unsigned long long* status);

// k_bases.hip: tables for caller-chosen points (xy: the point's 2 x 8 words, any curve point) and bjj_mul_bases,
// out[i] = sum_j scalars[j][i] * P_j over the A.t tables of A (one item per lane, one 512-lane workgroup per CU)
int bases_lanes_per_cu();
hipError_t base_window_bases(hipStream_t st, uint32_t* bases, int W, int nwin, const uint32_t xy[16]);
hipError_t check_base_table(hipStream_t st, int grid, const uint32_t* table, const uint32_t* bases, int W, int nwin, const uint32_t xy[16],
                            unsigned long long* d_bad);
hipError_t mul_bases(hipStream_t st, int cus, int lanes_per_cu, const bjj::BasesArgs& A, size_t n, uint8_t* out, uint32_t* scratch);

// k_signer.hip: verify / verify_schnorr against the one public key whose table A.T is (one item per lane, 256-lane workgroups,
// no scratch): ok[i] = 0 / 1, with schnorr 0 / 1 / 2
int signer_lanes_per_cu();
hipError_t verify_signer(hipStream_t st, int cus, int lanes_per_cu, bool schnorr, const bjj::SignerArgs& A, const uint8_t* r, const uint8_t* s,
                         const uint8_t* msg, size_t n, uint8_t* ok);

// k_signer_set.hip: the tables of a set of k signers in ONE allocation (signer j at entry offset j * nwin * (2^(W-1) + 1); keys: k
// records of SET_KEY_WORDS words, bases: k * nwin Niels entries) -- three launches whatever k: window bases and fill
// (build_signer_set), check (check_signer_set) -- and verify /
// verify_schnorr against pks[idx[i]] (the shape of verify_signer; ok[i] = 3 for idx[i] >= k)
int set_lanes_per_cu();
hipError_t build_signer_set(hipStream_t st, uint32_t* table, uint32_t* bases, const uint32_t* keys, size_t k, int W, int nwin);
hipError_t check_signer_set(hipStream_t st, int grid, const uint32_t* table, const uint32_t* bases, const uint32_t* keys, size_t k, int W,
                            int nwin, unsigned long long* d_bad);
hipError_t verify_set(hipStream_t st, int cus, int lanes_per_cu, bool schnorr, const bjj::SetArgs& A, const uint32_t* idx, const uint8_t* r,
                      const uint8_t* s, const uint8_t* msg, size_t n, uint8_t* ok);

// k_dlog.hip: small-range discrete logarithms (dlog.hpp).  params: DLOG_PARAM_WORDS words that dlog_setup_table fills for the other
// launches; slots: 2^(b+2) zeroed 8-byte slots.  dlog_build_table adds the entries it could not place to *d_failed;
// dlog_check_table adds the violated conditions to d_bad2[0] and the occupied slots to d_bad2[1]; dlog_search runs giant steps
// s0 .. s1 - 1 for n items (s0 > 0: only items whose ok is BJJ_DLOG_IN_FLIGHT go on; last: this launch ends the call's walk)
hipError_t dlog_setup_table(hipStream_t st, uint32_t* params, int b, const uint32_t* xy /* 16 words, NULL = B8 */);
hipError_t dlog_build_table(hipStream_t st, unsigned long long* slots, const uint32_t* params, int b, unsigned long long* d_failed);
hipError_t dlog_check_table(hipStream_t st, int grid, const unsigned long long* slots, const uint32_t* params, int b, unsigned long long* d_bad2);
hipError_t dlog_search(hipStream_t st, const unsigned long long* slots, const uint32_t* params, int b, const uint8_t* pts, size_t n,
                       int range_bits, uint32_t s0, uint32_t s1, bool last, unsigned long long* out_m, uint8_t* ok);

// k_point_sum.hip: bjj_point_sum -- m signed point sums over the CSR segments offsets[0 .. m] of one point array (point_sum.hpp).
// The scratch of one call is ONE device block laid out by point_sum_layout (byte offsets, 256-B aligned): the offsets-are-bad word
// and the two entry lists the levels alternate between (two entries per tile).  `neg`: n bytes or nullptr; `out`, `status` as for
// msm_batch.  m >= 1.
struct PointSumLayout {
  int levels;
  size_t o_flag, o_e0, o_e1, bytes;
};
PointSumLayout point_sum_layout(size_t n);
hipError_t point_sum(hipStream_t st, const PointSumLayout& L, const uint8_t* pts, const uint8_t* neg, size_t n, const uint64_t* offsets,
                     size_t m, uint8_t* scratch, uint8_t* out, unsigned long long* status);

// k_common_scalar.hip: one scalar, many points (common_scalar.hpp) -- out[i] = add[i] + (the digits D) * pts[i], one 256-item tile per
// workgroup.  form: CS_FORM_NAF (no table, no slot queue) or CS_FORM_TABLE (vb_tables / slotq / slot_cap as for K2's tiles).
//   COMMON_POINT     add may be nullptr; out: n * 64 bytes, ok: n bytes (1, or 2 and (0, 0) for an off-curve item); scratch: n * 64 bytes
//   COMMON_SUBGROUP  ok: n bytes (1 = the product is the identity, 0 = it is not, 2 = off the curve); no add, out or scratch
//   COMMON_DECRYPT   the point form with add != nullptr and no ok
enum { COMMON_POINT = 0, COMMON_SUBGROUP = 1, COMMON_DECRYPT = 2 };
int common_scalar_table_blocks_per_cu();
hipError_t mul_common(hipStream_t st, int form, int epi, const bjj::CsDigits& D, const uint8_t* pts, const uint8_t* add, size_t n, uint8_t* out,
                      uint8_t* ok, uint32_t* scratch, uint32_t* vb_tables, uint32_t* slotq, uint32_t slot_cap);

// k_elgamal.hip: bjj_elgamal_encrypt -- c1[i] = A1[i] + r[i] G, c2[i] = A2[i] + m[i] G + r[i] PK (elgamal.hpp), one item per lane, one
// 512-lane workgroup per CU.  A.add_c1 / A.add_c2: both or neither (then ok may be nullptr); out_c1 / out_c2 may be the add arrays
// themselves; scratch: 2 * n records of 64 bytes
int elgamal_lanes_per_cu();
hipError_t elgamal_encrypt(hipStream_t st, int cus, int lanes_per_cu, const bjj::ElgamalArgs& A, size_t n, uint8_t* out_c1, uint8_t* out_c2,
                           uint8_t* ok, uint32_t* scratch);

// k_dleq.hip: bjj_mul_pair -- out[i] = add[i] + a[i] P[i] + b[i] Q[i] (dleq.hpp; A.add may be nullptr; ok: 1, or 2 and (0, 0) for an
// off-curve item; scratch: n * 64 bytes) -- and bjj_dleq_verify -- ok[i] = 0 / 1 / 2 --, one item per lane, 256-lane workgroups,
// grid-strided over at most cus * lanes_per_cu lanes; vb_tables: BJJ_DLEQ_LANE_WORDS words for each of those lanes.  The prover's
// chain starts with dleq_nonce (z[i] = w[i] mod l) and ends with dleq_respond (the hash and z; ok[i] == 1: the item has its points).
#define BJJ_DLEQ_LANE_WORDS (2 * 36 * 9)   // two raw per-lane tables
int dleq_lanes_per_cu();
int dleq_block();
int occ_dleq_respond();
hipError_t mul_pair(hipStream_t st, int cus, int lanes_per_cu, const bjj::PairArgs& A, size_t n, uint8_t* out, uint8_t* ok, uint32_t* scratch,
                    uint32_t* vb_tables);
hipError_t dleq_verify(hipStream_t st, int cus, int lanes_per_cu, const bjj::DleqVerifyArgs& A, size_t n, uint8_t* ok, uint32_t* vb_tables);
hipError_t dleq_nonce(hipStream_t st, int grid, const uint8_t* w, size_t n, uint8_t* z);
hipError_t dleq_respond(hipStream_t st, int grid, const bjj::DleqRespondArgs& A, size_t n, const uint8_t* ok);

}  // namespace bjjk
