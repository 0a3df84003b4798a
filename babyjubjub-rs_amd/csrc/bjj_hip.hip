// libbjj_hip.so -- host side: contexts and the extern "C" boundary declared in include/bjj_hip.h.
// There is no CPU fallback anywhere in this library: every entry point launches device code or
// returns an error.
//
// Kernel map (SURVEY.md section 2 "kernel inventory"; kernels in k_*.hip, bodies in bjj_device.hpp / sign.hpp):
//   k_fixed.hip       bjj_k_build_fixed_table   init-time: window table of B8 multiples (affine Niels form)
//                     bjj_k_mul_fixed_base      K1  B8.mul_scalar(n)               src/lib.rs:149-164, 37-46
//   k_var.hip         bjj_k_mul_var_base[_wide] K2  P.mul_scalar(n), on-curve P    src/lib.rs:149-164
//                     bjj_k_mul_var_base_exact  K6  the reference's exact op sequence for off-curve P
//                     bjj_k_point_add / bjj_k_proj_add / bjj_k_proj_affine         src/lib.rs:88-131, 70-85
//   k_hash_codec.hip  bjj_k_poseidon5           K3  POSEIDON.hash([a,b,c,d,e])     src/lib.rs:400-404
//                     bjj_k_compress_points / bjj_k_decompress_points / bjj_k_merge_codec_flags   src/lib.rs:166-224, 260-268
//                     bjj_k_scalar_keys                                            src/lib.rs:284-302
//   k_verify.hip      bjj_k_eddsa_verify_scan / bjj_k_eddsa_verify / bjj_k_schnorr_verify
//                                               K4  verify / verify_schnorr        src/lib.rs:395-412, 375-385
//   k_sign.hip        bjj_k_sign / bjj_k_sign_schnorr                              src/lib.rs:308-361
//   k_small.hip       bjj_k_mul_var_base_quad / bjj_k_poseidon5_coop / bjj_k_eddsa_verify_small
//                                               K2 / K3 / K4 for SHORT calls: four lanes per item, six per hash, eight per signature
// K5 (batched affine conversion) is the epilogue of K1/K2 (k_common.hpp: block_invert).
// Multi-GPU: bjj_multi_* (bjj_multi.inc, included at the end of this file) -- one context per device,
// contiguous ceil(n/G) blocks; the device-resident form scatters inputs / gathers results with RCCL (bound with dlopen on
// first use) or with peer copies.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bjj_hip.h"
#include "../../include/bjj_hip_msm_batch.h"
#include "../../include/bjj_hip_bases.h"
#include "../../include/bjj_hip_signer.h"
#include "../../include/bjj_hip_signer_set.h"
#include "../../include/bjj_hip_dlog.h"
#include "../../include/bjj_hip_point_sum.h"
#include "../../include/bjj_hip_common_scalar.h"
#include "../../include/bjj_hip_elgamal.h"
#include "../../include/bjj_hip_dleq.h"
#include "bjj_device.hpp"
#include "bases.hpp"
#include "signer.hpp"
#include "signer_set.hpp"
#include "dlog.hpp"
#include "common_scalar.hpp"
#include "elgamal.hpp"
#include "dleq.hpp"
#include "bjj_launch.hpp"
#include "msm.hpp"
#include "copy_pool.hpp"
#include "pipe_plan.hpp"
#include "stage_plan.hpp"

using namespace bjj;

#ifdef BJJ_TEST_HOOKS   // `make hooks`: the same library plus the failure injection of bjj_multi.inc; never the shipped one
#define BJJ_VERSION_STRING "bjj-hip 0.6.0 gfx950 +test-hooks"
#else
#define BJJ_VERSION_STRING "bjj-hip 0.6.0 gfx950"
#endif
// Fixed-base window width.  window_bits = 0 (default) is a modest 23 bits = 11 signed digits, 5.9 GB: a library that
// is linked into a process with other tenants of the GPU must not take half of the HBM unasked.  The wide tables are
// opt-in: an explicit width (28 bits = 9 digits, 9 x (2^27 + 1) entries = 154.6 GB of the 288 GB; 26 = 10 digits,
// 42.9 GB) or BJJ_WINDOW_AUTO (-1) = the widest of these whose table fits in 60 % of the device's free memory.  One
// addition less per step: the kernel is VALU-bound and the cooperative gathers keep the table reads off the critical
// path at any size (profiles/r01i_ablation_window_bits_coop_gather.txt).
static const int kAutoWindowBits[] = {28, 26, 23, 21, 16};
#define BJJ_DEFAULT_WINDOW_BITS 23
#define BJJ_MAX_WINDOW_BITS 28

// ===========================================================================
// context
// ===========================================================================
// The error messages concatenate temporaries, and namespace std has default visibility: the library has always exported this weak
// instantiation.  Instantiated explicitly, so that the list of exported symbols does not depend on how many uses the inliner leaves.
template std::string std::operator+(std::string&&, std::string&&);
static thread_local std::string g_err;
static int set_err(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCK(call)                                                                                  \
  do {                                                                                               \
    hipError_t e_ = (call);                                                                          \
    if (e_ != hipSuccess)                                                                            \
      return set_err(BJJ_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));                  \
  } while (0)

// Every entry point runs on its context's device and leaves the calling thread's current HIP device as it found it (a host
// that shares the thread with torch or another HIP user must not find its default device changed).
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev == dev) prev = -1; else err = hipSetDevice(dev);
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define ENTER_DEVICE(dev)                                                                                       \
  DeviceGuard dg_(dev);                                                                                         \
  if (dg_.err != hipSuccess) return set_err(BJJ_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(dg_.err))

static void secure_bzero(void* p, size_t n) {
  memset(p, 0, n);
  __asm__ __volatile__("" : : "r"(p) : "memory");   // the stores must not be elided as dead
}
// ---- grow-only blocks -----------------------------------------------------------------------------------------------------
// Every device block and every pinned host block of a context is one of these: a pointer and its capacity in BYTES, owned -- the
// destructor releases it (ctx_destroy deletes the context with its device current) and it is never copied.  grow() is the only way
// a block gets larger: nothing happens while the request fits; otherwise the old block is freed and a new one allocated.  After a
// failed allocation the block is EMPTY (null, capacity 0), never a dangling pointer with a stale size.  A block with `wipe` set is
// zeroed over its whole capacity before it is freed, on growth as on release (bjj_init names the blocks key material passes through).
enum BlockWait { NO_WAIT, WAIT_DEVICE };
template <typename T, bool kPinned>
struct Block {
  T* p = nullptr;
  size_t bytes = 0;
  bool wipe = false;
  Block() = default;
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
  ~Block() { (void)release(); }
  operator T*() const { return p; }   // a block is used where its pointer is
  hipError_t release() {
    if (!p) return hipSuccess;
    if (wipe) { if (kPinned) secure_bzero(p, bytes); else (void)hipMemset(p, 0, bytes); }
    const hipError_t e = kPinned ? hipHostFree(p) : hipFree(p);
    p = nullptr; bytes = 0;
    return e;
  }
  // WAIT_DEVICE: launches of any stream may still use the old block, so the device is waited for before it is freed (a first
  // allocation and a request that fits wait for nothing).  NO_WAIT: nothing can be using it, or the site has waited itself.
  hipError_t grow(size_t want, BlockWait wait = WAIT_DEVICE) {
    if (want <= bytes) return hipSuccess;
    if (p && wait == WAIT_DEVICE) { const hipError_t e = hipDeviceSynchronize(); if (e != hipSuccess) return e; }
    hipError_t e = release();
    if (e == hipSuccess) e = kPinned ? hipHostMalloc((void**)&p, want, hipHostMallocDefault) : hipMalloc((void**)&p, want);
    if (e != hipSuccess) { p = nullptr; return e; }
    bytes = want;
    return hipSuccess;
  }
};
template <typename T> using DevBlock = Block<T, false>;
template <typename T> using PinBlock = Block<T, true>;
// a list of the items that take the exact-path kernels (ScratchSet::slow, bjj_ctx::pipe_wl): [0] = count, then n item indices at most
static size_t list_bytes(size_t n) { return (n + 16) * sizeof(u32); }

#define BJJ_PIPE_BUFS 4
#define BJJ_SCRATCH_SETS 2
// K1's two-workgroup shape on device pointers: workgroup slots per CU one launch takes (2 = 512 workgroups of 8 items per lane at 2^20
// items, 1 = 256 of 16; profiles/r09_ab_k1_long_lanes.txt)
#ifndef BJJ_K1_OVERLAP_SLOTS_DEFAULT
#define BJJ_K1_OVERLAP_SLOTS_DEFAULT 1
#endif
#define BJJ_STREAM_MARKS 8
struct ScratchSet {
  DevBlock<u32> scratch;       // n * 64 B (Z, prefix)
  DevBlock<u32> vb_tables;     // grid threads * VB_TABLE_WORDS_MAX * 4 B
  DevBlock<u32> slow;          // list_bytes(n): the items deferred to the exact-path kernels
  // verify: the on-curve scan of a call is routed through this stream of the HIGHEST priority, so that while another launch
  // of the context fills the chip its few light waves get the next slots that free up instead of queueing behind that
  // launch's pending workgroups for a whole launch (profiles/r03_ab_verify_group_dispatch.txt)
  hipStream_t scan_stream = nullptr;
  hipEvent_t ev_scan_in = nullptr, ev_scan_out = nullptr;
  u32* slotq2 = nullptr;       // variable base, one tile per workgroup: the same per-XCD rings, one slot = one workgroup's tables
  u32 slot_cap2 = 0;
  u32* slotq = nullptr;        // verify, one group per workgroup: per-XCD ring of free per-lane-table slots (k_verify.hip)
  u32 slot_cap = 0;            // slots per XCD
  DevBlock<uint8_t> codec;     // verify_compressed: n * (64 pk + 64 R + 32 s + 2 flags) bytes; public_keys: the scalar keys (wiped)
  DevBlock<uint8_t> xy;        // K1 with compressed output: n * 64 B, the phase-1 stash of X, Y (the 32-byte output slot cannot hold it)
  // The blocks of the staged host forms (Staged): one call's arrays at the offsets of a StagePlan
  DevBlock<uint8_t> msm;       // bjj_msm*, bjj_point_sum: the scratch the kernel layout describes (all the _dev forms take); host forms: + offsets, inputs, results
  DevBlock<uint8_t> bases_io;  // the host forms of bjj_mul_bases, *_verify_signer, *_verify_set, bjj_dlog, bjj_mul_common, bjj_in_subgroup and
                               // bjj_elgamal_decrypt: inputs, then outputs (wiped: ElGamal's r and the ciphertexts pass through)
  DevBlock<uint8_t> common_m;  // bjj_elgamal_decrypt: n * 64 B, M = C2 - sk * C1 between the shared-scalar launch and the logarithm's
  // Ordering of the set: every call that uses it records `ev_last` on its stream after enqueueing, and a call on a
  // DIFFERENT stream first makes its stream wait for it.  Calls return before the work runs, so "serialised by the
  // caller" alone would not order execution.
  hipEvent_t ev_last = nullptr;
  hipStream_t last_stream = nullptr;
  bool have_last = false;
  uint64_t last_use = 0;
  uint64_t last_set_use = 0;   // value of bjj_ctx::set_uses when this set was taken last
};
struct StreamMark {
  hipStream_t stream = nullptr;
  hipEvent_t ev = nullptr;
  bool used = false;
  uint64_t last_use = 0;
};
// A fixed-base table for a caller-chosen curve point (include/bjj_hip_bases.h): the layout of the context's B8 table with
// base_nwin(W) windows (bases.hpp).  Owned by its context (bjj_ctx::user_bases); a handle that exists is a table that passed its check.
struct bjj_base {
  bjj_ctx* ctx = nullptr;
  int W = 0, nwin = 0;
  u32 xy[16] = {0};          // the point as given (the kernels reduce the coordinates mod r)
  DevBlock<u32> table;       // [window][digit 0 .. 2^(W-1)] x 128 B
  DevBlock<u32> bases;       // P_j = 2^(W j) * P, one Niels entry per window
};
// The tables of a set of k signers (include/bjj_hip_signer_set.h): ONE allocation, signer j at entry offset j * nwin * (2^(W-1) + 1)
// (signer_set.hpp).  Owned by its context (bjj_ctx::user_sets); a handle that exists is a set whose k tables passed their check.
struct bjj_signer_set {
  bjj_ctx* ctx = nullptr;
  int W = 0, nwin = 0;
  size_t k = 0;
  DevBlock<u32> table;       // [signer][window][digit 0 .. 2^(W-1)] x 128 B
  DevBlock<u32> bases;       // P_{s,j} = 2^(W j) * key_s, one Niels entry per signer and window
  DevBlock<u32> keys;        // the k keys as the hash takes them: SET_KEY_WORDS words each
};
// The baby-step table of one base point (include/bjj_hip_dlog.h, dlog.hpp).  Owned by its context (bjj_ctx::user_dlogs); a handle
// that exists is a table that passed its check.
struct bjj_dlog_table {
  bjj_ctx* ctx = nullptr;
  int b = 0;                               // baby_bits
  uint8_t base_xy[64] = {0};               // the base point, coordinates reduced mod r
  DevBlock<unsigned long long> slots;      // 2^(b+2) slots {tag, j + 1}
  DevBlock<u32> params;                    // DLOG_PARAM_WORDS words: Niels(G), Niels(-2^b G), Niels(-2^(b+1) G), the base's record
};
// The handles a context has handed out and not been given back (bjj_base, bjj_signer_set, bjj_dlog_table): the context owns them
template <typename T>
struct Handles {
  std::vector<T*> v;
  bool owns(const T* h) const { for (const T* k : v) if (k == h) return true; return false; }
  void add(T* h) { v.push_back(h); }   // may throw: the caller still owns h then
  void drop(T* h) {                    // forgets and deletes h
    for (size_t i = 0; i < v.size(); i++) if (v[i] == h) { v.erase(v.begin() + (long)i); break; }
    delete h;
  }
  void clear() { for (T* h : v) delete h; v.clear(); }   // the handles the caller never freed
};
// Giant steps ONE launch of bjj_dlog / bjj_dlog_dev performs at most, summed over its items; a longer call is cut into consecutive
// launches: 2^27 steps fill the chip for 29 ms.  BJJ_DLOG_LAUNCH_STEPS, read once here, lowers or raises it
// (tests force the cut with it).  Beside it, no launch walks an item further than BJJ_DLOG_LAUNCH_STEPS_PER_ITEM steps -- a workgroup
// takes 56 us per step whatever the rest of the chip does, so 512 steps are 29 ms for a launch of few items too -- nor, where the
// bound would allow fewer, less than BJJ_DLOG_LAUNCH_STEPS_MIN (a later launch pays a ladder worth 13 steps to get to its first).
#define BJJ_DLOG_LAUNCH_STEPS_DEFAULT ((uint64_t)1 << 27)
#define BJJ_DLOG_LAUNCH_STEPS_MIN 64
#define BJJ_DLOG_LAUNCH_STEPS_PER_ITEM 512
static uint64_t dlog_launch_steps_from_env() {
  uint64_t v = BJJ_DLOG_LAUNCH_STEPS_DEFAULT;
  if (const char* e = getenv("BJJ_DLOG_LAUNCH_STEPS")) {
    char* end = nullptr;
    const unsigned long long x = strtoull(e, &end, 10);
    if (end != e && *end == 0 && x >= BJJ_DLOG_LAUNCH_STEPS_MIN) v = (uint64_t)x;
  }
  return v;
}
static int common_form_from_env();   // bjj_common_scalar.inc
struct bjj_ctx {
  int device = 0;
  int cus = 0;
  int W = 16, nwin = 16;
  double init_ms = 0.0;
  // residency of each kernel (hipOccupancyMaxActiveBlocksPerMultiprocessor): grids are sized to exactly one resident set
  // of workgroups, items are grid-strided.  K1 / K2: resident LANES per CU (their workgroup size is the kernel unit's
  // business); the others: resident 256-lane workgroups per CU
  int lanes_fixed = 512, lanes_var = 512;
  int lanes_fixed_2x256 = 512;   // resident lanes per CU of K1's two-workgroup shape
  int lanes_bases = 512;         // resident lanes per CU of bjj_k_mul_bases
  int lanes_elgamal = 512;       // ... of bjj_k_elgamal_encrypt
  int lanes_dleq = 512;          // ... of the k_dleq.hip kernels with per-lane tables (dleq_tables)
  int occ_dleq_respond = 1;      // resident 256-lane workgroups per CU of the prover's two small kernels
  int lanes_signer = 512;        // resident lanes per CU of the bjj_k_*_verify_signer kernels
  Handles<bjj_base> user_bases;         // the tables bjj_base_create made and bjj_base_free has not released yet
  int lanes_set = 512;           // resident lanes per CU of the bjj_k_*_verify_set kernels
  Handles<bjj_signer_set> user_sets;        // the sets bjj_signer_set_create made and bjj_signer_set_free has not released yet
  Handles<bjj_dlog_table> user_dlogs;      // the tables bjj_dlog_table_create made and bjj_dlog_table_free has not released yet
  uint64_t dlog_launch_steps = 0;           // giant steps one launch of bjj_dlog performs at most, over all its items (BJJ_DLOG_LAUNCH_STEPS)
  int common_form = -1;          // one scalar, many points: -1 = per call by the multiplication count, 0 = table-free, 1 = table (BJJ_COMMON_FORM)
  int last_common_form = -1;
  int verify_mode = -1;          // -1 = per call (persistent waves for one launch > 2^21 items that runs alone, groups otherwise), 0 / 1 = forced (BJJ_VERIFY_DISPATCH)
  int k2_variant = -1;           // -1 = per call (tiles for a launch that runs alone, grid-strided while another is in flight), 0 / 1 = forced (BJJ_K2_VARIANT)
  int k1_variant = -1;           // -1 = per call (two-workgroup shape while another launch of the context is in flight), 0 / 1 = forced (BJJ_K1_VARIANT)
  int k1_overlap_slots = BJJ_K1_OVERLAP_SLOTS_DEFAULT;   // workgroup slots per CU a launch of the two-workgroup shape takes (BJJ_K1_OVERLAP_SLOTS = 1 | 2)
  int last_k1_slots = -1;
  int occ_poseidon = 1, occ_verify = 1, occ_scan = 1, occ_add = 1;
  // Variable base, off-curve points (k_var.hip): K6 runs BEHIND K2 on the caller's stream (nothing extra for a clean batch) or,
  // with the list made by a scan, BESIDE it on the set's priority stream.  -1 = per call by what the previous calls met
  // (vb_seen: one device-visible pinned word per scratch set, written by K6 with the number of items it had), 0 / 1 = forced
  // (BJJ_VB_SPLIT)
  int vb_split = -1;
  int occ_vb_scan = 1;
  PinBlock<u32> vb_seen;                   // [BJJ_SCRATCH_SETS] per set (device-pointer calls) + [1] the host-pointer pipeline
  int last_vb_split = -1;
  PinBlock<uint8_t> patch_host;            // host-pointer pipeline: K6's results on their way into the caller's array
  int xccs = 1;                // XCDs of the device (probed at init; sizes the verify kernels' slot queues)
  int occ_decomp = 1, occ_sign = 1, occ_sign_schnorr = 1;
  // signer hardening (bjj_set_signer_constant_time): a second, small fixed-base table (4-bit windows: 63 x 9 entries) that
  // the signer kernels SCAN instead of indexing; built on first use
  bool ct_signer = false;
  DevBlock<u32> ct_table, ct_bases;
  int occ_sign_ct = 1, occ_sign_schnorr_ct = 1;
  hipStream_t stream = nullptr;
  DevBlock<u32> table;       // [window][digit 0 .. 2^(W-1)] x 128 B
  DevBlock<u32> bases;       // P_j = 2^(W j) * B8, one Niels entry per window
  int table_alloc = BJJ_TABLE_ALLOC_PLAIN;   // how `table` was allocated (bjj_info.table_alloc)
  // Scratch is kept in BJJ_SCRATCH_SETS independent sets so that calls on two streams can be in flight at once
  // (pick_set): a launch whose last wave-round is only partly filled -- 2^20 verifications are 8.1 rounds of the 2 048
  // resident waves, 2^20 variable-base multiplications 5.3 rounds of the 196 608 resident lanes -- then shares the chip
  // with the head of the next launch instead of idling it.  A single-stream caller only ever touches (and allocates) set 0.
  ScratchSet set[BJJ_SCRATCH_SETS];
  uint64_t use_counter = 0;
  uint64_t set_uses = 0;         // calls that took a scratch set (streams_alternate)
  // calls that use no scratch (Poseidon, point add, codec, sign) are not ordered behind anything; their completion
  // events are only kept so that bjj_sync can wait for them: one slot per distinct caller stream
  StreamMark marks[BJJ_STREAM_MARKS];
  // host-pointer API (run_pipelined): chunked pipeline
  //   caller's array -[H2D, s_in]-> dstage -[kernels on the lanes stream / stream2, chunks alternating]-> dstage -[D2H, s_out]-> caller's array
  // straight from / to the caller's memory when that is pinned (bjj_host_alloc / bjj_host_register / any hipHostMalloc'd or
  // hipHostRegister'ed range); a PAGEABLE array goes through the rings pin_in[] / pin_out[], moved by the context's copy workers
  // (CopyPool), never by the enqueueing thread
  hipStream_t s_in = nullptr, s_out = nullptr, stream2 = nullptr;
  std::vector<hipEvent_t> ev_in, ev_k, ev_out;   // per chunk of a super-batch (grown on demand)
  std::vector<hipEvent_t> ev_mid;          // ... and behind a chunk's decompressions on its lane (the wire-format verifier's exact list)
  hipEvent_t ev_tail = nullptr;            // behind the exact-list stage of a call (ExactListStage::close)
  DevBlock<u32> pipe_wl;                   // ONE list of the items that take the exact kernel, per super-batch (ExactListStage)
  DevBlock<uint8_t> dstage;                // device staging for one super-batch: every array contiguous (wiped)
  PinBlock<uint8_t> pin_in[BJJ_PIPE_BUFS];    // pinned rings of the staged path (allocated on the first call that has a pageable array; wiped)
  PinBlock<uint8_t> pin_out[BJJ_PIPE_BUFS];
  size_t pipe_budget = 0;                  // bytes of device staging a call may take (BJJ_PIPE_STAGING_MB)
  CopyPool* pool = nullptr;
  size_t pipe_chunk = 0, pipe_first = 0;   // chunk schedule (items): first chunk, doubling up to pipe_chunk
  bool pipe_env_schedule = false;          // ... given in the environment: it overrides the entry points' own schedules too
  bool pipe_ready = false;                 // ensure_pipe's first-use block ran to its end
  bool pipe_small_direct = true;           // BJJ_PIPE_SMALL_DIRECT=0: short calls on pinned memory keep their copies (A/B, tests)
  bool pipe_zero_copy_in = true;           // BJJ_PIPE_ZERO_COPY_IN=0: inputs always arrive through the copy engines (A/B, tests)
  bool k1_half_now = false;                // a host-pointer call is enqueueing chunk launches of K1 that take ONE workgroup slot per CU each
  bool pipe_zero_copy = true;              // BJJ_PIPE_ZERO_COPY=0: results always leave through the copy engines (A/B, tests)
  u32 last_host_zero_copy = 0;
  bool in_pipeline = false;                // a host-pointer call is enqueueing (enqueue_verify: where the scans run)
  bool pipe_scan_inline = true;            // BJJ_PIPE_SCAN=prio (developer): scans of the pipeline's chunks on the priority streams
  bool force_staged = false;               // BJJ_HOST_FORCE_STAGED=1: treat every host array as pageable (A/B, tests)
  // what the last calls did (bjj_get_info; tests and the bench line read these)
  int last_k1 = -1, last_k2 = -1, last_verify_mode = -1;
  size_t fb_quad_max = (size_t)1 << 15;        // fixed base / public keys: calls of at most this many items run four lanes per item (BJJ_FB_QUAD_MAX; 0 = never)
  size_t sign_small_max = (size_t)1 << 13;     // sign: calls of at most this many signatures run eight lanes per signature (BJJ_SIGN_SMALL_MAX; 0 = never)
  int last_sign = -1;
  size_t verify_small_max = (size_t)1 << 13;   // EdDSA verify: calls of at most this many signatures run eight lanes per signature (BJJ_VERIFY_SMALL_MAX; 0 = never)
  size_t p5_coop_max = (size_t)1 << 14;    // Poseidon: calls of at most this many hashes run six lanes per hash (BJJ_P5_COOP_MAX; 0 = never)
  int last_p5 = -1;
  size_t vb_quad_max = (size_t)1 << 14;    // variable base: calls of at most this many items run four lanes per item (BJJ_VB_QUAD_MAX; 0 = never)
  int idle_alternations = 0;               // expect_overlap: consecutive alternating calls that found the other set idle
  u32 last_host_direct = 0, last_host_staged = 0, last_host_chunks = 0;
  DevBlock<u32> slot_block;                // all slot-queue rings of the context in one device allocation (slot_block_make)
  PinBlock<u32> err_words;                 // the ring block as read back by ctx_check_slot_queues
  bool rings_used = false;                 // a kernel that pops / pushes slots has been launched since the last check
};

static int grid_for(const bjj_ctx* c, size_t n, int blocks_per_cu, int block = BJJ_BLOCK) {
  return bjjk::capped_grid(n, block, (size_t)c->cus * blocks_per_cu);   // the same number for every n, n = 0 included (one workgroup)
}

// Which scratch set a call on stream `st` uses:
//  (1) the set this stream used last -- calls of one stream are ordered by the stream itself, nothing to wait for;
//  (2) else a set that was never used;  (3) else the least recently used one (the caller then waits for its last call).
// Two streams that alternate therefore settle on one set each and overlap; one stream never leaves set 0.
static ScratchSet* pick_set(bjj_ctx* c, hipStream_t st) {
  for (ScratchSet& S : c->set) if (S.have_last && S.last_stream == st) return &S;
  for (ScratchSet& S : c->set) if (!S.have_last) return &S;
  ScratchSet* lru = &c->set[0];
  for (ScratchSet& S : c->set) if (S.last_use < lru->last_use) lru = &S;
  return lru;
}
// Makes `st` safe to touch set S: waits (on the device) for the set's last call if that ran on another stream.
static int set_enter(bjj_ctx* c, ScratchSet* S, hipStream_t st) {
  if (!S->ev_last) HIPCK(hipEventCreateWithFlags(&S->ev_last, hipEventDisableTiming));
  if (S->have_last && S->last_stream != st) HIPCK(hipStreamWaitEvent(st, S->ev_last, 0));
  return BJJ_OK;
}
static int set_leave(bjj_ctx* c, ScratchSet* S, hipStream_t st) {
  HIPCK(hipEventRecord(S->ev_last, st));
  S->last_stream = st;
  S->have_last = true;
  S->last_use = ++c->use_counter;
  S->last_set_use = ++c->set_uses;
  return BJJ_OK;
}
// Is a launch of this context that uses ANOTHER scratch set still queued or running?  (event query: no synchronisation)
// hipEventQuery leaves hipErrorNotReady as the thread's last error; it is cleared on EVERY path so that a launcher that reads
// hipGetLastError() after its launch never reports it.
static bool other_launch_in_flight(bjj_ctx* c, const ScratchSet* mine) {
  bool busy = false;
  for (const ScratchSet& S : c->set)
    if (&S != mine && S.have_last && hipEventQuery(S.ev_last) == hipErrorNotReady) busy = true;
  (void)hipGetLastError();   // hipErrorNotReady is not an error
  return busy;
}
// Does the caller ALTERNATE over streams (one scratch set each)?  True when another set took one of the last
// BJJ_SCRATCH_SETS calls that used scratch.  Unlike the event query above this does not depend on how far the device has got
// when the host enqueues: a caller that ping-pongs over two streams gets the same kernel shape for every launch of the run,
// a one-stream caller never sees it (profiles/r04_driver_protocol.txt).
static bool streams_alternate(const bjj_ctx* c, const ScratchSet* mine) {
  for (const ScratchSet& S : c->set)
    if (&S != mine && S.have_last && c->set_uses - S.last_set_use < BJJ_SCRATCH_SETS) return true;
  return false;
}
// A launch of more than 2^21 items gains nothing from sharing the chip with another launch of the context (its partly empty last
// round is a fraction of a percent) but would lose the kernel form that is best for a launch that runs alone (persistent verify
// waves, K2 tiles: 2-4 % at >= 2^22 items, profiles/r03_throughput_vs_batch.txt).  Such a launch therefore queues BEHIND the other
// scratch sets' last calls (a device-side wait, no host synchronisation) and is then enqueued as a launch that runs alone.
#define BJJ_LARGE_LAUNCH ((size_t)1 << 21)
static int wait_for_other_sets(bjj_ctx* c, const ScratchSet* mine, hipStream_t st) {
  for (const ScratchSet& S : c->set)
    if (&S != mine && S.have_last && S.last_stream != st) HIPCK(hipStreamWaitEvent(st, S.ev_last, 0));
  return BJJ_OK;
}
// Will this launch share the chip with another launch of the context?  The kernels come in a form for a launch that runs alone
// and a form for overlapping launches (K1: one 512-lane workgroup per CU / two of 256 lanes; K2: tiles / grid-strided; verify:
// scan in line / on the priority stream), and the wrong form costs: K1's two-workgroup shape run ALONE takes 0.611-0.623 ms instead
// of 0.602-0.605 ms (+1.5 ... 3 %), K2's grid-strided form alone 14.63 instead of 14.13 ms (+3.5 %; profiles/r05_driver_protocol.txt,
// r05_host_pipeline.txt).  Pattern AND state decide:
//   * another set's launch is still queued or running (event query)          -> overlap
//   * else the caller alternates over streams (streams_alternate) and this is the FIRST such call that finds the other set
//     idle -- the first launch behind a synchronisation point of a caller that ping-pongs, e.g. launch 0 of a timed region:
//     the pattern says the next launch follows at once (profiles/r04_driver_protocol.txt)                   -> overlap
//   * else (one stream; or a caller that alternates but synchronises between its launches, so that the second call in a row
//     finds the other set idle)                                                                             -> alone
// One rule for the three entry points (enqueue_verify used the bare event query until round 4).
static bool expect_overlap(bjj_ctx* c, const ScratchSet* S) {
  if (other_launch_in_flight(c, S)) { c->idle_alternations = 0; return true; }
  if (!streams_alternate(c, S)) { c->idle_alternations = 0; return false; }
  if (c->idle_alternations < 2) c->idle_alternations++;
  return c->idle_alternations < 2;
}
static int fixed_base_variant(bjj_ctx* c, const ScratchSet* S) {
  const int kv = c->k1_half_now ? 1 : (c->k1_variant >= 0 ? c->k1_variant : (expect_overlap(c, S) ? 1 : 0));
  c->last_k1 = kv;
  return kv;
}
// lanes per CU the launch may take: everything its shape can hold, or ONE 256-lane workgroup per CU, so that the neighbouring
// launch has the other slot and every lane keeps its slot for the whole launch (one ramp, one running product, one inversion
// per slot instead of two) -- always for the chunk launches of a host-pointer call (PipeSpec::k1_half), and for launches on
// device pointers that get the two-workgroup shape when the context's k1_overlap_slots is 1.  The shape is only ever chosen for
// a launch that shares the chip (expect_overlap) or forced (BJJ_K1_VARIANT=1): a launch that runs alone keeps the 512-lane form.
static int fixed_base_lanes(bjj_ctx* c, int kv) {
  const bool one_slot = kv == 1 && (c->k1_half_now || c->k1_overlap_slots == 1);
  c->last_k1_slots = kv == 1 ? (one_slot ? 1 : 2) : 0;
  if (one_slot) return 256;
  return kv ? c->lanes_fixed_2x256 : c->lanes_fixed;
}
// completion mark of a call that used no scratch (bjj_sync waits for these)
static int mark_stream(bjj_ctx* c, hipStream_t st) {
  if (st == c->stream) return BJJ_OK;   // bjj_sync synchronises the context's own stream anyway
  StreamMark* m = nullptr;
  for (StreamMark& k : c->marks) if (k.used && k.stream == st) { m = &k; break; }
  if (!m) for (StreamMark& k : c->marks) if (!k.used) { m = &k; break; }
  if (!m) {   // more caller streams than slots: retire the oldest mark (wait for it, then reuse the slot)
    m = &c->marks[0];
    for (StreamMark& k : c->marks) if (k.last_use < m->last_use) m = &k;
    HIPCK(hipEventSynchronize(m->ev));
  }
  if (!m->ev) HIPCK(hipEventCreateWithFlags(&m->ev, hipEventDisableTiming));
  HIPCK(hipEventRecord(m->ev, st));
  m->stream = st; m->used = true; m->last_use = ++c->use_counter;
  return BJJ_OK;
}

// Per-XCD rings of free table slots (k_common.hpp): [0] head ticket, [1] tail ticket, [2] pops that gave up (SLOTQ_ERR),
// [16 + i] = slot id + 1.  (Re)built on the host: every slot free.
#define BJJ_SLOTQ_HDR 16
#define BJJ_SLOTQ_ERR 2
static int slot_queue_fill(bjj_ctx* c, u32* d_q, u32 cap) {
  const size_t stride = BJJ_SLOTQ_HDR + cap;
  std::vector<u32> h((size_t)c->xccs * stride, 0u);
  for (int x = 0; x < c->xccs; x++)
    for (u32 i = 0; i < cap; i++) h[(size_t)x * stride + BJJ_SLOTQ_HDR + i] = (u32)x * cap + i + 1u;   // slot id + 1
  HIPCK(hipMemcpyAsync(d_q, h.data(), h.size() * sizeof(u32), hipMemcpyHostToDevice, c->stream));   // pageable source: staged before the call returns
  HIPCK(hipStreamSynchronize(c->stream));
  return BJJ_OK;
}
// All rings of a context -- two per scratch set: verify's (cap slots per XCD) and the variable-base tiles' (cap2) -- live in ONE
// device block, so that the check below reads them back with a single copy.  The capacities are constants of the context
// (occupancy x CUs per XCD): the block is made once, when the first scratch set is sized.
static size_t slot_ring_words(const bjj_ctx* c, u32 cap) { return (size_t)c->xccs * (BJJ_SLOTQ_HDR + cap); }
static int slot_block_make(bjj_ctx* c, u32 cap, u32 cap2) {
  if (c->slot_block) return BJJ_OK;
  const size_t per_set = slot_ring_words(c, cap) + slot_ring_words(c, cap2);
  HIPCK(c->slot_block.grow(BJJ_SCRATCH_SETS * per_set * sizeof(u32), NO_WAIT));
  if (c->err_words.grow(c->slot_block.bytes, NO_WAIT) != hipSuccess) {
    (void)hipGetLastError(); (void)c->slot_block.release();
    return set_err(BJJ_E_NOMEM, "slot queues: no pinned memory for the read-back buffer");
  }
  for (int k = 0; k < BJJ_SCRATCH_SETS; k++) {
    ScratchSet& S = c->set[k];
    S.slotq = c->slot_block + (size_t)k * per_set;  S.slot_cap = cap;
    S.slotq2 = S.slotq + slot_ring_words(c, cap);     S.slot_cap2 = cap2;
    int rc = slot_queue_fill(c, S.slotq, cap);
    if (!rc) rc = slot_queue_fill(c, S.slotq2, cap2);
    if (rc) { for (ScratchSet& T : c->set) { T.slotq = T.slotq2 = nullptr; T.slot_cap = T.slot_cap2 = 0; } (void)c->slot_block.release(); return rc; }
  }
  return BJJ_OK;
}
// After the launches in question have completed: did a pop ever give up waiting for a slot?  ONE asynchronous copy of the ring
// block (35 KB) on the context's own non-blocking stream into pinned memory -- not four synchronous pageable copies through
// the legacy null stream, which also made the caller wait for other tenants' blocking streams -- and only when a
// kernel that uses the rings has been launched since the last check (rings_used: 2^20 fixed-base multiplications on host
// pointers take 1.5 ms, a check that costs 0.17 ms has no business there).  A ring is rebuilt only when its counter is
// non-zero.  Every entry point that synchronises for the caller ends with this check (bjj_sync, the host-pointer pipeline, the
// multi-GPU pipeline): a launch that worked on the overflow slot must never be reported as BJJ_OK.
static int ctx_check_slot_queues(bjj_ctx* c, const char* who) {
  if (!c->slot_block || !c->rings_used) return BJJ_OK;
  HIPCK(hipMemcpyAsync(c->err_words, c->slot_block, c->slot_block.bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCK(hipStreamSynchronize(c->stream));
  c->rings_used = false;
  unsigned long long starved = 0;
  for (ScratchSet& S : c->set) {
    struct Ring { u32* q; u32 cap; } rings[2] = {{S.slotq, S.slot_cap}, {S.slotq2, S.slot_cap2}};
    for (const Ring& r : rings) {
      const u32* h = c->err_words + (r.q - c->slot_block);
      unsigned long long bad = 0;
      for (int x = 0; x < c->xccs; x++) bad += h[(size_t)x * (BJJ_SLOTQ_HDR + r.cap) + BJJ_SLOTQ_ERR];
      if (bad) { int rc = slot_queue_fill(c, r.q, r.cap); if (rc) return rc; }
      starved += bad;
    }
  }
  if (starved)
    return set_err(BJJ_E_HIP, std::string(who) + ": " + std::to_string(starved) + " workgroup(s) gave up waiting for a per-lane table slot; the results of "
                   "the verify / variable-base launches since the last synchronising call are not valid (slot queues rebuilt)");
  return BJJ_OK;
}

static int ensure_scratch(bjj_ctx* c, ScratchSet* S, size_t n) {
  HIPCK(S->scratch.grow(n * 64));
  HIPCK(S->slow.grow(list_bytes(n)));
  // slots of per-lane tables: K2 needs its resident lanes; verify (2 tables per lane) the waves that can be resident, rounded
  // up to a whole number per XCD (the slot queues are per XCD); plus ONE overflow slot per XCD behind the regular ones (what a
  // pop that gave up waiting continues on, k_common.hpp)
  const size_t cu_per_xcc = ((size_t)c->cus + c->xccs - 1) / c->xccs;
  const u32 cap = (u32)(cu_per_xcc * c->occ_verify);   // occ_verify counts waves
  const u32 cap2 = (u32)(cu_per_xcc * (size_t)(c->lanes_var / bjjk::var_base_block()));
  const size_t tv = (size_t)c->xccs * ((size_t)cap2 + 1) * (size_t)bjjk::var_base_block();
  const size_t tv_strided = cu_per_xcc * c->xccs * (size_t)c->lanes_var;          // the grid-strided form indexes by global lane
  const size_t te = (size_t)c->xccs * ((size_t)cap + 1) * 64 * 2;
  size_t threads = tv > te ? tv : te;
  if (tv_strided > threads) threads = tv_strided;
  { int rc = slot_block_make(c, cap, cap2); if (rc) return rc; }
  HIPCK(S->vb_tables.grow(threads * VB_TABLE_WORDS_MAX * sizeof(u32)));
  return BJJ_OK;
}
#include "host_pipe.inc"
static int ensure_codec(ScratchSet* S, size_t n) {  // 162 bytes per item of intermediate records
  HIPCK(S->codec.grow(n * 162 + 64));
  return BJJ_OK;
}
static int ensure_xy(ScratchSet* S, size_t n) {     // 64 bytes per item: X, Y of phase 1 when the output slot is 32 bytes
  HIPCK(S->xy.grow(n * 64));
  return BJJ_OK;
}
static bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
// a block of a scratch set holds at least `bytes`; a block this size may well not fit: the set stays usable, without that block
static int grow_block(DevBlock<uint8_t>& b, size_t bytes, const char* who, const char* noun) {
  if (b.grow(bytes) == hipSuccess) return BJJ_OK;
  (void)hipGetLastError();
  return set_err(BJJ_E_NOMEM, std::string(who) + ": cannot allocate " + std::to_string(bytes >> 20) + " MB of " + noun);
}
// ---- the synchronous single-launch host forms --------------------------------------------------------------
// One staged call on the context's own stream.  The entry declares its arrays in argument order, the inputs first (in / out; *_opt:
// an array the caller may leave out; *_at: at an offset inside the scratch prefix), and begin() lays them out in ONE block of the
// stream's scratch set (StagePlan), grows the block, enters the set and enqueues one copy in per array, straight from the caller's
// memory (pinned or pageable).  The entry then enqueues its launches on dev() pointers -- through the same function as its _dev
// twin -- and finish() enqueues one copy out per output, leaves the set and waits for the stream.  The block grows BEFORE the set
// is entered: Block::grow(WAIT_DEVICE) waits for the whole device itself before it frees a block, so the order carries no dependency.
static_assert(STAGE_MAX_ARRAYS == BJJ_MAX_BASES + 1, "stage_plan.hpp: room for the largest site, bjj_mul_bases");
struct Staged {
  bjj_ctx* c;
  const char* who;
  hipStream_t st;
  ScratchSet* S;
  StagePlan plan;
  void* host[STAGE_MAX_ARRAYS] = {};
  bool absent[STAGE_MAX_ARRAYS] = {};
  uint8_t* blk = nullptr;
  Staged(bjj_ctx* c_, const char* who_, size_t prefix = 0) : c(c_), who(who_), st(c_->stream), S(pick_set(c_, c_->stream)), plan(prefix) {}
  int note(int i, const void* h, bool gone = false) { if (i >= 0) { host[i] = const_cast<void*>(h); absent[i] = gone; } return i; }
  int in(const void* h, size_t count, size_t width) { return note(plan.add(false, count, width), h); }
  int out(void* h, size_t count, size_t width) { return note(plan.add(true, count, width), h); }
  int in_opt(const void* h, size_t count, size_t width) { return note(plan.add(false, h ? count : 0, width), h, !h); }
  int out_opt(void* h, size_t count, size_t width) { return note(plan.add(true, h ? count : 0, width), h, !h); }
  int in_at(size_t off, const void* h, size_t bytes) { return note(plan.at(false, off, bytes), h); }
  int out_at(size_t off, void* h, size_t bytes) { return note(plan.at(true, off, bytes), h); }
  uint8_t* dev(int i) const { return absent[i] ? nullptr : blk + plan.a[i].off; }
  int copy(bool outputs) {   // in declaration order; an array of zero bytes has no copy
    for (int i = 0; i < plan.n; i++) {
      const StagePlan::Array& a = plan.a[i];
      if (a.out != outputs || !a.bytes) continue;
      if (outputs) HIPCK(hipMemcpyAsync(host[i], blk + a.off, a.bytes, hipMemcpyDeviceToHost, st));
      else HIPCK(hipMemcpyAsync(blk + a.off, host[i], a.bytes, hipMemcpyHostToDevice, st));
    }
    return BJJ_OK;
  }
  // noun: what the out-of-memory message calls the block; round_last: the site allocates its last array rounded up to 256 too
  int begin(DevBlock<uint8_t>& block, const char* noun, bool round_last = false) {
    { int rc = grow_block(block, plan.total(round_last), who, noun); if (rc) return rc; }
    { int rc = set_enter(c, S, st); if (rc) return rc; }
    blk = block;
    return copy(false);
  }
  int finish() {
    { int rc = copy(true); if (rc) return rc; }
    { int rc = set_leave(c, S, st); if (rc) return rc; }
    HIPCK(hipStreamSynchronize(st));
    return BJJ_OK;
  }
};
// Counts violated conditions on the device: `words` zeroed 64-bit counters, launch(d_counters) enqueues the checker (and what it has
// to run behind) on the context's stream, the counters come back in h[] -- or the HIP error does, behind "who: ".
template <typename Launch>
static int device_counters(bjj_ctx* c, int words, unsigned long long* h, const char* who, Launch launch) {
  DevBlock<unsigned long long> d;
  const size_t bytes = (size_t)words * sizeof(unsigned long long);
  hipError_t e = d.grow(bytes, NO_WAIT);
  if (e == hipSuccess) e = hipMemsetAsync(d, 0, bytes, c->stream);
  if (e == hipSuccess) e = launch(d.p);
  if (e == hipSuccess) e = hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return set_err(BJJ_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
  return BJJ_OK;
}

// Streams, events and the copy workers; the blocks release themselves when the context is deleted -- here, with its device current
// and idle (the wiped ones zero themselves first: Block::wipe).
static void ctx_destroy(bjj_ctx* c) {
  DeviceGuard dg_(c->device);
  hipDeviceSynchronize();
  for (ScratchSet& S : c->set) {
    if (S.ev_scan_in) hipEventDestroy(S.ev_scan_in);
    if (S.ev_scan_out) hipEventDestroy(S.ev_scan_out);
    if (S.scan_stream) hipStreamDestroy(S.scan_stream);
    if (S.ev_last) hipEventDestroy(S.ev_last);
  }
  for (StreamMark& k : c->marks) if (k.ev) hipEventDestroy(k.ev);
  c->user_bases.clear(); c->user_sets.clear(); c->user_dlogs.clear();   // tables, signer sets and logarithm tables the caller never freed
  delete c->pool;   // joins the copy workers
  c->pool = nullptr;
  for (hipEvent_t e : c->ev_in) hipEventDestroy(e);
  for (hipEvent_t e : c->ev_out) hipEventDestroy(e);
  if (c->ev_tail) hipEventDestroy(c->ev_tail);
  for (hipEvent_t e : c->ev_k) hipEventDestroy(e);
  for (hipEvent_t e : c->ev_mid) hipEventDestroy(e);
  if (c->s_in) hipStreamDestroy(c->s_in);
  if (c->s_out) hipStreamDestroy(c->s_out);
  if (c->stream2) hipStreamDestroy(c->stream2);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
}

extern "C" {
#pragma GCC visibility push(default)

const char* bjj_version(void) { return BJJ_VERSION_STRING; }
const char* bjj_last_error(void) { return g_err.c_str(); }

int bjj_init(int device, int window_bits, bjj_ctx** out_ctx) {
  if (!out_ctx) return set_err(BJJ_E_INVALID, "bjj_init: out_ctx is NULL");
  *out_ctx = nullptr;
  if (window_bits != 0 && window_bits != BJJ_WINDOW_AUTO && (window_bits < 4 || window_bits > BJJ_MAX_WINDOW_BITS))
    return set_err(BJJ_E_INVALID, "bjj_init: window_bits must be 0 (default, 23), BJJ_WINDOW_AUTO (-1) or 4..28");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return set_err(BJJ_E_NO_DEVICE, "bjj_init: no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return set_err(BJJ_E_INVALID, "bjj_init: device index out of range");
  ENTER_DEVICE(device);
  const auto t0 = std::chrono::steady_clock::now();
  hipDeviceProp_t prop;
  HIPCK(hipGetDeviceProperties(&prop, device));
  bjj_ctx* c = new (std::nothrow) bjj_ctx();
  if (!c) return set_err(BJJ_E_NOMEM, "bjj_init: out of host memory");
  c->device = device;
  c->cus = prop.multiProcessorCount;
  // key-derived material passes through these blocks (scalar keys in the codec records, keys in the staging levels): zeroed before they are freed
  c->dstage.wipe = true;
  for (ScratchSet& S : c->set) S.codec.wipe = S.bases_io.wipe = true;
  for (int b = 0; b < BJJ_PIPE_BUFS; b++) c->pin_in[b].wipe = c->pin_out[b].wipe = true;
  const bool autow = window_bits == BJJ_WINDOW_AUTO;
  int W = window_bits == 0 ? BJJ_DEFAULT_WINDOW_BITS : window_bits;
  if (autow) {  // widest table that leaves 40 % of the free memory to the caller (a second context gets 26 bits)
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    W = kAutoWindowBits[sizeof(kAutoWindowBits) / sizeof(int) - 1];
    for (int cand : kAutoWindowBits) {
      const size_t need = fixed_stride(cand) * (size_t)fixed_nwin(cand) * NIELS_WORDS * sizeof(u32);
      if (need <= free_b / 5 * 3) { W = cand; break; }
    }
  }
  c->W = W;
  c->nwin = fixed_nwin(W);
  c->lanes_fixed = bjjk::fixed_base_lanes_per_cu(0);
  c->lanes_fixed_2x256 = bjjk::fixed_base_lanes_per_cu(1);
  c->lanes_bases = bjjk::bases_lanes_per_cu();
  c->lanes_elgamal = bjjk::elgamal_lanes_per_cu();
  c->lanes_dleq = bjjk::dleq_lanes_per_cu();
  c->occ_dleq_respond = bjjk::occ_dleq_respond();
  c->lanes_signer = bjjk::signer_lanes_per_cu();
  c->lanes_set = bjjk::set_lanes_per_cu();
  c->dlog_launch_steps = dlog_launch_steps_from_env();
  c->common_form = common_form_from_env();
  if (const char* e = getenv("BJJ_VERIFY_DISPATCH")) {
    if (e[0] == '0' || e[0] == '1') c->verify_mode = e[0] - '0';
  }
  if (const char* e = getenv("BJJ_K2_VARIANT")) {
    if (e[0] == '0' || e[0] == '1') c->k2_variant = e[0] - '0';
  }
  if (const char* e = getenv("BJJ_FB_QUAD_MAX")) {  // tests / A-B
    char* q = nullptr; const unsigned long long v = strtoull(e, &q, 0);
    if (q != e && v <= ((unsigned long long)1 << 20)) c->fb_quad_max = (size_t)v;
  }
  if (const char* e = getenv("BJJ_SIGN_SMALL_MAX")) {  // tests / A-B
    char* q = nullptr; const unsigned long long v = strtoull(e, &q, 0);
    if (q != e && v <= ((unsigned long long)1 << 20)) c->sign_small_max = (size_t)v;
  }
  if (const char* e = getenv("BJJ_VERIFY_SMALL_MAX")) {  // tests / A-B
    char* q = nullptr; const unsigned long long v = strtoull(e, &q, 0);
    if (q != e && v <= ((unsigned long long)1 << 20)) c->verify_small_max = (size_t)v;
  }
  if (const char* e = getenv("BJJ_P5_COOP_MAX")) {  // tests / A-B
    char* q = nullptr; const unsigned long long v = strtoull(e, &q, 0);
    if (q != e && v <= ((unsigned long long)1 << 20)) c->p5_coop_max = (size_t)v;
  }
  if (const char* e = getenv("BJJ_VB_QUAD_MAX")) {  // tests / A-B: variable-base calls of at most this many items run four lanes per item (0 = never)
    char* q = nullptr; const unsigned long long v = strtoull(e, &q, 0);
    if (q != e && v <= ((unsigned long long)1 << 20)) c->vb_quad_max = (size_t)v;
  }
  if (const char* e = getenv("BJJ_K1_VARIANT")) {   // tests / A-B: force one shape of the fixed-base kernel
    if (e[0] == '0' || e[0] == '1') c->k1_variant = e[0] - '0';
  }
  if (const char* e = getenv("BJJ_K1_OVERLAP_SLOTS")) {   // tests / A-B: workgroup slots per CU of a two-workgroup-shape launch on device pointers
    if (e[0] == '1' || e[0] == '2') c->k1_overlap_slots = e[0] - '0';
  }
  if (const char* e = getenv("BJJ_VB_SPLIT")) {     // tests / A-B: K6 always behind K2 (0) or always beside it, behind a scan (1)
    if (e[0] == '0' || e[0] == '1') c->vb_split = e[0] - '0';
  }
  c->occ_vb_scan = bjjk::occ_var_base_scan();
  c->lanes_var = bjjk::var_base_lanes_per_cu();
  // the table form of the shared-scalar kernel pops K2's slot queue: it must not have more workgroups resident than K2 has slots
  if (bjjk::common_scalar_table_blocks_per_cu() * bjjk::var_base_block() > c->lanes_var) c->common_form = CS_FORM_NAF;
  c->occ_poseidon = bjjk::occ_poseidon5();
  c->occ_verify = bjjk::occ_verify();
  c->occ_scan = bjjk::occ_verify_scan();
  c->occ_add = bjjk::occ_point_add();
  c->occ_decomp = bjjk::occ_decompress();
  c->occ_sign = bjjk::occ_sign();
  c->occ_sign_schnorr = bjjk::occ_sign_schnorr();
  hipError_t se = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (se == hipSuccess) se = c->vb_seen.grow((BJJ_SCRATCH_SETS + 1) * sizeof(u32), NO_WAIT);
  if (se != hipSuccess) { (void)hipGetLastError(); ctx_destroy(c); return set_err(BJJ_E_HIP, std::string("bjj_init: stream/event: ") + hipGetErrorString(se)); }
  memset(c->vb_seen, 0, c->vb_seen.bytes);
  { const int rc_ = ensure_pipe_streams(c); if (rc_) { ctx_destroy(c); return rc_; } }   // the hardware-queue plan of the context, fixed now
  {  // XCDs of this device (the verify kernels keep one queue of table slots per XCD)
    DevBlock<u32> d_word;
    if (d_word.grow(sizeof(u32), NO_WAIT) == hipSuccess) {
      const int x = bjjk::probe_xccs(c->stream, d_word);
      c->xccs = x >= 1 && x <= 16 ? x : 1;
    }
  }
  const char* env_uncached = getenv("BJJ_TABLE_UNCACHED");   // "1" / "0"; anything else = the default (plain)
  const bool want_uncached = env_uncached && env_uncached[0] == '1';
  for (;;) {
    const size_t table_bytes = fixed_stride(c->W) * (size_t)c->nwin * NIELS_WORDS * sizeof(u32);
    // BJJ_TABLE_UNCACHED=1 (internal switch, A/B of the gather's cache behaviour): the table, and only it, as fine-grained
    // "uncached" device memory.  The build and the check kernels access it with ordinary stores and loads either way.
    c->table_alloc = BJJ_TABLE_ALLOC_PLAIN;
    se = hipErrorUnknown;
    if (want_uncached) {
      se = hipExtMallocWithFlags((void**)&c->table.p, table_bytes, hipDeviceMallocUncached);   // released with hipFree like any other
      if (se == hipSuccess) { c->table.bytes = table_bytes; c->table_alloc = BJJ_TABLE_ALLOC_UNCACHED; }
      else { (void)hipGetLastError(); c->table.p = nullptr; c->table_alloc = BJJ_TABLE_ALLOC_UNCACHED_FELL_BACK; }
    }
    if (se != hipSuccess) se = c->table.grow(table_bytes, NO_WAIT);
    if (se == hipSuccess || !autow) break;
    (void)hipGetLastError();   // auto mode: the free-memory estimate was too optimistic, take the next narrower table
    int next = 0;
    for (int cand : kAutoWindowBits) if (cand < c->W) { next = cand; break; }
    if (!next) break;
    c->W = W = next;
    c->nwin = fixed_nwin(W);
  }
  if (se == hipSuccess) se = c->bases.grow((size_t)c->nwin * NIELS_WORDS * sizeof(u32), NO_WAIT);
  if (se != hipSuccess) {
    (void)hipGetLastError();
    ctx_destroy(c);
    return set_err(BJJ_E_NOMEM, "bjj_init: cannot allocate the fixed-base table");
  }
  se = bjjk::build_fixed_table(c->stream, c->table, c->bases, c->W, c->nwin);
  if (se == hipSuccess) se = hipStreamSynchronize(c->stream);
  if (se != hipSuccess) {
    ctx_destroy(c);
    return set_err(BJJ_E_HIP, std::string("bjj_init: table build failed: ") + hipGetErrorString(se));
  }
  c->init_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out_ctx = c;
  return BJJ_OK;
}

void bjj_free(bjj_ctx* c) {
  if (!c) return;
  ctx_destroy(c);
}

// waits for everything the context has enqueued, on its own stream and on the callers' (the context's device is current)
static int ctx_wait_enqueued(bjj_ctx* c) {
  for (ScratchSet& S : c->set)      // work enqueued on a caller's stream
    if (S.have_last && S.last_stream != c->stream) HIPCK(hipEventSynchronize(S.ev_last));
  for (StreamMark& k : c->marks)
    if (k.used) HIPCK(hipEventSynchronize(k.ev));
  HIPCK(hipStreamSynchronize(c->stream));
  return BJJ_OK;
}
int bjj_sync(bjj_ctx* c) {
  if (!c) return set_err(BJJ_E_INVALID, "bjj_sync: ctx is NULL");
  ENTER_DEVICE(c->device);
  { int rc = ctx_wait_enqueued(c); if (rc) return rc; }
  // everything the context enqueued has run: a slot-queue pop that gave up waiting (slot_queue.hpp) is an ERROR of the launches
  // just completed -- reported here instead of a hung GPU; the rings are rebuilt so that the context stays usable
  return ctx_check_slot_queues(c, "bjj_sync");
}
void* bjj_stream(bjj_ctx* c) { return c ? (void*)c->stream : nullptr; }

// Sizes the first `sets` scratch sets for n items (the codec records only on request).  bjj_reserve is the public form: set 0
// plus whatever a second stream has already brought into use.  The multi-GPU pipeline calls this with sets = 2 before it
// enqueues anything when a peer's block travels in more than one piece -- pieces alternate over two streams, and the second
// set must not be allocated (hipMalloc, a synchronous copy of the slot queues) in the middle of the pipeline.
static int reserve_sets(bjj_ctx* c, size_t n, int sets, bool with_codec) {
  ENTER_DEVICE(c->device);
  int k = 0;
  for (ScratchSet& S : c->set) {
    const bool wanted = k < sets || S.have_last;
    k++;
    if (!wanted) continue;
    int rc = ensure_scratch(c, &S, n ? n : 1); if (rc) return rc;
    if (with_codec) { rc = ensure_codec(&S, n ? n : 1); if (rc) return rc; }
  }
  return BJJ_OK;
}
int bjj_reserve(bjj_ctx* c, size_t n) {
  if (!c) return set_err(BJJ_E_INVALID, "bjj_reserve: ctx is NULL");
  return reserve_sets(c, n, 1, true);
}
// ---- pinned host memory for the host-pointer entry points (include/bjj_hip.h) ----------------------------------------------
int bjj_host_alloc(bjj_ctx* c, size_t bytes, void** out) {
  if (!c || !out) return set_err(BJJ_E_INVALID, "bjj_host_alloc: NULL argument");
  *out = nullptr;
  if (!bytes) return set_err(BJJ_E_INVALID, "bjj_host_alloc: zero bytes");
  ENTER_DEVICE(c->device);
  void* p = nullptr;
  const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocPortable);
  if (e != hipSuccess) { (void)hipGetLastError(); return set_err(BJJ_E_NOMEM, std::string("bjj_host_alloc: ") + hipGetErrorString(e)); }
  try {
    std::lock_guard<std::mutex> lk(g_host_mu);
    g_host_ranges.push_back({(uintptr_t)p, (uintptr_t)p + bytes, true});
  } catch (...) { hipHostFree(p); return set_err(BJJ_E_NOMEM, "bjj_host_alloc: out of host memory"); }
  *out = p;
  return BJJ_OK;
}
static int host_range_drop(void* p, bool owned, const char* who) {
  std::lock_guard<std::mutex> lk(g_host_mu);
  for (size_t i = 0; i < g_host_ranges.size(); i++)
    if (g_host_ranges[i].lo == (uintptr_t)p && g_host_ranges[i].owned == owned) {
      g_host_ranges.erase(g_host_ranges.begin() + (long)i);
      return BJJ_OK;
    }
  return set_err(BJJ_E_INVALID, std::string(who) + ": not a pointer this library " + (owned ? "allocated" : "registered"));
}
int bjj_host_free(bjj_ctx* c, void* p) {
  if (!c) return set_err(BJJ_E_INVALID, "bjj_host_free: ctx is NULL");
  if (!p) return BJJ_OK;
  { int rc = host_range_drop(p, true, "bjj_host_free"); if (rc) return rc; }
  ENTER_DEVICE(c->device);
  HIPCK(hipHostFree(p));
  return BJJ_OK;
}
int bjj_host_register(bjj_ctx* c, void* p, size_t bytes) {
  if (!c || !p || !bytes) return set_err(BJJ_E_INVALID, "bjj_host_register: NULL argument or zero bytes");
  ENTER_DEVICE(c->device);
  const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterPortable);
  if (e != hipSuccess) { (void)hipGetLastError(); return set_err(BJJ_E_HIP, std::string("bjj_host_register: ") + hipGetErrorString(e)); }
  try {
    std::lock_guard<std::mutex> lk(g_host_mu);
    g_host_ranges.push_back({(uintptr_t)p, (uintptr_t)p + bytes, false});
  } catch (...) { hipHostUnregister(p); return set_err(BJJ_E_NOMEM, "bjj_host_register: out of host memory"); }
  return BJJ_OK;
}
int bjj_host_unregister(bjj_ctx* c, void* p) {
  if (!c) return set_err(BJJ_E_INVALID, "bjj_host_unregister: ctx is NULL");
  if (!p) return BJJ_OK;
  { int rc = host_range_drop(p, false, "bjj_host_unregister"); if (rc) return rc; }
  ENTER_DEVICE(c->device);
  HIPCK(hipHostUnregister(p));
  return BJJ_OK;
}
int bjj_host_is_pinned(bjj_ctx* c, const void* p, size_t bytes) {
  if (!c || !p) return set_err(BJJ_E_INVALID, "bjj_host_is_pinned: NULL argument");
  ENTER_DEVICE(c->device);
  return host_range_pinned(p, bytes) ? 1 : 0;
}

int bjj_get_info(bjj_ctx* c, bjj_info* out) {
  if (!c || !out) return set_err(BJJ_E_INVALID, "bjj_get_info: NULL argument");
  const size_t cap = out->struct_size;
  if (cap < 8) return set_err(BJJ_E_INVALID, "bjj_get_info: set info.struct_size = sizeof(bjj_info) before the call");
  bjj_info full;
  memset(&full, 0, sizeof(full));
  bjj_info* info = &full;
  info->device = c->device;
  info->compute_units = c->cus;
  info->window_bits = c->W;
  info->n_windows = c->nwin;
  info->table_bytes = c->table.bytes;
  info->scratch_bytes = (uint64_t)c->dstage.bytes;
  for (const ScratchSet& S : c->set) info->scratch_bytes += S.scratch.bytes + S.vb_tables.bytes + S.slow.bytes + S.codec.bytes + S.xy.bytes;
  info->kernel_fixed_base = "bjj_k_mul_fixed_base";
  info->kernel_var_base = "bjj_k_mul_var_base_tiles";   // the form a launch that runs alone gets (k_var.hip)
  info->kernel_poseidon5 = "bjj_k_poseidon5";
  info->kernel_verify = "bjj_k_eddsa_verify_groups";
  info->init_ms = c->init_ms;
  info->signer_constant_time = c->ct_signer ? 1 : 0;
  info->last_fixed_base_shape = c->last_k1;
  info->last_var_base_form = c->last_k2;
  info->last_var_base_split = c->last_vb_split;
  info->last_host_zero_copy = c->last_host_zero_copy;
  info->last_poseidon_form = c->last_p5;
  info->last_sign_form = c->last_sign;
  info->last_verify_dispatch = c->last_verify_mode;
  info->last_host_direct_arrays = c->last_host_direct;
  info->last_host_staged_arrays = c->last_host_staged;
  info->last_host_chunks = c->last_host_chunks;
  info->host_copy_threads = c->pool ? (int)c->pool->th.size() : 0;
  info->kernel_fixed_base_overlap = "bjj_k_mul_fixed_base_2x256";   // the forms overlapping launches get (expect_overlap)
  info->kernel_var_base_overlap = "bjj_k_mul_var_base";
  info->table_alloc = c->table_alloc;
  info->last_fixed_base_slots = c->last_k1_slots;
  const size_t fill = cap < sizeof(full) ? cap : sizeof(full);   // never past the caller's struct
  full.struct_size = (uint32_t)fill;
  memcpy(out, &full, fill);
  return BJJ_OK;
}

int bjj_check_table(bjj_ctx* c, uint64_t* n_bad) {
  if (!c || !n_bad) return set_err(BJJ_E_INVALID, "bjj_check_table: NULL argument");
  ENTER_DEVICE(c->device);
  unsigned long long h = 0;
  { int rc = device_counters(c, 1, &h, "bjj_check_table", [&](unsigned long long* d_bad) {
      return bjjk::check_fixed_table(c->stream, c->cus * 8, c->table, c->bases, c->W, c->nwin, d_bad); });
    if (rc) return rc; }
  *n_bad = (uint64_t)h;
  return BJJ_OK;
}

// ---- device-pointer API ------------------------------------------------------
// item indices travel as 32-bit words in the work lists and cursors
#define CHECK_N(n) if ((n) >> 32) return set_err(BJJ_E_INVALID, "batches are limited to 2^32 - 1 items per call")
#define CHECK_CTX(c, name) if (!(c)) return set_err(BJJ_E_INVALID, name ": ctx is NULL")
#define CHECK_PTR(p, name) \
  if (!(p) || !aligned16(p)) return set_err(BJJ_E_INVALID, std::string(name) + ": NULL or not 16-byte aligned device pointer")
// Every *_dev entry selects the context's device (a second context on another GPU of the same process must not launch
// on a foreign device).  Entries that use scratch (SET_ENTER / SET_LEAVE) pick a scratch set for their stream, size it,
// order themselves behind the set's previous user and record; the others (DEV_ENTER / DEV_LEAVE) only leave a completion
// mark for bjj_sync.
#define DEV_ENTER(c, stream)                                              \
  hipStream_t st = (stream) ? (hipStream_t)(stream) : (c)->stream;        \
  ENTER_DEVICE((c)->device)
#define DEV_LEAVE(c) return mark_stream((c), st)
#define SET_ENTER(c, stream, n, with_codec)                               \
  hipStream_t st = (stream) ? (hipStream_t)(stream) : (c)->stream;        \
  ENTER_DEVICE((c)->device);                                              \
  ScratchSet* S = pick_set((c), st);                                      \
  { int rc_ = ensure_scratch((c), S, (n)); if (rc_) return rc_;           \
    if (with_codec) { rc_ = ensure_codec(S, (n)); if (rc_) return rc_; } \
    rc_ = set_enter((c), S, st); if (rc_) return rc_; }
#define SET_LEAVE(c) return set_leave((c), S, st)
#define LAUNCHCK_S(expr, who)                                                                       \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) return set_err(BJJ_E_HIP, std::string(who) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define LAUNCHCK(expr, name)                                                                        \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) return set_err(BJJ_E_HIP, std::string(name ": ") + hipGetErrorString(e_)); \
  } while (0)

static int ensure_scan_stream(ScratchSet* S) {
  if (!S->scan_stream) {
    int least = 0, greatest = 0;
    HIPCK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    static const bool normal = [] { const char* e = getenv("BJJ_SCAN_STREAM_PRIORITY"); return e && e[0] == 'n'; }();   // developer A/B
    HIPCK(hipStreamCreateWithPriority(&S->scan_stream, hipStreamNonBlocking, normal ? 0 : greatest));
    HIPCK(hipEventCreateWithFlags(&S->ev_scan_in, hipEventDisableTiming));
    HIPCK(hipEventCreateWithFlags(&S->ev_scan_out, hipEventDisableTiming));
  }
  return BJJ_OK;
}
// compressed: d_out holds 32-byte Point::compress records (src/lib.rs:166-178), the compression fused into K1's epilogue
static int fixed_base_launch(bjj_ctx* c, const void* d_scalars, size_t n, void* d_out, void* stream, bool compressed, const char* who) {
  if (!c) return set_err(BJJ_E_INVALID, std::string(who) + ": ctx is NULL");
  if (n == 0) return BJJ_OK;
  CHECK_N(n);
  if (!d_scalars || !d_out || !aligned16(d_scalars) || !aligned16(d_out))
    return set_err(BJJ_E_INVALID, std::string(who) + ": NULL or not 16-byte aligned device pointer");
  if (n <= c->fb_quad_max && c->k1_variant < 0) {   // short calls (a single B8.mul_scalar is one): four lanes per item, no scratch (k_small.hip)
    DEV_ENTER(c, stream);
    c->last_k1 = 2; c->last_k1_slots = 0;
    LAUNCHCK_S(bjjk::mul_fixed_base_quad(st, c->table, c->W, c->nwin, (const uint8_t*)d_scalars, n, (uint8_t*)d_out, compressed), who);
    DEV_LEAVE(c);
  }
  SET_ENTER(c, stream, n, false);
  if (compressed) { int rc_ = ensure_xy(S, n); if (rc_) return rc_; }
  const int kv = fixed_base_variant(c, S);
  LAUNCHCK(bjjk::mul_fixed_base(st, c->cus, fixed_base_lanes(c, kv), kv, c->table, c->W, c->nwin, (const uint8_t*)d_scalars, n,
                                (uint8_t*)d_out, S->scratch, compressed ? S->xy : nullptr), "bjj_mul_fixed_base_dev");
  SET_LEAVE(c);
}
int bjj_mul_fixed_base_dev(bjj_ctx* c, const void* d_scalars, size_t n, void* d_out, void* stream) {
  return fixed_base_launch(c, d_scalars, n, d_out, stream, false, "bjj_mul_fixed_base_dev");
}
int bjj_mul_fixed_base_compressed_dev(bjj_ctx* c, const void* d_scalars, size_t n, void* d_out32, void* stream) {
  return fixed_base_launch(c, d_scalars, n, d_out32, stream, true, "bjj_mul_fixed_base_compressed_dev");
}
// Off-curve points (k_var.hip): which form does this call take?  Forced by BJJ_VB_SPLIT, else by what K6 found in the calls that have
// COMPLETED so far (K6 writes its item count into the set's pinned word; a call that is still in flight has not reported yet, so a
// caller that enqueues many launches without synchronising gets one form for all of them).
static bool vb_want_split(const bjj_ctx* c) {
  if (c->vb_split >= 0) return c->vb_split == 1;
  u32 any = 0;
  for (int k = 0; k <= BJJ_SCRATCH_SETS; k++) any |= __atomic_load_n(&c->vb_seen[k], __ATOMIC_RELAXED);
  return any != 0;
}
static int var_base_check(bjj_ctx* c, const void* d_pts, const void* d_scalars, size_t scalar_bytes, size_t n, void* d_out, const char* who) {
  if (!c) return set_err(BJJ_E_INVALID, std::string(who) + ": ctx is NULL");
  if (scalar_bytes == 0 || (scalar_bytes & 31) || scalar_bytes > BJJ_MAX_SCALAR_BYTES)
    return set_err(BJJ_E_INVALID, std::string(who) + ": scalar_bytes must be a multiple of 32 in 32..BJJ_MAX_SCALAR_BYTES");
  if (n >> 32) return set_err(BJJ_E_INVALID, "batches are limited to 2^32 - 1 items per call");
  if (n && (!d_pts || !d_scalars || !d_out || !aligned16(d_pts) || !aligned16(d_scalars) || !aligned16(d_out)))
    return set_err(BJJ_E_INVALID, std::string(who) + ": NULL or not 16-byte aligned device pointer");
  return BJJ_OK;
}
// k_var.hip: the two forms of K2 -- tiles for a launch that runs alone, grid-strided for overlapping launches (expect_overlap).
// A large launch queues behind the other sets and runs alone (tiles).
static int var_base_form(bjj_ctx* c, ScratchSet* S, hipStream_t st, size_t n, int* kv_out) {
  bool overlap = c->k2_variant < 0 && expect_overlap(c, S);
  if (overlap && n > BJJ_LARGE_LAUNCH) { int rc_ = wait_for_other_sets(c, S, st); if (rc_) return rc_; overlap = false; }
  const int kv = c->k2_variant >= 0 ? c->k2_variant : (overlap ? 0 : 1);
  c->last_k2 = kv;
  if (kv == 1) c->rings_used = true;      // the tiles take their table scratch from the slot queues
  *kv_out = kv;
  static const bool trace = [] { const char* e = getenv("BJJ_PIPE_TRACE"); return e && e[0] == '1'; }();
  if (trace) fprintf(stderr, "[k2] %zu items on set %d: %s\n", n, (int)(S - c->set), kv ? "tiles" : "grid-strided");
  return BJJ_OK;
}
// One device-pointer call.  Clean batches (every point on the curve -- what the history says): K2 makes the list of the items it
// skips, K6 follows on the caller's stream and finds it empty: nothing extra.  Once a completed call has met an off-curve point:
//   caller's stream:   ------------------------- K2 (skips them, no list) ------------------------ wait --
//   priority stream:   wait -- scan (the list) -- K6 (its ~4.5 ms serial chains, a few waves) ---- record
// so that the malformed items cost their share of the chip instead of a launch-long tail: one off-curve point in 4 096 was +30 % on
// a 2^20-item launch with K6 behind K2 (profiles/r05_var_base_offcurve.txt); beside it, see profiles/r06_var_base_offcurve.txt.
static int var_base_launch(bjj_ctx* c, const void* d_pts, const void* d_scalars, size_t scalar_bytes, size_t n, void* d_out,
                           void* stream, const char* who) {
  { int rc_ = var_base_check(c, d_pts, d_scalars, scalar_bytes, n, d_out, who); if (rc_) return rc_; }
  if (n == 0) return BJJ_OK;
  SET_ENTER(c, stream, n, false);
  // Short calls (a single Point::mul_scalar is one): four lanes per item (k_small.hip) -- 0.50 ms per call up to 2^12 items, 0.56 ms at 2^14, against
  // K2's 1.15-1.22 ms, which is one lane's serial chain whatever the call's size; from 2^15 items on K2 is ahead (1.27 vs 1.38 ms;
  // profiles/r06_small_calls.txt).  32-byte scalars; off-curve points go to K6 as from K2.
  const bool quad = scalar_bytes == 32 && n <= c->vb_quad_max && c->k2_variant < 0;   // (BJJ_K2_VARIANT forces K2, in that form)
  int kv = 2;
  if (quad) c->last_k2 = 2;
  else { int rc_ = var_base_form(c, S, st, n, &kv); if (rc_) return rc_; }
  const uint8_t* pts = (const uint8_t*)d_pts;
  const uint8_t* sc = (const uint8_t*)d_scalars;
  const int sc_words = (int)(scalar_bytes / 4);
  u32* seen = &c->vb_seen[S - c->set];
  const bool split = vb_want_split(c);
  c->last_vb_split = split ? 1 : 0;
  if (split) {
    { int rc_ = ensure_scan_stream(S); if (rc_) return rc_; }
    hipStream_t xs = S->scan_stream;   // (the copy streams or the second lane instead: no difference, profiles/r06_var_base_beside_ab.txt)
    HIPCK(hipEventRecord(S->ev_scan_in, st));
    HIPCK(hipStreamWaitEvent(xs, S->ev_scan_in, 0));
    LAUNCHCK(bjjk::var_base_list_reset(xs, S->slow), "variable-base list");
    LAUNCHCK(bjjk::var_base_scan(xs, grid_for(c, n, c->occ_vb_scan, 64), pts, 0, n, S->slow), "variable-base scan");
    LAUNCHCK(bjjk::mul_var_base_exact(xs, c->cus * 4, pts, sc, sc_words, (uint8_t*)d_out, S->slow, nullptr, seen), "variable-base (exact)");
    HIPCK(hipEventRecord(S->ev_scan_out, xs));
  }
  if (quad) {
    if (!split) HIPCK(hipMemsetAsync(S->slow, 0, 8 * sizeof(u32), st));
    LAUNCHCK_S(bjjk::mul_var_base_quad(st, pts, sc, n, (uint8_t*)d_out, split ? nullptr : S->slow), who);
  } else
  LAUNCHCK_S(bjjk::mul_var_base_main(st, c->cus, c->lanes_var, kv, pts, sc, sc_words, n, (uint8_t*)d_out, S->scratch, S->vb_tables, split ? nullptr : S->slow,
                                     S->slotq2, S->slot_cap2 | ((u32)c->xccs << 16)), who);
  if (split) HIPCK(hipStreamWaitEvent(st, S->ev_scan_out, 0));
  else LAUNCHCK(bjjk::mul_var_base_exact(st, c->cus * 4, pts, sc, sc_words, (uint8_t*)d_out, S->slow, nullptr, seen), "variable-base (exact)");
  SET_LEAVE(c);
}
// ---- the exact list of the host-pointer pipeline (ExactListStage, declared beside PipeSpec) ----------------------------------------
// Before it, variable base ran K6 behind K2 in EVERY chunk's lane -- one off-curve point in 4 096 cost 2^20 items on pinned memory +71 %
// (15.9 -> 27.3 ms, profiles/r05_var_base_offcurve.txt) -- and a verify chunk carried its own exact groups: it lasted at least as long as
// they do, 6.6 ms for the first 2^15 items instead of 2.3, and the next chunk of its lane waited behind it; 2^20 verifications of
// BASELINE configs[3] (1 in 64 corrupted, half of those off the curve) took 25 ms on pinned host memory against 18.7 ms on device
// pointers (profiles/r05_host_verify_exact_split.txt).  Per kind:
//   VAR_BASE           scan: the on-curve scan of the chunk's points.  Bulk: K2, which skips an off-curve item by itself and never writes
//                      its slot.  Exact: ONE K6 launch, its results COMPACT beside the list (d_extra) -- a chunk's outputs leave the device
//                      when its K2 is done, long before K6 is -- which the host lays over their slots (finish).  Zero-copy outputs: K6
//                      stores straight into the caller's mapped array, and d_extra is K2's phase-1 stash.
//   VERIFY             scan: the on-curve scan of pk and R.  Bulk: a bulk workgroup recognises and skips an off-curve item by itself.
//                      Exact: ONE launch whose few workgroups take the next slots that free up; it shares the first scratch set's slot
//                      queue with that set's bulk launches -- the queue holds a slot for every workgroup that can be resident, whatever
//                      launch it belongs to.  The verdicts leave once, after both (PipeSpec::out_at_end: 1 byte per item).
//   VERIFY_COMPRESSED  as VERIFY, on what the chunk's decompressions wrote to d_extra (162 B per item).  After the exact launch ONE pass
//                      writes verdict 2 where pk or R did not decompress (such an item decompresses to (0, 0), which is off the curve: it
//                      is on the list).  The bulk launches write verdict 0 for every item with msg > Q, whatever its points, so the pass
//                      runs behind them as well -- as on device pointers, where it follows the launch on the caller's stream.
int ExactListStage::open(size_t n_, void* const* d_in, void* const* d_out, uint8_t* extra, bool zc) {
  n = n_;
  for (int i = 0; i < 4; i++) in[i] = (uint8_t*)d_in[i];
  out = (uint8_t*)d_out[0];
  d_extra = extra;
  zero_copy = zc;
  if (kind == VERIFY) { pk = in[0]; r = in[1]; s = in[2]; msg = in[3]; }
  if (kind == VERIFY_COMPRESSED) { pk = d_extra; r = pk + n * 64; s = r + n * 64; f_pk = s + n * 32; f_r = f_pk + n; msg = in[2]; }
  ScratchSet* S = &c->set[0];
  { int rc_ = ensure_scan_stream(S); if (rc_) return rc_; }
  if (kind != VAR_BASE) {
    // the verifiers' exact launch works in this set's tables without being one of its calls (set_enter / set_leave): whatever used the set
    // last on another stream -- a variable-base launch a caller has enqueued and not waited for lays ITS tables over the same memory --
    // must be done first.  Afterwards only this call's own bulk launches touch the set (slot queue), and the call does not return before
    // the exact launch has completed (ev_tail).
    int rc_ = ensure_scratch(c, S, 1); if (rc_) return rc_;      // the set's tables and slot queues exist
    rc_ = set_enter(c, S, S->scan_stream); if (rc_) return rc_;
  }
  HIPCK(c->pipe_wl.grow(list_bytes(n)));
  if (kind == VAR_BASE) LAUNCHCK(bjjk::var_base_list_reset(S->scan_stream, c->pipe_wl), "variable-base list");
  else LAUNCHCK(bjjk::verify_list_reset(S->scan_stream, c->pipe_wl), "verify list");
  return BJJ_OK;
}
int ExactListStage::decompress(size_t lo, size_t cnt, hipStream_t lane) {
  const int g = grid_for(c, cnt, c->occ_decomp);
  LAUNCHCK(bjjk::decompress_points(lane, g, in[0] + lo * 32, 32, cnt, pk + lo * 64, f_pk + lo, nullptr), "decompress(pk)");
  LAUNCHCK(bjjk::decompress_points(lane, g, in[1] + lo * 64, 64, cnt, r + lo * 64, f_r + lo, s + lo * 32), "decompress(sig)");
  return BJJ_OK;
}
int ExactListStage::scan(size_t lo, size_t cnt, hipEvent_t ready) {
  hipStream_t xs = c->set[0].scan_stream;
  HIPCK(hipStreamWaitEvent(xs, ready, 0));
  if (kind == VAR_BASE)
    LAUNCHCK(bjjk::var_base_scan(xs, grid_for(c, cnt, c->occ_vb_scan, 64), in[0], lo, lo + cnt, c->pipe_wl), "variable-base scan");
  else
    LAUNCHCK(bjjk::verify_scan_range(xs, grid_for(c, cnt, c->occ_scan, 64) * 64 / bjjk::verify_scan_block(), pk, r, msg, lo, lo + cnt, c->pipe_wl),
             "verify scan");
  return BJJ_OK;
}
int ExactListStage::close(const hipEvent_t* bulk_done, size_t lanes) {
  ScratchSet* S = &c->set[0];
  hipStream_t xs = S->scan_stream;
  if (kind == VAR_BASE) {
    LAUNCHCK(bjjk::mul_var_base_exact(xs, c->cus * 4, in[0], in[1], sc_words, zero_copy ? out : nullptr, c->pipe_wl, zero_copy ? nullptr : d_extra,
                                      &c->vb_seen[BJJ_SCRATCH_SETS]), "variable-base (exact)");
  } else {
    c->rings_used = true;
    LAUNCHCK(bjjk::verify_main(xs, 1, 0, schnorr, c->table, c->W, c->nwin, pk, r, s, msg, n, out, S->vb_tables, c->pipe_wl, S->slotq,
                               S->slot_cap | ((u32)c->xccs << 16), bjjk::VERIFY_EXACT), "verify (exact)");
  }
  if (kind == VERIFY_COMPRESSED) {   // output bytes the bulk launches write too: behind every lane's last one
    for (size_t l = 0; l < lanes; l++) HIPCK(hipStreamWaitEvent(xs, bulk_done[l], 0));
    LAUNCHCK(bjjk::merge_codec_flags(xs, grid_for(c, n, 8), out, f_pk, f_r, n), "merge_codec_flags");
  }
  HIPCK(hipEventRecord(c->ev_tail, xs));
  return BJJ_OK;
}
int ExactListStage::finish(uint8_t* host_out) {
  if (kind != VAR_BASE || zero_copy) return BJJ_OK;
  const size_t cnt = __atomic_load_n(&c->vb_seen[BJJ_SCRATCH_SETS], __ATOMIC_ACQUIRE);   // K6 is done (ev_tail): its count is in
  if (!cnt) return BJJ_OK;
  if (cnt > n) return set_err(BJJ_E_HIP, "variable base: the exact list is longer than the batch");
  const size_t need = cnt * 68;
  if (need > c->patch_host.bytes)   // at least 64 KB, else half as much again as the need; the last call's copy has been waited for
    HIPCK(c->patch_host.grow(need < ((size_t)1 << 16) ? (size_t)1 << 16 : need + need / 2, NO_WAIT));
  HIPCK(hipMemcpyAsync(c->patch_host, d_extra, cnt * 64, hipMemcpyDeviceToHost, c->s_out));
  HIPCK(hipMemcpyAsync(c->patch_host + cnt * 64, c->pipe_wl + 8, cnt * 4, hipMemcpyDeviceToHost, c->s_out));
  HIPCK(hipStreamSynchronize(c->s_out));
  const u32* idx = (const u32*)(c->patch_host + cnt * 64);
  for (size_t j = 0; j < cnt; j++) {
    if (idx[j] >= n) return set_err(BJJ_E_HIP, "variable base: index out of range on the exact list");
    memcpy(host_out + (size_t)idx[j] * 64, c->patch_host + j * 64, 64);
  }
  return BJJ_OK;
}
// Does a host-pointer call take the split form, bulk launches per chunk beside ONE exact launch over the exact list?  Not for a call of
// fewer than first + first / 2 items: that is one chunk, a device-pointer launch with copies around it (a single `verify` or
// Point::mul_scalar, src/lib.rs:395 / 149, is such a call) -- its exact groups start first inside the launch, nothing waits behind them,
// and three launches instead of two would only add latency.  Not when the persistent verify form (BJJ_VERIFY_DISPATCH=0) or K6 behind K2
// (BJJ_VB_SPLIT=0) is forced -- one launch per chunk, exact items included -- nor when the round-5 per-chunk form is (developer, and the
// tests' cross-check: BJJ_PIPE_VERIFY_SPLIT=0 / BJJ_PIPE_VAR_BASE_SPLIT=0).
static int exact_split_applies(bjj_ctx* c, bool var_base, size_t n, size_t first_chunk, bool* split) {
  { int rc_ = ensure_pipe(c, 0, 0, 0, 0); if (rc_) return rc_; }   // the knobs: the chunk schedule of the environment
  static const bool verify_per_chunk = [] { const char* e = getenv("BJJ_PIPE_VERIFY_SPLIT"); return e && e[0] == '0'; }();
  static const bool var_base_per_chunk = [] { const char* e = getenv("BJJ_PIPE_VAR_BASE_SPLIT"); return e && e[0] == '0'; }();
  const size_t first = c->pipe_env_schedule ? c->pipe_first : first_chunk;
  const bool forced_off = var_base ? var_base_per_chunk || c->vb_split == 0 : verify_per_chunk || c->verify_mode == 0;
  *split = !forced_off && n >= first + first / 2;
  return BJJ_OK;
}
// ---- variable base through the host-pointer pipeline ---------------------------------------------------------------------------
static int var_base_bulk_launch(bjj_ctx* c, const void* d_pts, const void* d_scalars, size_t scalar_bytes, size_t n, void* d_out, uint8_t* xy, void* stream) {
  SET_ENTER(c, stream, n, false);
  // one tile per workgroup, whatever else is in flight: the chunks' launches are then work-conserving among themselves -- a
  // workgroup retires after its tile and the slot goes to whichever launch has tiles pending -- where the grid-strided form's
  // resident sets (the better form for two whole 2^20-item launches that overlap) made the call's length depend on how the chunks'
  // partly filled rounds happened to interleave (15.6 ... 18.0 ms for the same 2^20 items, profiles/r06_var_base_host_schedule.txt)
  const int kv = c->k2_variant >= 0 ? c->k2_variant : 1;
  c->last_k2 = kv;
  if (kv == 1) c->rings_used = true;
  c->last_vb_split = 1;
  LAUNCHCK(bjjk::mul_var_base_main(st, c->cus, c->lanes_var, kv, (const uint8_t*)d_pts, (const uint8_t*)d_scalars, (int)(scalar_bytes / 4), n, (uint8_t*)d_out,
                                   S->scratch, S->vb_tables, nullptr, S->slotq2, S->slot_cap2 | ((u32)c->xccs << 16), xy), "variable base (bulk)");
  SET_LEAVE(c);
}
static int var_base_host(bjj_ctx* c, const uint8_t* pts, const uint8_t* scalars, size_t scalar_bytes, size_t n, uint8_t* out) {
  PipeSpec sp = {2, 1, {pts, scalars}, {64, scalar_bytes}, {out}, {64}, false};
  if (scalar_bytes == 32 && c->k2_variant < 0) sp.small_direct_max = small_direct_items(c->vb_quad_max);
  sp.first_chunk = (size_t)1 << 16;   // 14 ms of kernels over 3 ms of copies: a 2^15-item launch holds its lane for a whole round with a quarter of the chip
  sp.max_chunk = (size_t)1 << 18;
  bool split = false;
  { int rc_ = exact_split_applies(c, true, n, sp.first_chunk, &split); if (rc_) return rc_; }
  if (!split)
    return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) { return var_base_launch(c, i[0], i[1], scalar_bytes, cnt, o[0], st, "bjj_mul_var_base"); });
  ExactListStage ex(c, ExactListStage::VAR_BASE);
  ex.sc_words = (int)(scalar_bytes / 4);
  sp.exact = &ex;
  sp.extra_dev_per_item = 64;         // K6's compact results (as many as there are items, at worst) -- or, zero-copy, K2's phase-1 stash
  sp.last_on_priority_lane = true;
  // Pinned output array: the kernels store into it themselves (64 MB of results over the 15 ms the kernels take anyway) -- no copy-out
  // stage, so nothing favours small chunks once the inputs are in: the chunks double without a cap (2^16, 2^17, 2^18, the rest), and
  // the call ends when the last tile does, like one device-pointer launch.  Pageable output: copies chunk by chunk as before, the last
  // chunk small (its copy-out is the one nothing hides).
  if (c->pipe_zero_copy && c->k2_variant != 0 && !c->force_staged && host_range_pinned(out, n * 64)) { sp.zero_copy_out = true; sp.max_chunk = (size_t)1 << 24; }   // (the stash apart exists for the tiles)
  else { sp.tail_chunk = (size_t)1 << 16; sp.max_chunk = (size_t)1 << 18; }
  return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) {
    const size_t lo = (size_t)((uint8_t*)i[0] - ex.in[0]) / 64;           // this chunk's first item within the super-batch
    return var_base_bulk_launch(c, i[0], i[1], scalar_bytes, cnt, o[0], ex.zero_copy ? ex.d_extra + lo * 64 : nullptr, st); });
}
int bjj_mul_var_base_dev(bjj_ctx* c, const void* d_pts, const void* d_scalars, size_t n, void* d_out, void* stream) {
  return var_base_launch(c, d_pts, d_scalars, 32, n, d_out, stream, "bjj_mul_var_base_dev");
}
int bjj_mul_var_base_wide_dev(bjj_ctx* c, const void* d_pts, const void* d_scalars, size_t scalar_bytes, size_t n, void* d_out,
                              void* stream) {
  return var_base_launch(c, d_pts, d_scalars, scalar_bytes, n, d_out, stream, "bjj_mul_var_base_wide_dev");
}
int bjj_poseidon5_dev(bjj_ctx* c, const void* d_in, size_t n, void* d_out, void* stream) {
  CHECK_CTX(c, "bjj_poseidon5_dev");
  if (n == 0) return BJJ_OK;
  CHECK_N(n);
  CHECK_PTR(d_in, "bjj_poseidon5_dev"); CHECK_PTR(d_out, "bjj_poseidon5_dev");
  DEV_ENTER(c, stream);
  // Short calls (a single POSEIDON.hash is one): six lanes per hash (k_small.hip) -- the permutation's dependent chain instead of all of
  // its ~1 000 multiplications in a row on one lane (profiles/r06_small_calls.txt)
  c->last_p5 = n <= c->p5_coop_max ? 1 : 0;
  if (c->last_p5) LAUNCHCK(bjjk::poseidon5_coop(st, (const uint8_t*)d_in, n, (uint8_t*)d_out), "bjj_poseidon5_dev");
  else
  LAUNCHCK(bjjk::poseidon5(st, grid_for(c, n, c->occ_poseidon), (const uint8_t*)d_in, n, (uint8_t*)d_out), "bjj_poseidon5_dev");
  DEV_LEAVE(c);
}
// scan (priority stream) -> main kernel (the caller's stream), both ordered behind what `st` has queued so far
static int enqueue_verify(bjj_ctx* c, ScratchSet* S, hipStream_t st, bool schnorr, const uint8_t* pk, const uint8_t* r, const uint8_t* s,
                          const uint8_t* msg, size_t n, uint8_t* ok) {
  { int rc_ = ensure_scan_stream(S); if (rc_) return rc_; }
  const int scan_grid = grid_for(c, n, c->occ_scan, 64) * 64 / bjjk::verify_scan_block();   // occ_scan counts waves
  // Short calls (a single `verify` is one): the bulk with eight lanes per signature (k_small.hip) between K4's scan and K4's exact
  // launch -- the hash on six lanes, the curve arithmetic on four, instead of one lane's serial chain (profiles/r06_small_calls.txt)
  if (n <= c->verify_small_max && c->verify_mode < 0) {
    c->last_verify_mode = 2;
    c->rings_used = true;               // the exact launch takes its table scratch from the slot queues
    LAUNCHCK(bjjk::verify_scan(st, scan_grid, pk, r, msg, n, S->slow), "verify scan");
    LAUNCHCK(bjjk::verify_small(st, schnorr, c->table, c->W, c->nwin, pk, r, s, msg, n, ok), "verify (short call)");
    LAUNCHCK(bjjk::verify_main(st, 1, 0, schnorr, c->table, c->W, c->nwin, pk, r, s, msg, n, ok, S->vb_tables, S->slow, S->slotq,
                               S->slot_cap | ((u32)c->xccs << 16), bjjk::VERIFY_EXACT), "verify (exact)");
    return BJJ_OK;
  }
  bool busy = expect_overlap(c, S);
  if (busy && c->verify_mode < 0 && n > BJJ_LARGE_LAUNCH) { int rc_ = wait_for_other_sets(c, S, st); if (rc_) return rc_; busy = false; }
  // k_verify.hip: persistent waves for ONE large launch that runs alone, one group per workgroup otherwise
  const int mode = c->verify_mode >= 0 ? c->verify_mode : ((!busy && n > BJJ_LARGE_LAUNCH) ? 0 : 1);
  c->last_verify_mode = mode;
  if (mode == 1) c->rings_used = true;    // one group per workgroup: table scratch from the slot queues
  // inside the host-pointer pipeline the scan stays in line: its lanes, copy streams and the scan streams would be five
  // co-active high-priority streams on four hardware queues, and a scan that lands behind the copy-out stream's wait for the
  // previous chunk's kernels would serialise the lanes
  if (busy && !(c->in_pipeline && c->pipe_scan_inline)) {   // the chip is (about to be) full of another launch's workgroups: priority stream
    HIPCK(hipEventRecord(S->ev_scan_in, st));
    HIPCK(hipStreamWaitEvent(S->scan_stream, S->ev_scan_in, 0));
    LAUNCHCK(bjjk::verify_scan(S->scan_stream, scan_grid, pk, r, msg, n, S->slow), "verify scan");
    HIPCK(hipEventRecord(S->ev_scan_out, S->scan_stream));
    HIPCK(hipStreamWaitEvent(st, S->ev_scan_out, 0));
  } else {                              // nothing to compete with: in line, no event hops
    LAUNCHCK(bjjk::verify_scan(st, scan_grid, pk, r, msg, n, S->slow), "verify scan");
  }
  LAUNCHCK(bjjk::verify_main(st, mode, grid_for(c, n, c->occ_verify, 64) * 64 / BJJ_VERIFY_BLOCK, schnorr, c->table, c->W, c->nwin, pk, r, s, msg, n, ok,
                             S->vb_tables, S->slow, S->slotq, S->slot_cap | ((u32)c->xccs << 16)), "verify");
  return BJJ_OK;
}
static int verify_launch(bjj_ctx* c, bool schnorr, const void* d_pk, const void* d_r, const void* d_s, const void* d_msg,
                         size_t n, void* d_ok, void* stream, const char* who) {
  if (!c) return set_err(BJJ_E_INVALID, std::string(who) + ": ctx is NULL");
  if (n == 0) return BJJ_OK;
  CHECK_N(n);
  if (!d_pk || !d_r || !d_s || !d_msg || !aligned16(d_pk) || !aligned16(d_r) || !aligned16(d_s) || !aligned16(d_msg))
    return set_err(BJJ_E_INVALID, std::string(who) + ": NULL or not 16-byte aligned device pointer");
  if (!d_ok) return set_err(BJJ_E_INVALID, std::string(who) + ": d_ok is NULL");
  SET_ENTER(c, stream, n, false);
  { int rc_ = enqueue_verify(c, S, st, schnorr, (const uint8_t*)d_pk, (const uint8_t*)d_r, (const uint8_t*)d_s, (const uint8_t*)d_msg, n,
                             (uint8_t*)d_ok); if (rc_) return rc_; }
  SET_LEAVE(c);
}
int bjj_eddsa_verify_dev(bjj_ctx* c, const void* d_pk, const void* d_r, const void* d_s, const void* d_msg, size_t n,
                         void* d_ok, void* stream) {
  return verify_launch(c, false, d_pk, d_r, d_s, d_msg, n, d_ok, stream, "bjj_eddsa_verify_dev");
}
// ---- the verifiers through the host-pointer pipeline -------------------------------------------------------------------------
// Items whose pk or R is off the curve take the reference's exact formula sequence, ~3x as long as a bulk item and strictly serial per
// lane (k_verify.hip): the pipeline takes them out of the chunks into the exact list (ExactListStage::VERIFY above).
static int verify_bulk_launch(bjj_ctx* c, bool schnorr, const void* d_pk, const void* d_r, const void* d_s, const void* d_msg, size_t n,
                              void* d_ok, void* stream) {
  SET_ENTER(c, stream, n, false);
  c->rings_used = true;
  c->last_verify_mode = 1;
  LAUNCHCK(bjjk::verify_main(st, 1, 0, schnorr, c->table, c->W, c->nwin, (const uint8_t*)d_pk, (const uint8_t*)d_r, (const uint8_t*)d_s,
                             (const uint8_t*)d_msg, n, (uint8_t*)d_ok, S->vb_tables, S->slow, S->slotq, S->slot_cap | ((u32)c->xccs << 16),
                             bjjk::VERIFY_BULK), "verify (bulk)");
  SET_LEAVE(c);
}
static int verify_host(bjj_ctx* c, bool schnorr, const uint8_t* pk, const uint8_t* r, const uint8_t* s, const uint8_t* msg, size_t n, uint8_t* ok) {
  PipeSpec sp = {4, 1, {pk, r, s, msg}, {64, 64, 32, 32}, {ok}, {1}, false};
  if (c->verify_mode < 0) sp.small_direct_max = small_direct_items(c->verify_small_max);
  // 18 ms of kernels against 3.9 ms of H2D for 2^20 items: the copy-out never bounds this call, what costs is the ramp (the
  // chip is part empty until the first chunks have arrived) and every launch's partly empty last round -- fewer, larger chunks
  // than the copy-bound default (2^16 / 2^19: 19.17 ms, 2^15 / 2^18: 19.36 ms; profiles/r05_host_verify_exact_split.txt)
  sp.first_chunk = (size_t)1 << 16;
  sp.max_chunk = (size_t)1 << 19;
  bool split = false;
  { int rc_ = exact_split_applies(c, false, n, sp.first_chunk, &split); if (rc_) return rc_; }
  if (!split)
    return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) {
      return schnorr ? bjj_schnorr_verify_dev(c, i[0], i[1], i[2], i[3], cnt, o[0], st) : bjj_eddsa_verify_dev(c, i[0], i[1], i[2], i[3], cnt, o[0], st); });
  ExactListStage ex(c, ExactListStage::VERIFY);
  ex.schnorr = schnorr;
  sp.exact = &ex;
  sp.out_at_end = true;
  return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) { return verify_bulk_launch(c, schnorr, i[0], i[1], i[2], i[3], cnt, o[0], st); });
}
// The wire-format verifier (round 6) used to be the device entry point per chunk: decompressions, scan and a launch that carried the chunk's
// own exact groups -- the form the plain verifiers left in round 5 -- and with the pipeline's default chunks it took 31.7 ms for 2^20
// signatures of which 1 in 64 is corrupted (39.5 ms with the 2^17-item cap of round 6) against 23.5 ms for one device-pointer launch.  Now the
// plain verifiers' form with the chunk's decompressions in front (ExactListStage::VERIFY_COMPRESSED).
static int verify_compressed_host(bjj_ctx* c, const uint8_t* pk32, const uint8_t* sig64, const uint8_t* msg, size_t n, uint8_t* ok) {
  PipeSpec sp = {3, 1, {pk32, sig64, msg}, {32, 64, 32}, {ok}, {1}, false};
  sp.first_chunk = (size_t)1 << 16;
  sp.max_chunk = (size_t)1 << 19;          // the verifiers' schedule: 23 ms of kernels hide 2.5 ms of copies several times over
  bool split = false;
  { int rc_ = exact_split_applies(c, false, n, sp.first_chunk, &split); if (rc_) return rc_; }
  if (!split)
    return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) { return bjj_eddsa_verify_compressed_dev(c, i[0], i[1], i[2], cnt, o[0], st); });
  ExactListStage ex(c, ExactListStage::VERIFY_COMPRESSED);
  sp.exact = &ex;
  sp.extra_dev_per_item = 162;             // decompressed pk (64) + R (64) + s (32) + the two decompression flags
  sp.out_at_end = true;
  return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) {   // the chunk's decompressions are on its lane already
    const size_t lo = (size_t)((uint8_t*)i[0] - ex.in[0]) / 32;
    return verify_bulk_launch(c, false, ex.pk + lo * 64, ex.r + lo * 64, ex.s + lo * 32, i[2], cnt, o[0], st); });
}
int bjj_schnorr_verify_dev(bjj_ctx* c, const void* d_pk, const void* d_r, const void* d_s, const void* d_msg, size_t n,
                           void* d_ok, void* stream) {
  return verify_launch(c, true, d_pk, d_r, d_s, d_msg, n, d_ok, stream, "bjj_schnorr_verify_dev");
}
int bjj_point_add_dev(bjj_ctx* c, const void* d_p, const void* d_q, size_t n, void* d_out, void* stream) {
  CHECK_CTX(c, "bjj_point_add_dev");
  if (n == 0) return BJJ_OK;
  CHECK_N(n);
  CHECK_PTR(d_p, "bjj_point_add_dev"); CHECK_PTR(d_q, "bjj_point_add_dev"); CHECK_PTR(d_out, "bjj_point_add_dev");
  DEV_ENTER(c, stream);
  LAUNCHCK(bjjk::point_add(st, grid_for(c, n, c->occ_add), (const uint8_t*)d_p, (const uint8_t*)d_q, n, (uint8_t*)d_out), "bjj_point_add_dev");
  DEV_LEAVE(c);
}
int bjj_proj_add_dev(bjj_ctx* c, const void* d_p, const void* d_q, size_t n, void* d_out, void* stream) {
  CHECK_CTX(c, "bjj_proj_add_dev");
  if (n == 0) return BJJ_OK;
  CHECK_N(n);
  CHECK_PTR(d_p, "bjj_proj_add_dev"); CHECK_PTR(d_q, "bjj_proj_add_dev"); CHECK_PTR(d_out, "bjj_proj_add_dev");
  DEV_ENTER(c, stream);
  LAUNCHCK(bjjk::proj_add(st, grid_for(c, n, c->occ_add), (const uint8_t*)d_p, (const uint8_t*)d_q, n, (uint8_t*)d_out), "bjj_proj_add_dev");
  DEV_LEAVE(c);
}
int bjj_proj_affine_dev(bjj_ctx* c, const void* d_p, size_t n, void* d_out, void* stream) {
  CHECK_CTX(c, "bjj_proj_affine_dev");
  if (n == 0) return BJJ_OK;
  CHECK_N(n);
  CHECK_PTR(d_p, "bjj_proj_affine_dev"); CHECK_PTR(d_out, "bjj_proj_affine_dev");
  DEV_ENTER(c, stream);
  LAUNCHCK(bjjk::proj_affine(st, grid_for(c, n, c->occ_add), (const uint8_t*)d_p, n, (uint8_t*)d_out), "bjj_proj_affine_dev");
  DEV_LEAVE(c);
}

int bjj_compress_points_dev(bjj_ctx* c, const void* d_pts, size_t n, void* d_out, void* stream) {
  CHECK_CTX(c, "bjj_compress_points_dev");
  if (n == 0) return BJJ_OK;
  CHECK_N(n);
  CHECK_PTR(d_pts, "bjj_compress_points_dev"); CHECK_PTR(d_out, "bjj_compress_points_dev");
  DEV_ENTER(c, stream);
  LAUNCHCK(bjjk::compress_points(st, grid_for(c, n, 8), (const uint8_t*)d_pts, n, (uint8_t*)d_out), "bjj_compress_points_dev");
  DEV_LEAVE(c);
}
int bjj_decompress_points_dev(bjj_ctx* c, const void* d_in, size_t n, void* d_out_xy, void* d_ok, void* stream) {
  CHECK_CTX(c, "bjj_decompress_points_dev");
  if (n == 0) return BJJ_OK;
  CHECK_N(n);
  CHECK_PTR(d_in, "bjj_decompress_points_dev"); CHECK_PTR(d_out_xy, "bjj_decompress_points_dev");
  if (!d_ok) return set_err(BJJ_E_INVALID, "bjj_decompress_points_dev: d_ok is NULL");
  DEV_ENTER(c, stream);
  LAUNCHCK(bjjk::decompress_points(st, grid_for(c, n, c->occ_decomp), (const uint8_t*)d_in, 32, n, (uint8_t*)d_out_xy, (uint8_t*)d_ok,
                                   nullptr), "bjj_decompress_points_dev");
  DEV_LEAVE(c);
}
int bjj_eddsa_verify_compressed_dev(bjj_ctx* c, const void* d_pk32, const void* d_sig64, const void* d_msg, size_t n,
                                    void* d_ok, void* stream) {
  CHECK_CTX(c, "bjj_eddsa_verify_compressed_dev");
  if (n == 0) return BJJ_OK;
  CHECK_N(n);
  CHECK_PTR(d_pk32, "bjj_eddsa_verify_compressed_dev"); CHECK_PTR(d_sig64, "bjj_eddsa_verify_compressed_dev");
  CHECK_PTR(d_msg, "bjj_eddsa_verify_compressed_dev");
  if (!d_ok) return set_err(BJJ_E_INVALID, "bjj_eddsa_verify_compressed_dev: d_ok is NULL");
  SET_ENTER(c, stream, n, true);
  uint8_t* pk_xy = S->codec;
  uint8_t* r_xy = pk_xy + n * 64;
  uint8_t* s32 = r_xy + n * 64;
  uint8_t* f_pk = s32 + n * 32;
  uint8_t* f_r = f_pk + n;
  const int g = grid_for(c, n, c->occ_decomp);
  LAUNCHCK(bjjk::decompress_points(st, g, (const uint8_t*)d_pk32, 32, n, pk_xy, f_pk, nullptr), "decompress(pk)");
  LAUNCHCK(bjjk::decompress_points(st, g, (const uint8_t*)d_sig64, 64, n, r_xy, f_r, s32), "decompress(sig)");
  { int rc_ = enqueue_verify(c, S, st, false, pk_xy, r_xy, s32, (const uint8_t*)d_msg, n, (uint8_t*)d_ok); if (rc_) return rc_; }
  LAUNCHCK(bjjk::merge_codec_flags(st, grid_for(c, n, 8), (uint8_t*)d_ok, f_pk, f_r, n), "merge_codec_flags");
  SET_LEAVE(c);
}

// ---- signer hardening ---------------------------------------------------------------------------------------------
#define BJJ_CT_W 4
static int ensure_ct_table(bjj_ctx* c) {
  if (c->ct_table) return BJJ_OK;
  ENTER_DEVICE(c->device);
  const int nwin = fixed_nwin(BJJ_CT_W);
  const size_t bytes = fixed_stride(BJJ_CT_W) * (size_t)nwin * NIELS_WORDS * sizeof(u32);
  unsigned long long bad = 1;
  const int rc = device_counters(c, 1, &bad, "constant-time signer table", [&](unsigned long long* d_bad) {
    hipError_t e = c->ct_table.grow(bytes, NO_WAIT);
    if (e == hipSuccess) e = c->ct_bases.grow((size_t)nwin * NIELS_WORDS * sizeof(u32), NO_WAIT);
    if (e == hipSuccess) e = bjjk::build_fixed_table(c->stream, c->ct_table, c->ct_bases, BJJ_CT_W, nwin);
    if (e == hipSuccess) e = bjjk::check_fixed_table(c->stream, 8, c->ct_table, c->ct_bases, BJJ_CT_W, nwin, d_bad);   // the same induction proof as the big table
    return e;
  });
  if (rc || bad != 0) {   // a table that exists is a table that passed: the next call starts over
    (void)c->ct_table.release(); (void)c->ct_bases.release();
    return rc ? rc : set_err(BJJ_E_HIP, "constant-time signer table failed its self-check");
  }
  c->occ_sign_ct = bjjk::occ_sign_ct();
  c->occ_sign_schnorr_ct = bjjk::occ_sign_schnorr_ct();
  return BJJ_OK;
}
int bjj_set_signer_constant_time(bjj_ctx* c, int on) {
  CHECK_CTX(c, "bjj_set_signer_constant_time");
  if (on) { int rc = ensure_ct_table(c); if (rc) return rc; }
  c->ct_signer = on != 0;
  return BJJ_OK;
}

int bjj_scalar_keys_dev(bjj_ctx* c, const void* d_keys, size_t n, void* d_out, void* stream) {
  CHECK_CTX(c, "bjj_scalar_keys_dev");
  if (n == 0) return BJJ_OK;
  CHECK_N(n);
  CHECK_PTR(d_keys, "bjj_scalar_keys_dev"); CHECK_PTR(d_out, "bjj_scalar_keys_dev");
  DEV_ENTER(c, stream);
  LAUNCHCK(bjjk::scalar_keys(st, grid_for(c, n, 4), (const uint8_t*)d_keys, n, (uint8_t*)d_out), "bjj_scalar_keys_dev");
  DEV_LEAVE(c);
}
// compressed: d_out holds the 32-byte records of sk.public().compress() (src/lib.rs:304-306, 166-178)
static int public_keys_launch(bjj_ctx* c, const void* d_keys, size_t n, void* d_out_xy, void* stream, bool compressed, const char* who) {
  if (!c) return set_err(BJJ_E_INVALID, std::string(who) + ": ctx is NULL");
  if (n == 0) return BJJ_OK;
  CHECK_N(n);
  if (!d_keys || !d_out_xy || !aligned16(d_keys) || !aligned16(d_out_xy))
    return set_err(BJJ_E_INVALID, std::string(who) + ": NULL or not 16-byte aligned device pointer");
  SET_ENTER(c, stream, n, true);
  if (compressed) { int rc_ = ensure_xy(S, n); if (rc_) return rc_; }
  uint8_t* xy = compressed ? S->xy : nullptr;
  // B8.mul_scalar(&self.scalar_key()), src/lib.rs:304-306; the scalar keys live in the codec scratch only for the
  // duration of the multiplication and are wiped on the same stream right behind it
  LAUNCHCK(bjjk::scalar_keys(st, grid_for(c, n, 4), (const uint8_t*)d_keys, n, S->codec), "scalar_keys");
  if (c->ct_signer) {
    LAUNCHCK(bjjk::mul_fixed_base_scan(st, c->cus, c->ct_table, BJJ_CT_W, fixed_nwin(BJJ_CT_W), S->codec, n, (uint8_t*)d_out_xy, S->scratch, xy),
             "mul_fixed_base_scan");
  } else if (n <= c->fb_quad_max && c->k1_variant < 0) {   // short calls: four lanes per key (k_small.hip)
    c->last_k1 = 2; c->last_k1_slots = 0;
    LAUNCHCK(bjjk::mul_fixed_base_quad(st, c->table, c->W, c->nwin, S->codec, n, (uint8_t*)d_out_xy, compressed), "mul_fixed_base (short call)");
  } else {
    const int kv = fixed_base_variant(c, S);
    LAUNCHCK(bjjk::mul_fixed_base(st, c->cus, fixed_base_lanes(c, kv), kv, c->table, c->W, c->nwin, S->codec, n, (uint8_t*)d_out_xy,
                                  S->scratch, xy), "mul_fixed_base");
  }
  HIPCK(hipMemsetAsync(S->codec, 0, n * 32, st));
  SET_LEAVE(c);
}
int bjj_public_keys_dev(bjj_ctx* c, const void* d_keys, size_t n, void* d_out_xy, void* stream) {
  return public_keys_launch(c, d_keys, n, d_out_xy, stream, false, "bjj_public_keys_dev");
}
int bjj_public_keys_compressed_dev(bjj_ctx* c, const void* d_keys, size_t n, void* d_out32, void* stream) {
  return public_keys_launch(c, d_keys, n, d_out32, stream, true, "bjj_public_keys_compressed_dev");
}
// d_out_s == NULL: the compressed form -- d_out_r holds 64-byte Signature::compress records (src/lib.rs:245-258)
static int sign_launch(bjj_ctx* c, const void* d_keys, const void* d_msgs, size_t n, void* d_out_r, void* d_out_s, void* d_ok, void* stream) {
  DEV_ENTER(c, stream);
  c->last_sign = (!c->ct_signer && n <= c->sign_small_max) ? 1 : 0;
  if (c->last_sign)   // short calls (a single sk.sign(msg) is one): eight lanes per signature, the hash on six of them (k_small.hip)
    LAUNCHCK(bjjk::sign_small(st, c->table, c->W, c->nwin, (const uint8_t*)d_keys, (const uint8_t*)d_msgs, n, (uint8_t*)d_out_r, (uint8_t*)d_out_s,
                              (uint8_t*)d_ok), "bjj_sign_dev (short call)");
  else
  if (c->ct_signer)
    LAUNCHCK(bjjk::sign_ct(st, grid_for(c, n, c->occ_sign_ct), c->ct_table, BJJ_CT_W, fixed_nwin(BJJ_CT_W), (const uint8_t*)d_keys,
                           (const uint8_t*)d_msgs, n, (uint8_t*)d_out_r, (uint8_t*)d_out_s, (uint8_t*)d_ok), "bjj_sign_dev (constant-time)");
  else
  LAUNCHCK(bjjk::sign(st, grid_for(c, n, c->occ_sign), c->table, c->W, c->nwin, (const uint8_t*)d_keys, (const uint8_t*)d_msgs, n,
                      (uint8_t*)d_out_r, (uint8_t*)d_out_s, (uint8_t*)d_ok), "bjj_sign_dev");
  DEV_LEAVE(c);
}
int bjj_sign_dev(bjj_ctx* c, const void* d_keys, const void* d_msgs, size_t n, void* d_out_r, void* d_out_s, void* d_ok,
                 void* stream) {
  CHECK_CTX(c, "bjj_sign_dev");
  if (n == 0) return BJJ_OK;
  CHECK_N(n);
  CHECK_PTR(d_keys, "bjj_sign_dev"); CHECK_PTR(d_msgs, "bjj_sign_dev"); CHECK_PTR(d_out_r, "bjj_sign_dev");
  CHECK_PTR(d_out_s, "bjj_sign_dev");
  if (!d_ok) return set_err(BJJ_E_INVALID, "bjj_sign_dev: d_ok is NULL");
  return sign_launch(c, d_keys, d_msgs, n, d_out_r, d_out_s, d_ok, stream);
}
int bjj_sign_compressed_dev(bjj_ctx* c, const void* d_keys, const void* d_msgs, size_t n, void* d_out_sig64, void* d_ok, void* stream) {
  CHECK_CTX(c, "bjj_sign_compressed_dev");
  if (n == 0) return BJJ_OK;
  CHECK_N(n);
  CHECK_PTR(d_keys, "bjj_sign_compressed_dev"); CHECK_PTR(d_msgs, "bjj_sign_compressed_dev"); CHECK_PTR(d_out_sig64, "bjj_sign_compressed_dev");
  if (!d_ok) return set_err(BJJ_E_INVALID, "bjj_sign_compressed_dev: d_ok is NULL");
  return sign_launch(c, d_keys, d_msgs, n, d_out_sig64, nullptr, d_ok, stream);
}

int bjj_sign_schnorr_dev(bjj_ctx* c, const void* d_keys, const void* d_msgs, const void* d_nonces, size_t n, void* d_out_r,
                         void* d_out_s, void* d_ok, void* stream) {
  CHECK_CTX(c, "bjj_sign_schnorr_dev");
  if (n == 0) return BJJ_OK;
  CHECK_N(n);
  CHECK_PTR(d_keys, "bjj_sign_schnorr_dev"); CHECK_PTR(d_msgs, "bjj_sign_schnorr_dev"); CHECK_PTR(d_nonces, "bjj_sign_schnorr_dev");
  CHECK_PTR(d_out_r, "bjj_sign_schnorr_dev"); CHECK_PTR(d_out_s, "bjj_sign_schnorr_dev");
  if (!d_ok) return set_err(BJJ_E_INVALID, "bjj_sign_schnorr_dev: d_ok is NULL");
  DEV_ENTER(c, stream);
  if (c->ct_signer)
    LAUNCHCK(bjjk::sign_schnorr_ct(st, grid_for(c, n, c->occ_sign_schnorr_ct), c->ct_table, BJJ_CT_W, fixed_nwin(BJJ_CT_W), (const uint8_t*)d_keys,
                                   (const uint8_t*)d_msgs, (const uint8_t*)d_nonces, n, (uint8_t*)d_out_r, (uint8_t*)d_out_s, (uint8_t*)d_ok),
             "bjj_sign_schnorr_dev (constant-time)");
  else
  LAUNCHCK(bjjk::sign_schnorr(st, grid_for(c, n, c->occ_sign_schnorr), c->table, c->W, c->nwin, (const uint8_t*)d_keys,
                              (const uint8_t*)d_msgs, (const uint8_t*)d_nonces, n, (uint8_t*)d_out_r, (uint8_t*)d_out_s, (uint8_t*)d_ok),
           "bjj_sign_schnorr_dev");
  DEV_LEAVE(c);
}

// ---- host-pointer API: chunked pinned-staging pipeline around the *_dev entry points ----------
#define HOST_PROLOGUE(name, cond)                                             \
  CHECK_CTX(c, name);                                                         \
  if (n == 0) return BJJ_OK;                                                  \
  if (cond) return set_err(BJJ_E_INVALID, name ": NULL buffer")

// Chunk schedule of the K1 entry points with 32-byte results (the copy-out does not bound them: the launches do): chunks of 2^17
// items behind a first one of 2^16 -- one round of multiplications for every lane of a launch that takes one workgroup slot per CU
// (PipeSpec::k1_half).  2^18 .. 2^20 items: 8-15 % less than the schedule of the rounds before (doubling to 2^18, a 2^15-item last
// chunk; BJJ_PIPE_K1_HALF=0 brings it back for an A/B), profiles/r06_fb_host_half_slots.txt.  The affine forms keep the default
// schedule and full launches: their copy-out (64 bytes per item) is what bounds them, and they measured the same either way.
// Long calls (more than 1.5 * 2^20 items) take chunks of 2^18: their steady state is the copy engines', which move 8 MB blocks faster
// than 4 MB blocks (2^21 .. 2^23 items: 5-15 % less than with 2^17; 2^20 items: 14 % more).
static void k1_chunk_schedule(PipeSpec* sp, size_t n) {
  static const bool half = [] { const char* e = getenv("BJJ_PIPE_K1_HALF"); return !(e && e[0] == '0'); }();
  if (half) { sp->k1_half = true; sp->first_chunk = (size_t)1 << 16; sp->max_chunk = (size_t)1 << (n > ((size_t)3 << 19) ? 18 : 17); }
  else { sp->tail_chunk = (size_t)1 << 15; sp->max_chunk = (size_t)1 << 18; }
}
int bjj_mul_fixed_base(bjj_ctx* c, const uint8_t* scalars, size_t n, uint8_t* out) {
  HOST_PROLOGUE("bjj_mul_fixed_base", !scalars || !out);
  PipeSpec sp = {1, 1, {scalars}, {32}, {out}, {64}, false};
  sp.zero_copy_in = true;
  if (c->k1_variant < 0) sp.small_direct_max = small_direct_items(c->fb_quad_max);
  return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) { return bjj_mul_fixed_base_dev(c, i[0], cnt, o[0], st); });
}
// 32 bytes per result across PCIe instead of 64: the copy-out is what bounds the affine form (1.19 ms of 1.58 per 2^20 items)
int bjj_mul_fixed_base_compressed(bjj_ctx* c, const uint8_t* scalars, size_t n, uint8_t* out32) {
  HOST_PROLOGUE("bjj_mul_fixed_base_compressed", !scalars || !out32);
  PipeSpec sp = {1, 1, {scalars}, {32}, {out32}, {32}, false};
  if (c->k1_variant < 0) sp.small_direct_max = small_direct_items(c->fb_quad_max);
  k1_chunk_schedule(&sp, n);
  static const bool zc = [] { const char* e = getenv("BJJ_FB_COMPRESSED_ZERO_COPY"); return e && e[0] == '1'; }();   // experiment (tools/fb_compressed_sweep.py)
  if (zc) { sp.zero_copy_out = true; sp.tail_chunk = 0; }
  sp.zero_copy_in = true;
  return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) { return bjj_mul_fixed_base_compressed_dev(c, i[0], cnt, o[0], st); });
}
int bjj_mul_var_base(bjj_ctx* c, const uint8_t* pts, const uint8_t* scalars, size_t n, uint8_t* out) {
  HOST_PROLOGUE("bjj_mul_var_base", !pts || !scalars || !out);
  return var_base_host(c, pts, scalars, 32, n, out);
}
int bjj_mul_var_base_wide(bjj_ctx* c, const uint8_t* pts, const uint8_t* scalars, size_t scalar_bytes, size_t n, uint8_t* out) {
  HOST_PROLOGUE("bjj_mul_var_base_wide", !pts || !scalars || !out);
  if (scalar_bytes == 0 || (scalar_bytes & 31) || scalar_bytes > BJJ_MAX_SCALAR_BYTES)
    return set_err(BJJ_E_INVALID, "bjj_mul_var_base_wide: scalar_bytes must be a multiple of 32 in 32..BJJ_MAX_SCALAR_BYTES");
  return var_base_host(c, pts, scalars, scalar_bytes, n, out);
}
int bjj_poseidon5(bjj_ctx* c, const uint8_t* in, size_t n, uint8_t* out) {
  HOST_PROLOGUE("bjj_poseidon5", !in || !out);
  PipeSpec sp = {1, 1, {in}, {160}, {out}, {32}, false};
  sp.small_direct_max = small_direct_items(c->p5_coop_max);
  return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) { return bjj_poseidon5_dev(c, i[0], cnt, o[0], st); });
}
int bjj_eddsa_verify(bjj_ctx* c, const uint8_t* pk, const uint8_t* r, const uint8_t* s, const uint8_t* msg, size_t n,
                     uint8_t* ok) {
  HOST_PROLOGUE("bjj_eddsa_verify", !pk || !r || !s || !msg || !ok);
  return verify_host(c, false, pk, r, s, msg, n, ok);
}
int bjj_schnorr_verify(bjj_ctx* c, const uint8_t* pk, const uint8_t* r, const uint8_t* s, const uint8_t* msg, size_t n,
                       uint8_t* ok) {
  HOST_PROLOGUE("bjj_schnorr_verify", !pk || !r || !s || !msg || !ok);
  return verify_host(c, true, pk, r, s, msg, n, ok);
}
int bjj_point_add(bjj_ctx* c, const uint8_t* p, const uint8_t* q, size_t n, uint8_t* out) {
  HOST_PROLOGUE("bjj_point_add", !p || !q || !out);
  PipeSpec sp = {2, 1, {p, q}, {64, 64}, {out}, {64}, false};
  return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) { return bjj_point_add_dev(c, i[0], i[1], cnt, o[0], st); });
}
int bjj_proj_add(bjj_ctx* c, const uint8_t* p, const uint8_t* q, size_t n, uint8_t* out) {
  HOST_PROLOGUE("bjj_proj_add", !p || !q || !out);
  PipeSpec sp = {2, 1, {p, q}, {96, 96}, {out}, {96}, false};
  return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) { return bjj_proj_add_dev(c, i[0], i[1], cnt, o[0], st); });
}
int bjj_proj_affine(bjj_ctx* c, const uint8_t* p, size_t n, uint8_t* out) {
  HOST_PROLOGUE("bjj_proj_affine", !p || !out);
  PipeSpec sp = {1, 1, {p}, {96}, {out}, {64}, false};
  return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) { return bjj_proj_affine_dev(c, i[0], cnt, o[0], st); });
}
int bjj_compress_points(bjj_ctx* c, const uint8_t* pts, size_t n, uint8_t* out) {
  HOST_PROLOGUE("bjj_compress_points", !pts || !out);
  PipeSpec sp = {1, 1, {pts}, {64}, {out}, {32}, false};
  return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) { return bjj_compress_points_dev(c, i[0], cnt, o[0], st); });
}
int bjj_decompress_points(bjj_ctx* c, const uint8_t* in, size_t n, uint8_t* out_xy, uint8_t* ok) {
  HOST_PROLOGUE("bjj_decompress_points", !in || !out_xy || !ok);
  PipeSpec sp = {1, 2, {in}, {32}, {out_xy, ok}, {64, 1}, false};
  return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) { return bjj_decompress_points_dev(c, i[0], cnt, o[0], o[1], st); });
}
int bjj_eddsa_verify_compressed(bjj_ctx* c, const uint8_t* pk32, const uint8_t* sig64, const uint8_t* msg, size_t n,
                                uint8_t* ok) {
  HOST_PROLOGUE("bjj_eddsa_verify_compressed", !pk32 || !sig64 || !msg || !ok);
  return verify_compressed_host(c, pk32, sig64, msg, n, ok);
}
// signer side: the inputs are key material, so the staging buffers are wiped when the call is done (PipeSpec::secret)
int bjj_scalar_keys(bjj_ctx* c, const uint8_t* keys, size_t n, uint8_t* out) {
  HOST_PROLOGUE("bjj_scalar_keys", !keys || !out);
  PipeSpec sp = {1, 1, {keys}, {32}, {out}, {32}, true};
  return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) { return bjj_scalar_keys_dev(c, i[0], cnt, o[0], st); });
}
int bjj_public_keys(bjj_ctx* c, const uint8_t* keys, size_t n, uint8_t* out_xy) {
  HOST_PROLOGUE("bjj_public_keys", !keys || !out_xy);
  PipeSpec sp = {1, 1, {keys}, {32}, {out_xy}, {64}, true};
  if (c->k1_variant < 0 && !c->ct_signer) sp.small_direct_max = small_direct_items(c->fb_quad_max);
  sp.zero_copy_in = true;
  return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) { return bjj_public_keys_dev(c, i[0], cnt, o[0], st); });
}
int bjj_public_keys_compressed(bjj_ctx* c, const uint8_t* keys, size_t n, uint8_t* out32) {
  HOST_PROLOGUE("bjj_public_keys_compressed", !keys || !out32);
  PipeSpec sp = {1, 1, {keys}, {32}, {out32}, {32}, true};
  if (c->k1_variant < 0 && !c->ct_signer) sp.small_direct_max = small_direct_items(c->fb_quad_max);
  k1_chunk_schedule(&sp, n);
  sp.zero_copy_in = true;
  return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) { return bjj_public_keys_compressed_dev(c, i[0], cnt, o[0], st); });
}
int bjj_sign_compressed(bjj_ctx* c, const uint8_t* keys, const uint8_t* msgs, size_t n, uint8_t* out_sig64, uint8_t* ok) {
  HOST_PROLOGUE("bjj_sign_compressed", !keys || !msgs || !out_sig64 || !ok);
  PipeSpec sp = {2, 2, {keys, msgs}, {32, 32}, {out_sig64, ok}, {64, 1}, true};
  if (!c->ct_signer) sp.small_direct_max = small_direct_items(c->sign_small_max);
  return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) { return bjj_sign_compressed_dev(c, i[0], i[1], cnt, o[0], o[1], st); });
}
int bjj_sign(bjj_ctx* c, const uint8_t* keys, const uint8_t* msgs, size_t n, uint8_t* out_r, uint8_t* out_s, uint8_t* ok) {
  HOST_PROLOGUE("bjj_sign", !keys || !msgs || !out_r || !out_s || !ok);
  PipeSpec sp = {2, 3, {keys, msgs}, {32, 32}, {out_r, out_s, ok}, {64, 32, 1}, true};
  if (!c->ct_signer) sp.small_direct_max = small_direct_items(c->sign_small_max);
  return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) { return bjj_sign_dev(c, i[0], i[1], cnt, o[0], o[1], o[2], st); });
}
int bjj_sign_schnorr(bjj_ctx* c, const uint8_t* keys, const uint8_t* msgs, const uint8_t* nonces, size_t n, uint8_t* out_r,
                     uint8_t* out_s, uint8_t* ok) {
  HOST_PROLOGUE("bjj_sign_schnorr", !keys || !msgs || !nonces || !out_r || !out_s || !ok);
  PipeSpec sp = {3, 3, {keys, msgs, nonces}, {32, 32, BJJ_SCHNORR_NONCE_BYTES}, {out_r, out_s, ok}, {64, BJJ_SCHNORR_S_BYTES, 1}, true};
  return run_pipelined(c, n, sp, [&](void** i, void** o, size_t cnt, void* st) { return bjj_sign_schnorr_dev(c, i[0], i[1], i[2], cnt, o[0], o[1], o[2], st); });
}

// ---- bjj_msm: Q = sum k_i P_i (k_msm.hip, msm.hpp) ------------------------------------------------------------------------
// Window width c for window_bits = 0, by the number of points: index = ceil(log2 n), profiles/msm_window_sweep.txt.
// Below ~2^16 points every c from 9 to 16 costs the same ~1.3-1.6 ms: the floor is the serial Horner chain of the last kernel (255
// doublings on one lane, ~0.9 ms) and the launches, not the buckets.
static const signed char kMsmAutoWindow[33] = {10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 13, 13, 15, 15, 15, 15, 15, 15, 16, 16, 18, 18,
                                                18, 18, 18, 18, 18, 18, 18, 18, 18};
static int msm_window(size_t n, int window_bits) {
  if (window_bits) return window_bits;
  int lg = 0;
  while (lg < 32 && ((size_t)1 << lg) < n) lg++;
  return kMsmAutoWindow[lg];
}
static int msm_check(bjj_ctx* c, size_t n, int window_bits, const char* who) {
  if (!c) return set_err(BJJ_E_INVALID, std::string(who) + ": ctx is NULL");
  CHECK_N(n);
  if (window_bits != 0 && (window_bits < 4 || window_bits > 20))
    return set_err(BJJ_E_INVALID, std::string(who) + ": window_bits must be 0 (library's choice) or 4..20");
  return BJJ_OK;
}
int bjj_msm_dev(bjj_ctx* c, const void* d_pts, const void* d_scalars, size_t n, int window_bits, void* d_out, void* d_first_off_curve,
                void* stream) {
  { int rc = msm_check(c, n, window_bits, "bjj_msm_dev"); if (rc) return rc; }
  if (n) { CHECK_PTR(d_pts, "bjj_msm_dev"); CHECK_PTR(d_scalars, "bjj_msm_dev"); }
  CHECK_PTR(d_out, "bjj_msm_dev"); CHECK_PTR(d_first_off_curve, "bjj_msm_dev");
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  ENTER_DEVICE(c->device);
  ScratchSet* S = pick_set(c, st);
  const bjjk::MsmLayout L = bjjk::msm_layout(n, msm_window(n, window_bits));
  { int rc = grow_block(S->msm, L.bytes, "bjj_msm_dev", "MSM scratch"); if (rc) return rc; }
  { int rc = set_enter(c, S, st); if (rc) return rc; }
  LAUNCHCK(bjjk::msm(st, L, (const uint8_t*)d_pts, (const uint8_t*)d_scalars, n, S->msm, (uint8_t*)d_out, (unsigned long long*)d_first_off_curve),
           "bjj_msm_dev");
  return set_leave(c, S, st);
}
// Synchronous (Staged): the inputs behind the scratch that L lays out; the result and the status word come back out of L's own slots.
int bjj_msm(bjj_ctx* c, const uint8_t* pts, const uint8_t* scalars, size_t n, int window_bits, uint8_t* out_xy, int64_t* out_first_off_curve) {
  { int rc = msm_check(c, n, window_bits, "bjj_msm"); if (rc) return rc; }
  if (!out_xy || !out_first_off_curve || (n && (!pts || !scalars))) return set_err(BJJ_E_INVALID, "bjj_msm: NULL buffer");
  const bjjk::MsmLayout L = bjjk::msm_layout(n, msm_window(n, window_bits));
  ENTER_DEVICE(c->device);
  Staged G(c, "bjj_msm", L.bytes);
  const int i_pts = G.in(pts, n, 64), i_sc = G.in(scalars, n, 32);
  G.out_at(L.o_out, out_xy, 64); G.out_at(L.o_status, out_first_off_curve, 8);
  { int rc = G.begin(G.S->msm, "MSM scratch", true); if (rc) return rc; }
  uint8_t* blk = G.blk;
  LAUNCHCK(bjjk::msm(G.st, L, G.dev(i_pts), G.dev(i_sc), n, blk, blk + L.o_out, (unsigned long long*)(blk + L.o_status)), "bjj_msm");
  return G.finish();
}

// ---- bjj_msm_batch: m sums over CSR segments in one launch chain (k_msm_batch.hip, include/bjj_hip_msm_batch.h) -------------------
// Window width c for window_bits = 0, by the MEAN segment length n / m: index = ceil(log2 mean), profiles/msm_batch_window_sweep.txt
// (n = 2^20; means 2^4 .. 2^16 measured, the entries between them interpolated, those beyond 2^16 extrapolated).  A single segment
// is bjj_msm's own choice.  The key space m W B grows with 2^c for EVERY segment, so the widths stay far below bjj_msm's: per
// segment the window pass costs about W B (2 + (2 c - 1) / 8) additions next to the W len of the records.
static const signed char kMsmBatchAutoWindow[33] = {4, 4, 4, 4, 4, 4, 4, 4, 4, 6, 7, 8, 8, 8, 9, 9, 9, 10, 11, 12, 13, 14, 14, 14,
                                                     14, 14, 14, 14, 14, 14, 14, 14, 14};
static bool msm_batch_keys_fit(size_t m, int c) {
  return (unsigned __int128)m * (unsigned)msm_windows(c) * msm_buckets(c) < ((unsigned __int128)1 << 31);
}
// 0 when no width fits the 31-bit key (more than 2^22 segments)
static int msm_batch_window(size_t n, size_t m, int window_bits) {
  if (window_bits) return window_bits;
  if (m <= 1) return msm_window(n, 0);
  const size_t mean = (n + m - 1) / m;
  int lg = 0;
  while (lg < 32 && ((size_t)1 << lg) < mean) lg++;
  int c = kMsmBatchAutoWindow[lg];
  while (c > MSM_MIN_C && !msm_batch_keys_fit(m, c)) c--;
  return c;
}
// argument checks of both forms, before any allocation; *c_out: the window width of the call
static int msm_batch_check(bjj_ctx* c, size_t n, size_t m, int window_bits, const char* who, int* c_out) {
  { int rc = msm_check(c, n, window_bits, who); if (rc) return rc; }
  if (m == 0) {
    if (n) return set_err(BJJ_E_INVALID, std::string(who) + ": m == 0 requires n == 0");
    return BJJ_OK;
  }
  const int w = msm_batch_window(n, m, window_bits);
  if (!msm_batch_keys_fit(m, w))
    return set_err(BJJ_E_INVALID, std::string(who) + ": key range: m * W * B = " + std::to_string(m) + " * " + std::to_string(msm_windows(w)) +
                                      " * " + std::to_string(msm_buckets(w)) + " (window_bits " + std::to_string(w) +
                                      ") must stay below 2^31; use fewer segments per call or a smaller window_bits");
  *c_out = w;
  return BJJ_OK;
}
int bjj_msm_batch_dev(bjj_ctx* c, const void* d_pts, const void* d_scalars, size_t n, const void* d_offsets, size_t m, int window_bits,
                      void* d_out, void* d_first_off_curve, void* stream) {
  int w = 0;
  { int rc = msm_batch_check(c, n, m, window_bits, "bjj_msm_batch_dev", &w); if (rc) return rc; }
  if (m == 0) return BJJ_OK;
  if (n) { CHECK_PTR(d_pts, "bjj_msm_batch_dev"); CHECK_PTR(d_scalars, "bjj_msm_batch_dev"); }
  CHECK_PTR(d_offsets, "bjj_msm_batch_dev"); CHECK_PTR(d_out, "bjj_msm_batch_dev"); CHECK_PTR(d_first_off_curve, "bjj_msm_batch_dev");
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  ENTER_DEVICE(c->device);
  ScratchSet* S = pick_set(c, st);
  const bjjk::MsmLayout L = bjjk::msm_batch_layout(n, m, w);
  { int rc = grow_block(S->msm, L.bytes, "bjj_msm_batch_dev", "MSM scratch"); if (rc) return rc; }
  { int rc = set_enter(c, S, st); if (rc) return rc; }
  LAUNCHCK(bjjk::msm_batch(st, L, (const uint8_t*)d_pts, (const uint8_t*)d_scalars, n, (const uint64_t*)d_offsets, m, S->msm, (uint8_t*)d_out,
                           (unsigned long long*)d_first_off_curve),
           "bjj_msm_batch_dev");
  return set_leave(c, S, st);
}
// Synchronous.  The offsets are checked here, before anything is enqueued; inputs and offsets are copied once into the set's block.
int bjj_msm_batch(bjj_ctx* c, const uint8_t* pts, const uint8_t* scalars, size_t n, const uint64_t* offsets, size_t m, int window_bits,
                  uint8_t* out_xy, int64_t* out_first_off_curve) {
  int w = 0;
  { int rc = msm_batch_check(c, n, m, window_bits, "bjj_msm_batch", &w); if (rc) return rc; }
  if (m == 0) return BJJ_OK;
  if (!offsets || !out_xy || !out_first_off_curve || (n && (!pts || !scalars))) return set_err(BJJ_E_INVALID, "bjj_msm_batch: NULL buffer");
  if (offsets[0] != 0) return set_err(BJJ_E_INVALID, "bjj_msm_batch: offsets[0] must be 0");
  for (size_t s = 0; s < m; s++)
    if (offsets[s] > offsets[s + 1]) return set_err(BJJ_E_INVALID, "bjj_msm_batch: offsets decrease at segment " + std::to_string(s));
  if (offsets[m] != n) return set_err(BJJ_E_INVALID, "bjj_msm_batch: offsets[m] must equal n");
  const bjjk::MsmLayout L = bjjk::msm_batch_layout(n, m, w);
  ENTER_DEVICE(c->device);
  Staged G(c, "bjj_msm_batch", L.bytes);
  const int i_pts = G.in(pts, n, 64), i_sc = G.in(scalars, n, 32), i_off = G.in_at(L.o_offsets, offsets, (m + 1) * 8);
  G.out_at(L.o_out, out_xy, m * 64); G.out_at(L.o_status, out_first_off_curve, m * 8);
  { int rc = G.begin(G.S->msm, "MSM scratch", true); if (rc) return rc; }
  uint8_t* blk = G.blk;
  LAUNCHCK(bjjk::msm_batch(G.st, L, G.dev(i_pts), G.dev(i_sc), n, (const uint64_t*)G.dev(i_off), m, blk, blk + L.o_out,
                           (unsigned long long*)(blk + L.o_status)),
           "bjj_msm_batch");
  return G.finish();
}

// ---- fixed-base tables for caller-chosen points (k_bases.hip, bases.hpp, include/bjj_hip_bases.h) --------------------------------
#define BJJ_BASE_DEFAULT_WINDOW_BITS 16
// A x^2 + y^2 == 1 + D x^2 y^2 for the 2 x 8 words of a point record, on the host: a handle is refused before anything is allocated
static bool point_words_on_curve(const u32 xy[16]) {
  const u32 a[8] = {168700u, 0, 0, 0, 0, 0, 0, 0}, d[8] = {168696u, 0, 0, 0, 0, 0, 0, 0};
  const Fr x = fr_to_mont_words(xy), y = fr_to_mont_words(xy + 8);
  const Fr x2 = fr_sqr(x), y2 = fr_sqr(y);
  const Fr lhs = fr_add(fr_mul(fr_to_mont_words(a), x2), y2);
  const Fr rhs = fr_add(fr_one(), fr_mul(fr_to_mont_words(d), fr_mul(x2, y2)));
  return fr_eq(lhs, rhs);
}
static int base_run_check(bjj_ctx* c, const bjj_base* b, unsigned long long* bad, const char* who) {
  return device_counters(c, 1, bad, who, [&](unsigned long long* d_bad) {
    return bjjk::check_base_table(c->stream, c->cus * 8, b->table, b->bases, b->W, b->nwin, b->xy, d_bad); });
}
int bjj_base_create(bjj_ctx* c, const uint8_t* point_xy, int window_bits, bjj_base** out) {
  CHECK_CTX(c, "bjj_base_create");
  if (!point_xy || !out) return set_err(BJJ_E_INVALID, "bjj_base_create: NULL argument");
  if (window_bits != 0 && (window_bits < 4 || window_bits > BJJ_MAX_WINDOW_BITS))
    return set_err(BJJ_E_INVALID, "bjj_base_create: window_bits must be 0 (default, 16) or 4..28");
  u32 xy[16];
  memcpy(xy, point_xy, 64);
  if (!point_words_on_curve(xy)) return set_err(BJJ_E_INVALID, "bjj_base_create: the point is not on the curve");
  ENTER_DEVICE(c->device);
  bjj_base* b = new (std::nothrow) bjj_base();
  if (!b) return set_err(BJJ_E_NOMEM, "bjj_base_create: out of host memory");
  b->ctx = c;
  b->W = window_bits ? window_bits : BJJ_BASE_DEFAULT_WINDOW_BITS;
  b->nwin = base_nwin(b->W);
  memcpy(b->xy, xy, 64);
  const size_t bytes = fixed_stride(b->W) * (size_t)b->nwin * NIELS_WORDS * sizeof(u32);
  hipError_t e = b->table.grow(bytes, NO_WAIT);
  if (e == hipSuccess) e = b->bases.grow((size_t)b->nwin * NIELS_WORDS * sizeof(u32), NO_WAIT);
  if (e != hipSuccess) {
    (void)hipGetLastError(); delete b;
    return set_err(BJJ_E_NOMEM, "bjj_base_create: cannot allocate the table (" + std::to_string(bytes >> 20) + " MB)");
  }
  e = bjjk::base_window_bases(c->stream, b->bases, b->W, b->nwin, b->xy);
  if (e == hipSuccess) e = bjjk::fill_fixed_table(c->stream, b->table, b->bases, b->W, b->nwin);
  if (e != hipSuccess) { delete b; return set_err(BJJ_E_HIP, std::string("bjj_base_create: table build failed: ") + hipGetErrorString(e)); }
  unsigned long long bad = 1;   // a handle that exists is a table that passed (the rule of ensure_ct_table)
  { int rc = base_run_check(c, b, &bad, "bjj_base_create"); if (rc) { delete b; return rc; } }
  if (bad != 0) { delete b; return set_err(BJJ_E_HIP, "bjj_base_create: the table failed its self-check (" + std::to_string(bad) + " conditions)"); }
  try { c->user_bases.add(b); } catch (...) { delete b; return set_err(BJJ_E_NOMEM, "bjj_base_create: out of host memory"); }
  *out = b;
  return BJJ_OK;
}
int bjj_base_free(bjj_ctx* c, bjj_base* b) {
  CHECK_CTX(c, "bjj_base_free");
  if (!b) return BJJ_OK;
  if (!c->user_bases.owns(b)) return set_err(BJJ_E_INVALID, "bjj_base_free: not a base of this context");
  ENTER_DEVICE(c->device);
  { int rc = ctx_wait_enqueued(c); if (rc) return rc; }   // launches that gather from the table
  c->user_bases.drop(b);
  return BJJ_OK;
}
int bjj_base_info(const bjj_base* b, int* window_bits, int* n_windows, uint64_t* table_bytes) {
  if (!b) return set_err(BJJ_E_INVALID, "bjj_base_info: base is NULL");
  if (window_bits) *window_bits = b->W;
  if (n_windows) *n_windows = b->nwin;
  if (table_bytes) *table_bytes = (uint64_t)b->table.bytes;
  return BJJ_OK;
}
int bjj_base_check(bjj_ctx* c, const bjj_base* b, uint64_t* n_bad) {
  CHECK_CTX(c, "bjj_base_check");
  if (!b || !n_bad) return set_err(BJJ_E_INVALID, "bjj_base_check: NULL argument");
  if (!c->user_bases.owns(b)) return set_err(BJJ_E_INVALID, "bjj_base_check: not a base of this context");
  ENTER_DEVICE(c->device);
  unsigned long long bad = 0;
  { int rc = base_run_check(c, b, &bad, "bjj_base_check"); if (rc) return rc; }
  *n_bad = (uint64_t)bad;
  return BJJ_OK;
}
// What the kernels know of the table of `b` (scalar mod 8l), or of the context's B8 table when b is NULL (scalar mod l).  The
// scalar pointer stays NULL: only bjj_mul_bases has one per base.
static BaseDesc base_desc(const bjj_ctx* c, const bjj_base* b) {
  return b ? BaseDesc{b->table.p, nullptr, b->W, b->nwin, 0, 0} : BaseDesc{c->table.p, nullptr, c->W, c->nwin, 1, 0};
}
// argument checks of both forms; fills the descriptors but for the scalar pointers
static int mul_bases_check(bjj_ctx* c, const bjj_base* const* bases, int t, const void* const* scalars, size_t n, const char* who,
                           BasesArgs* A) {
  if (!c) return set_err(BJJ_E_INVALID, std::string(who) + ": ctx is NULL");
  if (t < 1 || t > BJJ_MAX_BASES) return set_err(BJJ_E_INVALID, std::string(who) + ": t must be 1..BJJ_MAX_BASES (8)");
  if (!bases || !scalars) return set_err(BJJ_E_INVALID, std::string(who) + ": NULL array of bases or of scalar arrays");
  CHECK_N(n);
  memset(A, 0, sizeof(*A));
  A->t = t;
  for (int j = 0; j < t; j++) {
    const bjj_base* b = bases[j];
    if (b && !c->user_bases.owns(b)) return set_err(BJJ_E_INVALID, std::string(who) + ": bases[" + std::to_string(j) + "] is not a base of this context");
    if (n && !scalars[j]) return set_err(BJJ_E_INVALID, std::string(who) + ": scalars[" + std::to_string(j) + "] is NULL");
    A->b[j] = base_desc(c, b);
  }
  return BJJ_OK;
}
static_assert(BJJ_MAX_BASES == BJJ_BASES_MAX, "include/bjj_hip_bases.h and bases.hpp disagree");
int bjj_mul_bases_dev(bjj_ctx* c, const bjj_base* const* bases, int t, const void* const* d_scalars, size_t n, void* d_out, void* stream) {
  BasesArgs A;
  { int rc = mul_bases_check(c, bases, t, d_scalars, n, "bjj_mul_bases_dev", &A); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  CHECK_PTR(d_out, "bjj_mul_bases_dev");
  for (int j = 0; j < t; j++) { CHECK_PTR(d_scalars[j], "bjj_mul_bases_dev"); A.b[j].scalars = (const uint8_t*)d_scalars[j]; }
  SET_ENTER(c, stream, n, false);
  LAUNCHCK(bjjk::mul_bases(st, c->cus, c->lanes_bases, A, n, (uint8_t*)d_out, S->scratch), "bjj_mul_bases_dev");
  SET_LEAVE(c);
}
// Synchronous (Staged): the t scalar arrays, then the results
int bjj_mul_bases(bjj_ctx* c, const bjj_base* const* bases, int t, const uint8_t* const* scalars, size_t n, uint8_t* out_xy) {
  BasesArgs A;
  { int rc = mul_bases_check(c, bases, t, (const void* const*)scalars, n, "bjj_mul_bases", &A); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  if (!out_xy) return set_err(BJJ_E_INVALID, "bjj_mul_bases: out_xy is NULL");
  ENTER_DEVICE(c->device);
  Staged G(c, "bjj_mul_bases");
  { int rc = ensure_scratch(c, G.S, n); if (rc) return rc; }
  for (int j = 0; j < t; j++) G.in(scalars[j], n, 32);   // array j of the plan
  const int i_out = G.out(out_xy, n, 64);
  { int rc = G.begin(G.S->bases_io, "device staging"); if (rc) return rc; }
  for (int j = 0; j < t; j++) A.b[j].scalars = G.dev(j);
  LAUNCHCK(bjjk::mul_bases(G.st, c->cus, c->lanes_bases, A, n, G.dev(i_out), G.S->scratch), "bjj_mul_bases");
  return G.finish();
}

// ---- verification against one signer's table (include/bjj_hip_signer.h) ------------------------------------------------------
// argument checks of both forms; fills the two table descriptors (the signer's table: mod 8l; the context's B8 table: mod l)
static int verify_signer_check(bjj_ctx* c, const bjj_base* signer, size_t n, const char* who, SignerArgs* A) {
  if (!c) return set_err(BJJ_E_INVALID, std::string(who) + ": ctx is NULL");
  if (!signer) return set_err(BJJ_E_INVALID, std::string(who) + ": signer is NULL");
  if (!c->user_bases.owns(signer)) return set_err(BJJ_E_INVALID, std::string(who) + ": signer is not a base of this context");
  CHECK_N(n);
  memset(A, 0, sizeof(*A));
  A->T = base_desc(c, signer);
  A->L = base_desc(c, nullptr);
  A->pk = signer_point(signer->xy);
  return BJJ_OK;
}
static hipError_t verify_signer_enqueue(bjj_ctx* c, hipStream_t st, bool schnorr, const SignerArgs& A, const uint8_t* r, const uint8_t* s,
                                        const uint8_t* msg, size_t n, uint8_t* ok) {
  return bjjk::verify_signer(st, c->cus, c->lanes_signer, schnorr, A, r, s, msg, n, ok);
}
// No scratch set: the kernel keeps everything in registers and LDS, so calls on different streams share nothing.
static int verify_signer_dev(bjj_ctx* c, bool schnorr, const bjj_base* signer, const void* d_r, const void* d_s, const void* d_msg, size_t n,
                             void* d_ok, void* stream, const char* who) {
  SignerArgs A;
  { int rc = verify_signer_check(c, signer, n, who, &A); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  if (!d_r || !d_s || !d_msg || !aligned16(d_r) || !aligned16(d_s) || !aligned16(d_msg))
    return set_err(BJJ_E_INVALID, std::string(who) + ": NULL or not 16-byte aligned device pointer");
  if (!d_ok) return set_err(BJJ_E_INVALID, std::string(who) + ": d_ok is NULL");
  DEV_ENTER(c, stream);
  LAUNCHCK_S(verify_signer_enqueue(c, st, schnorr, A, (const uint8_t*)d_r, (const uint8_t*)d_s, (const uint8_t*)d_msg, n, (uint8_t*)d_ok), who);
  DEV_LEAVE(c);
}
// Synchronous (Staged): R, s, msg, then the verdicts
static int verify_signer_host(bjj_ctx* c, bool schnorr, const bjj_base* signer, const uint8_t* r, const uint8_t* s, const uint8_t* msg, size_t n,
                              uint8_t* ok, const char* who) {
  SignerArgs A;
  { int rc = verify_signer_check(c, signer, n, who, &A); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  if (!r || !s || !msg || !ok) return set_err(BJJ_E_INVALID, std::string(who) + ": NULL buffer");
  ENTER_DEVICE(c->device);
  Staged G(c, who);
  const int i_r = G.in(r, n, 64), i_s = G.in(s, n, 32), i_msg = G.in(msg, n, 32), i_ok = G.out(ok, n, 1);
  { int rc = G.begin(G.S->bases_io, "device staging"); if (rc) return rc; }
  LAUNCHCK_S(verify_signer_enqueue(c, G.st, schnorr, A, G.dev(i_r), G.dev(i_s), G.dev(i_msg), n, G.dev(i_ok)), who);
  return G.finish();
}
int bjj_eddsa_verify_signer(bjj_ctx* c, const bjj_base* signer, const uint8_t* r_xy, const uint8_t* s, const uint8_t* msg, size_t n, uint8_t* ok) {
  return verify_signer_host(c, false, signer, r_xy, s, msg, n, ok, "bjj_eddsa_verify_signer");
}
int bjj_eddsa_verify_signer_dev(bjj_ctx* c, const bjj_base* signer, const void* d_r_xy, const void* d_s, const void* d_msg, size_t n, void* d_ok,
                                void* stream) {
  return verify_signer_dev(c, false, signer, d_r_xy, d_s, d_msg, n, d_ok, stream, "bjj_eddsa_verify_signer_dev");
}
int bjj_schnorr_verify_signer(bjj_ctx* c, const bjj_base* signer, const uint8_t* r_xy, const uint8_t* s, const uint8_t* msg, size_t n, uint8_t* ok) {
  return verify_signer_host(c, true, signer, r_xy, s, msg, n, ok, "bjj_schnorr_verify_signer");
}
int bjj_schnorr_verify_signer_dev(bjj_ctx* c, const bjj_base* signer, const void* d_r_xy, const void* d_s, const void* d_msg, size_t n, void* d_ok,
                                  void* stream) {
  return verify_signer_dev(c, true, signer, d_r_xy, d_s, d_msg, n, d_ok, stream, "bjj_schnorr_verify_signer_dev");
}

// ---- verification against a set of signers' tables, by per-item index (include/bjj_hip_signer_set.h) ------------------------------
#define BJJ_SET_DEFAULT_WINDOW_BITS 8
#define BJJ_SET_MAX_WINDOW_BITS 16
static_assert(BJJ_VERIFY_BAD_SIGNER == BJJ_SET_BAD_SIGNER, "include/bjj_hip_signer_set.h and signer_set.hpp disagree");
static int set_run_check(bjj_ctx* c, const bjj_signer_set* t, unsigned long long* bad, const char* who) {
  return device_counters(c, 1, bad, who, [&](unsigned long long* d_bad) {
    return bjjk::check_signer_set(c->stream, c->cus * 8, t->table, t->bases, t->keys, t->k, t->W, t->nwin, d_bad); });
}
int bjj_signer_set_create(bjj_ctx* c, const uint8_t* pks_xy, size_t k, int window_bits, bjj_signer_set** out, int64_t* out_first_off_curve) {
  CHECK_CTX(c, "bjj_signer_set_create");
  if (!pks_xy || !out) return set_err(BJJ_E_INVALID, "bjj_signer_set_create: NULL argument");
  if (window_bits != 0 && (window_bits < 4 || window_bits > BJJ_SET_MAX_WINDOW_BITS))
    return set_err(BJJ_E_INVALID, "bjj_signer_set_create: window_bits must be 0 (default, 8) or 4..16");
  const int W = window_bits ? window_bits : BJJ_SET_DEFAULT_WINDOW_BITS;
  // the gather carries slot numbers as 32-bit words: before any point is looked at, before anything is allocated
  if (!set_slots_fit((u64)k, W))
    return set_err(BJJ_E_INVALID, "bjj_signer_set_create: k must be 1 .. 2^32 / (n_windows * (2^(window_bits-1) + 1)) = " +
                                      std::to_string((((u64)1) << 32) / set_entries_per_signer(W)));
  std::vector<u32> keys;
  try { keys.resize(k * SET_KEY_WORDS); } catch (...) { return set_err(BJJ_E_NOMEM, "bjj_signer_set_create: out of host memory"); }
  for (size_t j = 0; j < k; j++) {
    u32 xy[16];
    memcpy(xy, pks_xy + j * 64, 64);
    if (!point_words_on_curve(xy)) {
      if (out_first_off_curve) *out_first_off_curve = (int64_t)j;
      return set_err(BJJ_E_INVALID, "bjj_signer_set_create: key " + std::to_string(j) + " is not on the curve");
    }
    set_key_store(keys.data() + j * SET_KEY_WORDS, signer_point(xy));
  }
  ENTER_DEVICE(c->device);
  bjj_signer_set* t = new (std::nothrow) bjj_signer_set();
  if (!t) return set_err(BJJ_E_NOMEM, "bjj_signer_set_create: out of host memory");
  t->ctx = c; t->W = W; t->nwin = base_nwin(W); t->k = k;
  const size_t bytes = k * (size_t)set_entries_per_signer(W) * NIELS_WORDS * sizeof(u32);
  hipError_t e = t->table.grow(bytes, NO_WAIT);
  if (e == hipSuccess) e = t->bases.grow(k * (size_t)t->nwin * NIELS_WORDS * sizeof(u32), NO_WAIT);
  if (e == hipSuccess) e = t->keys.grow(keys.size() * sizeof(u32), NO_WAIT);
  if (e != hipSuccess) {
    (void)hipGetLastError(); delete t;
    return set_err(BJJ_E_NOMEM, "bjj_signer_set_create: cannot allocate the tables (" + std::to_string(bytes >> 20) + " MB)");
  }
  e = hipMemcpyAsync(t->keys, keys.data(), keys.size() * sizeof(u32), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = bjjk::build_signer_set(c->stream, t->table, t->bases, t->keys, k, W, t->nwin);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // `keys` is this call's own memory
  if (e != hipSuccess) { delete t; return set_err(BJJ_E_HIP, std::string("bjj_signer_set_create: table build failed: ") + hipGetErrorString(e)); }
  unsigned long long bad = 1;   // a handle that exists is a set that passed (the rule of bjj_base_create)
  { int rc = set_run_check(c, t, &bad, "bjj_signer_set_create"); if (rc) { delete t; return rc; } }
  if (bad != 0) { delete t; return set_err(BJJ_E_HIP, "bjj_signer_set_create: the tables failed their self-check (" + std::to_string(bad) + " conditions)"); }
  try { c->user_sets.add(t); } catch (...) { delete t; return set_err(BJJ_E_NOMEM, "bjj_signer_set_create: out of host memory"); }
  if (out_first_off_curve) *out_first_off_curve = -1;
  *out = t;
  return BJJ_OK;
}
int bjj_signer_set_free(bjj_ctx* c, bjj_signer_set* t) {
  CHECK_CTX(c, "bjj_signer_set_free");
  if (!t) return BJJ_OK;
  if (!c->user_sets.owns(t)) return set_err(BJJ_E_INVALID, "bjj_signer_set_free: not a signer set of this context");
  ENTER_DEVICE(c->device);
  { int rc = ctx_wait_enqueued(c); if (rc) return rc; }   // launches that gather from the tables
  c->user_sets.drop(t);
  return BJJ_OK;
}
int bjj_signer_set_info(const bjj_signer_set* t, uint64_t* n_signers, int* window_bits, int* n_windows, uint64_t* table_bytes) {
  if (!t) return set_err(BJJ_E_INVALID, "bjj_signer_set_info: set is NULL");
  if (n_signers) *n_signers = (uint64_t)t->k;
  if (window_bits) *window_bits = t->W;
  if (n_windows) *n_windows = t->nwin;
  if (table_bytes) *table_bytes = (uint64_t)t->table.bytes;
  return BJJ_OK;
}
int bjj_signer_set_check(bjj_ctx* c, const bjj_signer_set* t, uint64_t* n_bad) {
  CHECK_CTX(c, "bjj_signer_set_check");
  if (!t || !n_bad) return set_err(BJJ_E_INVALID, "bjj_signer_set_check: NULL argument");
  if (!c->user_sets.owns(t)) return set_err(BJJ_E_INVALID, "bjj_signer_set_check: not a signer set of this context");
  ENTER_DEVICE(c->device);
  unsigned long long bad = 0;
  { int rc = set_run_check(c, t, &bad, "bjj_signer_set_check"); if (rc) return rc; }
  *n_bad = (uint64_t)bad;
  return BJJ_OK;
}
// argument checks of both forms; fills the descriptors (the set's tables: mod 8l; the context's B8 table: mod l)
static int verify_set_check(bjj_ctx* c, const bjj_signer_set* t, size_t n, const char* who, SetArgs* A) {
  if (!c) return set_err(BJJ_E_INVALID, std::string(who) + ": ctx is NULL");
  if (!t) return set_err(BJJ_E_INVALID, std::string(who) + ": set is NULL");
  if (!c->user_sets.owns(t)) return set_err(BJJ_E_INVALID, std::string(who) + ": set is not a signer set of this context");
  CHECK_N(n);
  memset(A, 0, sizeof(*A));
  A->T = BaseDesc{t->table.p, nullptr, t->W, t->nwin, 0, 0};   // signer 0's table = the base of the allocation
  A->L = base_desc(c, nullptr);
  A->keys = t->keys.p; A->k = (u32)t->k; A->eps = (u32)set_entries_per_signer(t->W);
  return BJJ_OK;
}
static hipError_t verify_set_enqueue(bjj_ctx* c, hipStream_t st, bool schnorr, const SetArgs& A, const uint32_t* idx, const uint8_t* r,
                                     const uint8_t* s, const uint8_t* msg, size_t n, uint8_t* ok) {
  return bjjk::verify_set(st, c->cus, c->lanes_set, schnorr, A, idx, r, s, msg, n, ok);
}
// No scratch set: the kernel keeps everything in registers and LDS, so calls on different streams share nothing.
static int verify_set_dev(bjj_ctx* c, bool schnorr, const bjj_signer_set* t, const void* d_idx, const void* d_r, const void* d_s,
                          const void* d_msg, size_t n, void* d_ok, void* stream, const char* who) {
  SetArgs A;
  { int rc = verify_set_check(c, t, n, who, &A); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  if (!d_idx || !d_r || !d_s || !d_msg || !aligned16(d_idx) || !aligned16(d_r) || !aligned16(d_s) || !aligned16(d_msg))
    return set_err(BJJ_E_INVALID, std::string(who) + ": NULL or not 16-byte aligned device pointer");
  if (!d_ok) return set_err(BJJ_E_INVALID, std::string(who) + ": d_ok is NULL");
  DEV_ENTER(c, stream);
  LAUNCHCK_S(verify_set_enqueue(c, st, schnorr, A, (const uint32_t*)d_idx, (const uint8_t*)d_r, (const uint8_t*)d_s, (const uint8_t*)d_msg, n,
                                (uint8_t*)d_ok), who);
  DEV_LEAVE(c);
}
// Synchronous (Staged): R, s, msg and the indices (behind the records, as the block always held them), then the verdicts
static int verify_set_host(bjj_ctx* c, bool schnorr, const bjj_signer_set* t, const uint32_t* idx, const uint8_t* r, const uint8_t* s,
                           const uint8_t* msg, size_t n, uint8_t* ok, const char* who) {
  SetArgs A;
  { int rc = verify_set_check(c, t, n, who, &A); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  if (!idx || !r || !s || !msg || !ok) return set_err(BJJ_E_INVALID, std::string(who) + ": NULL buffer");
  ENTER_DEVICE(c->device);
  Staged G(c, who);
  const int i_r = G.in(r, n, 64), i_s = G.in(s, n, 32), i_msg = G.in(msg, n, 32), i_idx = G.in(idx, n, 4), i_ok = G.out(ok, n, 1);
  { int rc = G.begin(G.S->bases_io, "device staging"); if (rc) return rc; }
  LAUNCHCK_S(verify_set_enqueue(c, G.st, schnorr, A, (const uint32_t*)G.dev(i_idx), G.dev(i_r), G.dev(i_s), G.dev(i_msg), n, G.dev(i_ok)), who);
  return G.finish();
}
int bjj_eddsa_verify_set(bjj_ctx* c, const bjj_signer_set* set, const uint32_t* signer_idx, const uint8_t* r_xy, const uint8_t* s,
                         const uint8_t* msg, size_t n, uint8_t* ok) {
  return verify_set_host(c, false, set, signer_idx, r_xy, s, msg, n, ok, "bjj_eddsa_verify_set");
}
int bjj_eddsa_verify_set_dev(bjj_ctx* c, const bjj_signer_set* set, const void* d_signer_idx, const void* d_r_xy, const void* d_s,
                             const void* d_msg, size_t n, void* d_ok, void* stream) {
  return verify_set_dev(c, false, set, d_signer_idx, d_r_xy, d_s, d_msg, n, d_ok, stream, "bjj_eddsa_verify_set_dev");
}
int bjj_schnorr_verify_set(bjj_ctx* c, const bjj_signer_set* set, const uint32_t* signer_idx, const uint8_t* r_xy, const uint8_t* s,
                           const uint8_t* msg, size_t n, uint8_t* ok) {
  return verify_set_host(c, true, set, signer_idx, r_xy, s, msg, n, ok, "bjj_schnorr_verify_set");
}
int bjj_schnorr_verify_set_dev(bjj_ctx* c, const bjj_signer_set* set, const void* d_signer_idx, const void* d_r_xy, const void* d_s,
                               const void* d_msg, size_t n, void* d_ok, void* stream) {
  return verify_set_dev(c, true, set, d_signer_idx, d_r_xy, d_s, d_msg, n, d_ok, stream, "bjj_schnorr_verify_set_dev");
}

#include "bjj_dlog.inc"
#include "bjj_point_sum.inc"
#include "bjj_common_scalar.inc"
#include "bjj_elgamal.inc"
#include "bjj_dleq.inc"

#pragma GCC visibility pop
}  // extern "C"

#include "bjj_multi.inc"
