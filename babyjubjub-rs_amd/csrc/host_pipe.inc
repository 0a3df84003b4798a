// host_pipe.inc -- the host-pointer pipeline: everything between an extern "C" entry point that takes host pointers and the
// device-pointer launches it is made of.  Included by bjj_hip.hip (one translation unit with the contexts); the arithmetic that
// decides what runs -- chunk schedule, lane parity, staging and ring offsets, the super-batch cap -- is pipe_plan.hpp.
// ---------------------------------------------------------------------------
// Host-pointer API plumbing.
//
// A call is cut into chunks; chunk k flows
//     H2D (copy stream s_in)  ->  kernels on lane k % 2 (stream / stream2)  ->  D2H (copy stream s_out)
// through device staging that holds the WHOLE batch (every array contiguous, up to BJJ_PIPE_STAGING_MB = 1 GB per call; a
// larger batch runs as consecutive super-batches), so nothing on the device is ever reused inside a call.
// * Pinned caller memory (bjj_host_alloc, bjj_host_register, or anything the HIP runtime reports as pinned host memory) is
//   copied from / to DIRECTLY: no staging copy at all, the bound is the slower PCIe direction (2^20 fixed-base
//   multiplications: 64 MB of results, 1.19 ms).  Round 4 staged everything through two pinned buffers with a memcpy on the
//   calling thread and ran at 17 % of the device rate (VERDICT r04 item 5).
// * A pageable array goes through a ring of pinned buffers; the memcpy between ring and caller memory is done by the
//   context's copy workers (CopyPool) while the calling thread only enqueues.  (A pageable hipMemcpy runs at ~3 GB/s.)
// * Two lanes = the context's two scratch sets: the kernels of consecutive chunks overlap on the chip like the two-stream
//   launches of the device-pointer API (verify in 2^18-item chunks on ONE stream ran 6.76 ms per chunk, on two 4.47 ms:
//   profiles/r04_throughput_vs_batch.txt).  The lanes carry kernels only.
// * What orders the stages is chosen so that NO mapping of streams onto hardware queues can hurt.  HIP binds a stream, at its
//   first use, to one of FOUR hardware queues of its priority (a fifth stream shares one), packets of a hardware queue run in
//   order, and an event record or a cross-stream wait behind an SDMA copy -- or a wait for a kernel on a copy stream -- is a
//   barrier packet there: a kernel of ANOTHER stream that lands behind such a packet waits for whatever the packet waits for.
//   The forms of this pipeline, in the order they were measured (profiles/r05_host_pipeline.txt; 2^20 fixed-base, pinned):
//     normal-priority copy streams, one event per chunk and stage: every kernel ran behind the previous chunk's D2H   2.7 ms
//     D2H in stream order behind the kernels (no events; the runtime then copies with a shader blit at half rate)       1.65 ms
//     copy streams and second lane of the HIGHEST priority (their own queue pool), s_out waiting for the kernels'
//     events on the device: 1.62 ms in a fresh process, but 12 % slower verifications in a process whose other
//     high-priority streams (the verify scan streams) had pushed the second lane onto s_out's hardware queue
//     the same with the wait moved to the HOST (ships): the calling thread, idle anyway, watches the chunks' kernel
//     events in order and enqueues each D2H when its kernels are done -- s_out's queue holds no packet at all          1.58 ms
//   What remains on the device: one event per chunk behind the H2D on s_in, which completes early (copies on s_in run in
//   order and far ahead of the kernels), and the lanes' kernels.  Apart from the context's own stream the pipeline occupies
//   no normal-priority queue: a library that parks streams there leaves the caller's streams to share what is left (two torch
//   streams first used after a host-pointer call landed on ONE hardware queue and their launches ran one after the other).
//   The verify scans of the pipeline's chunks run in line (on their priority streams they were no faster here: 19.0 vs 19.1 ms).
// * The first chunk is small (2^15 items: the copy-out engine, which bounds a copy-bound call, starts 0.1 ms after the call)
//   and the size doubles up to 2^18; a remainder below half a chunk is merged into the
//   last chunk (a small last launch leaves the chip half empty).  BJJ_PIPE_FIRST_CHUNK / BJJ_PIPE_CHUNK (items) override.
// ---------------------------------------------------------------------------
// The cap was 2^18 until round 6.  With 2^18-item chunks (16 MB copy-outs for 64-byte results) the copy engines' device-to-host rate has two
// states per process -- 56 or 44 GB/s, the SOC clock domain awake or asleep between calls, depending on what the process did before
// (profiles/r06_host_d2h_power_states.txt): 2^20 fixed-base multiplications take 1.575 or 1.92 ms.  With 2^17-item chunks the slow state
// does not occur (1.565-1.60 ms in every sequence tried) and the fast state loses nothing.  The compressed fixed-base forms keep 2^18
// (1.155 ms in the fast state against 1.26 with 2^17; 1.30-1.36 in the slow state with either).
#define BJJ_PIPE_CHUNK ((size_t)1 << 17)
#define BJJ_PIPE_FIRST_CHUNK ((size_t)1 << 15)
struct PipeSpec {
  int n_in, n_out;
  const uint8_t* in[4]; size_t in_stride[4];
  uint8_t* out[4];      size_t out_stride[4];
  bool secret;          // inputs are key material: wipe the staging buffers when the call is done
  struct ExactListStage* exact = nullptr;   // the batch-wide exact list beside the chunk launches (below)
  bool out_at_end = false;             // outputs leave the device once, after everything (they are not final chunk by chunk)
  size_t first_chunk = 0, max_chunk = 0;   // chunk schedule of this entry point (items; 0 = the context's, which the environment overrides)
  size_t extra_dev_per_item = 0;           // bytes of device staging per item for `exact` (ExactListStage::d_extra), beside the arrays
  // Kernel-bound calls whose launches are work-conserving among themselves (one tile / group per workgroup):
  //   tail_chunk            the LAST chunk has at most this many items (0 = no rule): its copy-out is the only one nothing hides
  //   last_on_priority_lane the lanes are the context's stream (normal priority) and stream2 (highest): the hardware serves the
  //                         priority lane's workgroups first, so ITS chain of launches ends first and the other lane's last launch
  //                         runs its tail alone.  With the last chunk on the priority lane the other lane's launches fill every tail
  //                         but the very last one -- as in ONE launch (profiles/r06_var_base_host_schedule.txt)
  size_t tail_chunk = 0;
  bool last_on_priority_lane = false;
  // The kernels of this entry point write every output byte exactly once and never read it (their scratch is elsewhere): when ALL
  // output arrays are pinned, the launches get the arrays' DEVICE MAPPINGS instead of staging and there is no copy-out stage at all.
  // Only for kernel-bound calls: a kernel's stores to mapped host memory run at the copy engines' rate (54.9 GB/s), but a workgroup
  // holds its slot until PCIe has taken them -- K1, which is copy-bound, lost 5 % this way (profiles/r05_host_pipeline.txt).
  bool zero_copy_out = false;
  // The first kernel of a chunk reads every input byte exactly once, coalesced, at the start of an item's work: when ALL input arrays are
  // pinned, the launches read them through the arrays' DEVICE MAPPINGS and there is no copy-in stage -- the first kernel starts at once
  // instead of behind a copy, and the chain of launches is no longer paced by the copy engine (43 GB/s over the small copies of a
  // schedule) but by the kernels.  For launch chains that outrun their copy-in: K1, whose 2^20 items are 0.55 ms of kernel behind
  // 0.77 ms of copy-in (profiles/r06_fb_zero_copy_in.txt).  Not with an `exact` stage (its scans wait for copies).
  bool zero_copy_in = false;
  // K1 chunk launches (fixed base, public keys): a launch of K1 is persistent -- every lane walks its items, then ONE epilogue per
  // workgroup (inversion, phase 2) -- and its ramp, epilogue and tail cost about one round of multiplications (~70 us) whatever
  // its size.  A chunk launch that fills both workgroup slots of every CU runs that fixed part with nothing beside it; one that
  // takes ONE slot per CU (256 lanes) shares each CU with the neighbouring chunk's launch on the other lane, out of phase by the
  // pacing of the copies, and the fixed part of one is covered by the main loop of the other -- as on two caller streams
  // (profiles/r03_ab_k1_2x256_two_streams.txt).  Calls of >= 2 chunks only (profiles/r06_fb_host_half_slots.txt).
  bool k1_half = false;
  // Short calls (a call of ONE item is the reference's single-item API): with at most this many items, one chunk and every array pinned and 16-byte aligned,
  // the kernels read the inputs AND store the results through the arrays' device mappings -- no copy, no event hop, the host does not come back between
  // the kernel and a copy-out: launch and synchronise (20-30 us of a 100-600 us call).  Only for entry points whose short calls run kernels that write every
  // output byte once and read none of it back (csrc/k_small.hip).  0 = never.
  size_t small_direct_max = 0;
};
// The batch-wide exact list of a host-pointer call: variable base (off-curve points), the verifiers (off-curve pk / R) and the wire-format
// verifier (the same, after decompression).  An item of that kind takes the exact kernel, ~3x as long as a bulk item and strictly serial per
// lane; a chunk launch that carried its own would last as long as they do and hold its lane.  So each chunk's bulk launch skips them, and ONE
// exact launch over ONE list serves the super-batch, on the first scratch set's scan stream, beside the bulk launches.  The pipeline calls,
// on the calling thread while it enqueues:
//   open        once per super-batch, before the first copy: the list, reset on the scan stream; d_in / d_out = the super-batch's arrays
//   decompress  wire format only, per chunk, on its lane behind its H2D: pk, R and s into d_extra; the pipeline records ev_mid behind it
//   scan        per chunk: the scan stream waits for `ready` (the chunk's ev_in, or its ev_mid), then appends the chunk's items to the list
//   close       once, behind the last chunk's launch (every scan is enqueued): the exact launch, then a pass over the whole batch where
//               there is one -- it writes output bytes the bulk launches write too, so it waits for every lane's last bulk launch
//               (bulk_done) -- then ev_tail, which the call waits for before it copies `out_at_end` outputs and returns
//   finish      last, every copy landed (host_out = where the super-batch's outputs begin): variable base with staged outputs lays K6's
//               compact results over their slots in the caller's array
struct ExactListStage {
  enum Kind { VAR_BASE, VERIFY, VERIFY_COMPRESSED };
  bjj_ctx* const c;
  const Kind kind;
  bool schnorr = false;              // VERIFY
  int sc_words = 0;                  // VAR_BASE: 4-byte words per scalar
  size_t n = 0;                      // items of the super-batch
  uint8_t* in[4] = {};               // its inputs on the device: pts, scalars | pk, r, s, msg | pk32, sig64, msg
  uint8_t* out = nullptr;            // its output: the staging, or (zero_copy) the device mapping of the caller's pinned array
  uint8_t* d_extra = nullptr;        // n * PipeSpec::extra_dev_per_item bytes of the super-batch's staging
  bool zero_copy = false;
  uint8_t *pk = nullptr, *r = nullptr, *s = nullptr, *msg = nullptr;   // what the verify kernels read: in[], or what decompress wrote to d_extra
  uint8_t *f_pk = nullptr, *f_r = nullptr;                               // VERIFY_COMPRESSED: the decompression flags (d_extra)
  ExactListStage(bjj_ctx* c_, Kind k) : c(c_), kind(k) {}
  int open(size_t n, void* const* d_in, void* const* d_out, uint8_t* d_extra, bool zero_copy);
  int decompress(size_t lo, size_t cnt, hipStream_t lane);
  int scan(size_t lo, size_t cnt, hipEvent_t ready);
  int close(const hipEvent_t* bulk_done, size_t lanes);
  int finish(uint8_t* host_out);
};

// ---- pinned host memory ---------------------------------------------------------------------------------------------------
// Ranges handed out by bjj_host_alloc (hipHostMalloc) or pinned in place by bjj_host_register (hipHostRegister): process-wide,
// any context may copy from / to them.  Memory pinned by somebody else (torch's pin_memory, the caller's own hipHostMalloc) is
// recognised through the driver's pointer attributes.  A wrong answer can only cost speed: hipMemcpyAsync accepts any host
// pointer, and every call waits for its copies before it returns.
struct HostRange { uintptr_t lo, hi; bool owned; };
static std::mutex g_host_mu;
static std::vector<HostRange> g_host_ranges;
static bool host_range_registered(const void* p, size_t bytes) {
  const uintptr_t lo = (uintptr_t)p, hi = lo + bytes;
  std::lock_guard<std::mutex> lk(g_host_mu);
  for (const HostRange& r : g_host_ranges) if (lo >= r.lo && hi <= r.hi) return true;
  return false;
}
static bool driver_attr(const void* p, hipPointerAttribute_t* a) {
  memset(a, 0, sizeof(*a));
  if (hipPointerGetAttributes(a, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // an ordinary malloc'd pointer
  return true;
}
static bool host_range_pinned(const void* p, size_t bytes) {
  if (!bytes || host_range_registered(p, bytes)) return true;
  hipPointerAttribute_t a0, a1;
  if (!driver_attr(p, &a0) || a0.type != hipMemoryTypeHost) return false;
  if (!driver_attr((const uint8_t*)p + bytes - 1, &a1) || a1.type != hipMemoryTypeHost) return false;
  // both ends are pinned: one mapping?  (two pinned allocations with a pageable hole between them would pass the end test)
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (a0.devicePointer && hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)a0.devicePointer) == hipSuccess)
    return (uintptr_t)a0.devicePointer - (uintptr_t)base + bytes <= size;
  (void)hipGetLastError();
  return a0.devicePointer && a1.devicePointer && (uintptr_t)a1.devicePointer - (uintptr_t)a0.devicePointer == bytes - 1;
}

static size_t env_items(const char* name, size_t dflt) { return pipe_parse_items(getenv(name), dflt); }
// The context's high-priority streams, created AND first used in a fixed order when the context is made.  HIP binds a stream to a
// hardware queue at its first use: the streams of one priority share FOUR queues, a fifth stream takes the queue of the first, and
// packets of streams that share a queue run one after the other.  Created on demand, the assignment depended on what the caller
// did first: after two-stream verifications (both sets' scan streams in use) the pipeline's second lane landed on the first scan
// stream's queue -- the stream the host-pointer pipelines run their scans and exact launches on, whose small kernels wait for
// wave slots while the lanes' kernels fill the chip -- and a chunk's launch on that lane queued behind them: 2^20 variable-base
// multiplications on pinned memory took 17.0 ms instead of 15.9 (profiles/r06_var_base_host_schedule.txt).  Now: copy-in, copy-out,
// second lane, first scan stream = queues 0..3, always; the second set's scan stream (two-stream device-pointer callers only) is
// the one that shares -- with the copy-in stream, which carries nothing while a device-pointer launch is what the caller is doing.
//   * the second lane is a high-priority stream as well: a library that parks two normal-priority streams in the four queues of
//     that priority (the context's own stream is one) leaves the caller's streams to share what is left -- two torch streams first
//     used after a host-pointer call landed on ONE hardware queue and their launches ran one after the other
//     (tools/queue_map_probe.py, profiles/r05_host_pipeline.txt)
static int ensure_scan_stream(ScratchSet* S);
static int ensure_pipe_streams(bjj_ctx* c) {
  if (c->s_in && c->s_out && c->stream2 && c->ev_tail && c->set[0].scan_stream) return BJJ_OK;
  int least = 0, greatest = 0;
  HIPCK(hipDeviceGetStreamPriorityRange(&least, &greatest));
  int prio_in = greatest, prio_out = greatest;
  if (const char* e = getenv("BJJ_PIPE_COPY_PRIORITY")) {   // developer: "nn" / "hn" / "nh" / "hh" = normal / high for s_in, s_out
    if (e[0] == 'n') prio_in = 0;
    if (e[0] && e[1] == 'n') prio_out = 0;
  }
  if (!c->ev_tail) HIPCK(hipEventCreateWithFlags(&c->ev_tail, hipEventDisableTiming));
  hipStream_t* order[3] = {&c->s_in, &c->s_out, &c->stream2};
  const int prio[3] = {prio_in, prio_out, greatest};
  for (int k = 0; k < 3; k++)
    if (!*order[k]) {
      HIPCK(hipStreamCreateWithPriority(order[k], hipStreamNonBlocking, prio[k]));
      HIPCK(hipEventRecord(c->ev_tail, *order[k]));              // first use: binds the hardware queue
      HIPCK(hipStreamSynchronize(*order[k]));
    }
  if (!c->set[0].scan_stream) {
    int rc = ensure_scan_stream(&c->set[0]); if (rc) return rc;
    HIPCK(hipEventRecord(c->ev_tail, c->set[0].scan_stream));
    HIPCK(hipStreamSynchronize(c->set[0].scan_stream));
  }
  return BJJ_OK;
}
// streams of the pipeline, events for `chunks` chunks, dev_bytes of device staging and -- only when a pageable array takes
// part -- the pinned rings (in_ring / out_ring bytes per slot) and the copy workers
static int ensure_pipe(bjj_ctx* c, size_t chunks, size_t dev_bytes, size_t in_ring, size_t out_ring) {
  ENTER_DEVICE(c->device);
  // first use: the knobs first (they cannot fail), then whatever of streams / event is still missing; `pipe_ready` only when all of it
  // exists -- a call after a failed first use comes through here again instead of running with a zero chunk size (ADVICE r05)
  if (!c->pipe_ready) {
    c->pipe_env_schedule = getenv("BJJ_PIPE_CHUNK") || getenv("BJJ_PIPE_FIRST_CHUNK");
    c->pipe_chunk = env_items("BJJ_PIPE_CHUNK", BJJ_PIPE_CHUNK);
    c->pipe_first = env_items("BJJ_PIPE_FIRST_CHUNK", BJJ_PIPE_FIRST_CHUNK);
    if (c->pipe_first > c->pipe_chunk) c->pipe_first = c->pipe_chunk;
    c->pipe_budget = (size_t)1 << 30;
    if (const char* e = getenv("BJJ_PIPE_STAGING_MB")) { const long v = atol(e); if (v >= 1 && v <= 65536) c->pipe_budget = (size_t)v << 20; }
    if (const char* e = getenv("BJJ_HOST_FORCE_STAGED")) c->force_staged = e[0] == '1';
    if (const char* e = getenv("BJJ_PIPE_SCAN")) c->pipe_scan_inline = e[0] != 'p';
    if (const char* e = getenv("BJJ_PIPE_ZERO_COPY")) c->pipe_zero_copy = e[0] != '0';
    if (const char* e = getenv("BJJ_PIPE_ZERO_COPY_IN")) c->pipe_zero_copy_in = e[0] != '0';
    if (const char* e = getenv("BJJ_PIPE_SMALL_DIRECT")) c->pipe_small_direct = e[0] != '0';
    { int rc = ensure_pipe_streams(c); if (rc) return rc; }
    c->pipe_ready = true;
  }
  try {
    while (c->ev_in.size() < chunks) {
      hipEvent_t e = nullptr;
      HIPCK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); c->ev_in.push_back(e);
      e = nullptr;
      HIPCK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); c->ev_k.push_back(e);
      e = nullptr;
      HIPCK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); c->ev_out.push_back(e);
      e = nullptr;
      HIPCK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); c->ev_mid.push_back(e);
    }
  } catch (...) { return set_err(BJJ_E_NOMEM, "host-pointer pipeline: out of host memory"); }
  if (dev_bytes > c->dstage.bytes) {   // only the lanes' kernels can still be using the staging: every call waits for its copies
    HIPCK(hipStreamSynchronize(c->stream));
    HIPCK(hipStreamSynchronize(c->stream2));
  }
  HIPCK(c->dstage.grow(dev_bytes, NO_WAIT));
  for (PinBlock<uint8_t>& pin_in : c->pin_in) HIPCK(pin_in.grow(in_ring, NO_WAIT));      // nothing is in flight through the rings between calls
  for (PinBlock<uint8_t>& pin_out : c->pin_out) HIPCK(pin_out.grow(out_ring, NO_WAIT));
  if ((in_ring || out_ring) && !c->pool) {
    int want = 4;
    if (const char* e = getenv("BJJ_STAGE_THREADS")) { const int v = atoi(e); if (v >= 1 && v <= 32) want = v; }
    const unsigned hw = std::thread::hardware_concurrency();
    if (hw && (unsigned)want > hw) want = (int)hw;
    c->pool = new (std::nothrow) CopyPool();
    if (!c->pool || !c->pool->start(want)) { delete c->pool; c->pool = nullptr; return set_err(BJJ_E_NOMEM, "host-pointer pipeline: cannot start the copy workers"); }
  }
  return BJJ_OK;
}
// BJJ_PIPE_TRACE=1 (developer): host-side timestamps of every enqueue step on stderr -- tells a host thread that blocks inside
// an "asynchronous" runtime call from a device-side dependency, which a kernel / copy trace cannot -- and, in the same mode, timing
// events behind every stage (device-side timeline of the call, printed at its end)
struct PipeTrace {
  bool on = false;
  std::chrono::steady_clock::time_point t0;
  std::vector<hipEvent_t> tev;   // [0] t = 0, then per chunk: H2D done, kernels done, D2H done
  void begin(bool on_, size_t nchunks) { on = on_; t0 = std::chrono::steady_clock::now(); tev.assign(1 + 3 * nchunks, nullptr); }
  void step(const char* what, size_t ch) const {
    if (on) fprintf(stderr, "[pipe] %8.1f us  chunk %zu  %s\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), ch, what);
  }
  void mark(size_t slot, hipStream_t st) {
    if (!on) return;
    if (hipEventCreate(&tev[slot]) == hipSuccess) hipEventRecord(tev[slot], st);
  }
  void end(const PipePlan& pl, bool ok) {
    for (size_t ch = 0; on && ok && ch < pl.nchunks(); ch++) {
      float t[3] = {0, 0, 0};
      for (int k = 0; k < 3; k++) if (tev[0] && tev[1 + 3 * ch + k]) hipEventElapsedTime(&t[k], tev[0], tev[1 + 3 * ch + k]);
      fprintf(stderr, "[pipe-dev] chunk %zu (%7zu items)  H2D done %7.1f us  kernels done %7.1f us  D2H done %7.1f us\n", ch, pl.cnt_of(ch), t[0] * 1e3, t[1] * 1e3, t[2] * 1e3);
    }
    for (hipEvent_t e : tev) if (e) hipEventDestroy(e);
  }
};
// One super-batch of at most `cap` items (everything fits in the device staging).  launch(d_in[], d_out[], count, stream)
// enqueues the kernels of one chunk on `stream`.  What its stages share: the plan (pipe_plan.hpp), what the kernels reach in place,
// the workers' copy groups and how far each stage has got.
template <typename Launch>
struct SuperBatch : PipePlan {
  bjj_ctx* const c;
  const size_t n;
  const PipeSpec& sp;
  const bool* const in_direct;
  const bool* const out_direct;
  Launch& launch;
  const bool chunk_out_ring = out_ring && !sp.out_at_end;   // pageable outputs travel chunk by chunk through the ring
  bool zc = false;                // zero-copy outputs: every output array pinned AND mapped into the device's address space
  size_t zi_chunks = 0;           // leading chunks whose launch reads the caller's arrays in place
  uint8_t* mapped_in[4] = {nullptr, nullptr, nullptr, nullptr};
  uint8_t* mapped_out[4] = {nullptr, nullptr, nullptr, nullptr};
  CopyPool* const pool = c->pool;
  std::vector<CopyGroup> g_in, g_out;
  size_t harvested = 0;           // chunks whose copy-out has been submitted (in order)
  size_t outs = 0;                // chunks whose D2H has been enqueued (in order)
  size_t fronts = 0;              // chunks whose H2D + kernels have been enqueued
  PipeTrace tr;

  // the plan of a super-batch; the two developer overrides are read once per entry point, on its first call
  static PipePlan plan(const bjj_ctx* c, size_t n, const PipeSpec& sp, const bool* in_direct, const bool* out_direct) {
    static const std::vector<size_t> forced = pipe_parse_schedule(getenv("BJJ_PIPE_SCHEDULE"));
    static const int parity_env = [] { const char* e = getenv("BJJ_PIPE_LANE_PARITY"); return e && (e[0] == '0' || e[0] == '1') ? e[0] - '0' : -1; }();   // developer A/B
    return pipe_plan({n, sp.n_in, sp.n_out, sp.in_stride, sp.out_stride, in_direct, out_direct, sp.extra_dev_per_item,
                      sp.first_chunk, sp.max_chunk, sp.tail_chunk, sp.last_on_priority_lane, sp.out_at_end,
                      c->pipe_first, c->pipe_chunk, c->pipe_env_schedule, &forced, parity_env});
  }
  // which arrays the kernels read / write through their device mappings (zc, zi_chunks), then the exact list opens on what they use
  int map_pinned_and_open() {
    const bool small_direct = sp.small_direct_max && n <= sp.small_direct_max && nchunks() == 1 && !sp.exact && c->pipe_small_direct;
    zc = (sp.zero_copy_out || small_direct) && !out_ring && sp.n_out > 0 && !sp.out_at_end && c->pipe_zero_copy;
    for (int i = 0; i < sp.n_out && zc; i++) {
      void* dp = nullptr;
      if (!out_direct[i] || ((uintptr_t)sp.out[i] & 15u) || hipHostGetDevicePointer(&dp, sp.out[i], 0) != hipSuccess || !dp) { (void)hipGetLastError(); zc = false; }   // (the kernels move 16-byte words)
      mapped_out[i] = (uint8_t*)dp;
    }
    // Calls of one or two chunks: every chunk.  Longer calls: the FIRST chunk only -- the head of the chain of launches starts at once instead
    // of behind its copy, and the copy-in of the chunks behind it, which keeps the two lanes' launches out of phase, starts earlier too.
    bool zi = (sp.zero_copy_in || small_direct) && !in_ring && sp.n_in > 0 && !sp.exact && c->pipe_zero_copy_in;
    for (int i = 0; i < sp.n_in && zi; i++) {
      void* dp = nullptr;
      if (!in_direct[i] || ((uintptr_t)sp.in[i] & 15u) || hipHostGetDevicePointer(&dp, (void*)sp.in[i], 0) != hipSuccess || !dp) { (void)hipGetLastError(); zi = false; }   // (the kernels move 16-byte words)
      mapped_in[i] = (uint8_t*)dp;
    }
    static const int zi_first_env = [] { const char* e = getenv("BJJ_PIPE_ZERO_COPY_IN_FIRST"); return e ? atoi(e) : 1; }();   // developer A/B: leading chunks of a long call that read in place
    if (small_direct && !(zi && zc)) { zi = zi && sp.zero_copy_in; zc = zc && sp.zero_copy_out; }   // both directions or the entry point's own rule
    zi_chunks = !zi ? 0 : (nchunks() <= 2 ? nchunks() : (size_t)zi_first_env);
    c->last_host_zero_copy = (zc ? 1u : 0u) | (zi_chunks == nchunks() ? 2u : 0u);
    c->k1_half_now = sp.k1_half && nchunks() >= 2;
    if (!sp.exact) return BJJ_OK;
    void* bi[4] = {}; void* bo[4] = {};
    for (int i = 0; i < sp.n_in; i++) bi[i] = c->dstage + d_in_off[i];
    for (int i = 0; i < sp.n_out; i++) bo[i] = zc ? (void*)mapped_out[i] : (void*)(c->dstage + d_out_off[i]);
    return sp.exact->open(n, bi, bo, sp.extra_dev_per_item ? c->dstage + d_extra_off : nullptr, zc);
  }
  // pageable inputs of chunk ch -> pin_in[ch % BUFS] (workers); the slot is free once the H2D of chunk ch - BUFS has run
  int submit_in(size_t ch) {
    const int b = (int)(ch % BJJ_PIPE_BUFS);
    if (!in_ring) return BJJ_OK;
    if (ch >= BJJ_PIPE_BUFS) HIPCK(hipEventSynchronize(c->ev_in[ch - BJJ_PIPE_BUFS]));
    for (int i = 0; i < sp.n_in; i++)
      if (!in_direct[i]) pool->submit(c->pin_in[b] + r_in_off[i], sp.in[i] + lo_of[ch] * sp.in_stride[i], cnt_of(ch) * sp.in_stride[i], &g_in[ch]);
    return BJJ_OK;
  }
  // chunk ch has left the device: pageable outputs pin_out[ch % BUFS] -> caller (workers)
  int harvest(size_t ch, bool block) {
    const int b = (int)(ch % BJJ_PIPE_BUFS);
    if (block) HIPCK(hipEventSynchronize(c->ev_out[ch]));
    else {
      const hipError_t q = hipEventQuery(c->ev_out[ch]);
      (void)hipGetLastError();
      if (q != hipSuccess) return 1;   // not yet
    }
    for (int i = 0; i < sp.n_out; i++)
      if (!out_direct[i]) pool->submit(sp.out[i] + lo_of[ch] * sp.out_stride[i], c->pin_out[b] + r_out_off[i], cnt_of(ch) * sp.out_stride[i], &g_out[ch]);
    return BJJ_OK;
  }
  // the pageable results of chunk ch are in the caller's memory: its pin_out slot is free
  int finish_out(size_t ch) {
    while (harvested <= ch) { int r = harvest(harvested, true); if (r) return r; harvested++; }
    pool->wait(&g_out[ch]);
    return BJJ_OK;
  }
  // H2D of chunk ch on s_in, its kernels on lane ch % 2 behind the copy's event, ev_k[ch] behind the kernels
  int enqueue_front(size_t ch) {
    const int b = (int)(ch % BJJ_PIPE_BUFS);
    const size_t lo = lo_of[ch], cnt = cnt_of(ch);
    tr.step("enqueue begin", ch);
    const bool zi = ch < zi_chunks;   // this chunk's launch reads the caller's arrays in place
    for (int i = 0; i < sp.n_in && !zi; i++)
      HIPCK(hipMemcpyAsync(c->dstage + d_in_off[i] + lo * sp.in_stride[i], in_direct[i] ? sp.in[i] + lo * sp.in_stride[i] : c->pin_in[b] + r_in_off[i],
                           cnt * sp.in_stride[i], hipMemcpyHostToDevice, c->s_in));
    if (!zi) HIPCK(hipEventRecord(c->ev_in[ch], c->s_in));
    tr.mark(1 + 3 * ch, c->s_in);                              // H2D done
    hipStream_t lane = ((ch + lane_flip) & 1) ? c->stream2 : c->stream;
    if (!zi) HIPCK(hipStreamWaitEvent(lane, c->ev_in[ch], 0));
    if (sp.exact) {   // the chunk's items onto the exact list: behind their copy, or behind their decompressions on the lane
      hipEvent_t ready = c->ev_in[ch];
      if (sp.exact->kind == ExactListStage::VERIFY_COMPRESSED) {
        int r = sp.exact->decompress(lo, cnt, lane); if (r) return r;
        HIPCK(hipEventRecord(c->ev_mid[ch], lane));
        ready = c->ev_mid[ch];
      }
      int r = sp.exact->scan(lo, cnt, ready); if (r) return r;
    }
    void* d_in[4]; void* d_out[4];
    for (int i = 0; i < sp.n_in; i++) d_in[i] = (zi ? mapped_in[i] : c->dstage + d_in_off[i]) + lo * sp.in_stride[i];
    for (int i = 0; i < sp.n_out; i++) d_out[i] = (zc ? mapped_out[i] : c->dstage + d_out_off[i]) + lo * sp.out_stride[i];
    int r = launch(d_in, d_out, cnt, (void*)lane); if (r) return r;
    HIPCK(hipEventRecord(c->ev_k[ch], lane));                  // behind a kernel: its completion signal, no extra packet
    if (sp.exact && ch + 1 == nchunks()) {   // every scan is enqueued; chunks ch and ch - 1 are the last of their lanes
      const hipEvent_t bulk_done[2] = {c->ev_k[ch], ch ? c->ev_k[ch - 1] : nullptr};
      r = sp.exact->close(bulk_done, ch ? 2 : 1); if (r) return r;
    }
    tr.mark(2 + 3 * ch, lane);                                 // kernels done
    tr.step("kernels enqueued", ch);
    return BJJ_OK;
  }
  // D2H of chunk ch, enqueued by the HOST once it has seen the chunk's kernels complete: the copy carries no device-side wait,
  // so s_out's hardware queue never holds a packet that another stream's kernel could get stuck behind
  int enqueue_out(size_t ch) {
    const int b = (int)(ch % BJJ_PIPE_BUFS);
    const size_t lo = lo_of[ch], cnt = cnt_of(ch);
    if (sp.out_at_end || zc) { tr.step("kernels seen complete", ch); return BJJ_OK; }   // nothing leaves chunk by chunk / the kernels wrote the caller's arrays themselves
    if (chunk_out_ring && ch >= BJJ_PIPE_BUFS) { int r = finish_out(ch - BJJ_PIPE_BUFS); if (r) return r; }   // frees pin_out[b]
    for (int i = 0; i < sp.n_out; i++)
      HIPCK(hipMemcpyAsync(out_direct[i] ? sp.out[i] + lo * sp.out_stride[i] : c->pin_out[b] + r_out_off[i], c->dstage + d_out_off[i] + lo * sp.out_stride[i],
                           cnt * sp.out_stride[i], hipMemcpyDeviceToHost, c->s_out));
    if (chunk_out_ring) HIPCK(hipEventRecord(c->ev_out[ch], c->s_out));   // only the staged path needs to know when ONE chunk has arrived
    tr.mark(3 + 3 * ch, c->s_out);                             // D2H done
    tr.step("D2H enqueued", ch);
    return BJJ_OK;
  }
  int drain_kernels(bool block, size_t upto) {   // D2H for the chunks < upto whose kernels have completed; block: wait for them
    while (outs < upto) {
      if (block) HIPCK(hipEventSynchronize(c->ev_k[outs]));
      else {
        const hipError_t q = hipEventQuery(c->ev_k[outs]);
        (void)hipGetLastError();
        if (q != hipSuccess) break;
      }
      { int r = enqueue_out(outs); if (r) return r; }
      outs++;
      while (chunk_out_ring && harvested < outs) {   // results that have already arrived: start their copy-out, do not wait
        const int r = harvest(harvested, false);
        if (r == 1) break;
        if (r) return r;
        harvested++;
      }
    }
    return BJJ_OK;
  }
  int body() {
    size_t next_in = 0;           // next chunk whose pageable inputs are handed to the workers (one chunk ahead of the enqueue)
    for (size_t ch = 0; ch < nchunks(); ch++) {
      while (next_in < nchunks() && next_in <= ch + 1) { int r = submit_in(next_in); if (r) return r; next_in++; }
      if (in_ring) pool->wait(&g_in[ch]);
      { int r = enqueue_front(ch); if (r) return r; }
      fronts = ch + 1;
      { int r = drain_kernels(false, fronts); if (r) return r; }   // only chunks that are enqueued can be drained
    }
    { int r = drain_kernels(true, nchunks()); if (r) return r; }
    if (chunk_out_ring) for (size_t ch = harvested; ch < nchunks(); ch++) { int r = finish_out(ch); if (r) return r; }
    if (chunk_out_ring) for (size_t ch = 0; ch < nchunks(); ch++) pool->wait(&g_out[ch]);
    if (sp.exact) { HIPCK(hipEventSynchronize(c->ev_tail)); tr.step("exact list complete", nchunks()); }
    if (sp.out_at_end) {   // the whole output arrays, once: pinned -> directly, pageable -> ring slot 0 -> workers
      for (int i = 0; i < sp.n_out; i++)
        HIPCK(hipMemcpyAsync(out_direct[i] ? sp.out[i] : c->pin_out[0] + r_out_off[i], c->dstage + d_out_off[i], n * sp.out_stride[i], hipMemcpyDeviceToHost, c->s_out));
      if (out_ring) {
        HIPCK(hipStreamSynchronize(c->s_out));
        for (int i = 0; i < sp.n_out; i++) if (!out_direct[i]) pool->submit(sp.out[i], c->pin_out[0] + r_out_off[i], n * sp.out_stride[i], &g_out[0]);
        pool->wait(&g_out[0]);
      }
    }
    HIPCK(hipStreamSynchronize(c->s_out));
    HIPCK(hipStreamSynchronize(c->stream));
    HIPCK(hipStreamSynchronize(c->stream2));
    return BJJ_OK;
  }
  void sync_pipe_streams() { hipStreamSynchronize(c->s_in); hipStreamSynchronize(c->stream); hipStreamSynchronize(c->stream2); hipStreamSynchronize(c->s_out); }
  // error path: nothing may still be writing into the caller's memory or reading the rings when we return
  void drain_after_error() {
    sync_pipe_streams();
    if (sp.exact) hipDeviceSynchronize();   // whatever the exact-list stage had enqueued on the scan stream
    (void)hipGetLastError();
    if (pool) for (size_t ch = 0; ch < nchunks(); ch++) { pool->wait(&g_in[ch]); pool->wait(&g_out[ch]); }
  }
  // key material went through the staging levels: wipe them (also on the error path) -- what THIS call can have used of them: the
  // rings keep the size of the largest call so far, and wiping all of it made a one-key call after a large one cost 0.3 ms more than its kernel
  void wipe_secret_staging() {
    sync_pipe_streams();
    if (c->dstage) hipMemsetAsync(c->dstage, 0, dev_tot, c->stream);
    const size_t slots = nchunks() < (size_t)BJJ_PIPE_BUFS ? nchunks() : (size_t)BJJ_PIPE_BUFS;
    for (size_t b = 0; b < slots; b++) {
      if (c->pin_in[b] && in_ring) secure_bzero(c->pin_in[b], in_ring < c->pin_in[b].bytes ? in_ring : c->pin_in[b].bytes);
      if (c->pin_out[b] && out_ring) secure_bzero(c->pin_out[b], out_ring < c->pin_out[b].bytes ? out_ring : c->pin_out[b].bytes);
    }
    hipStreamSynchronize(c->stream);
  }
};
template <typename Launch>
static int run_super_batch_body(bjj_ctx* c, size_t n, const PipeSpec& sp, const bool* in_direct, const bool* out_direct, Launch& launch, u32* chunks_out) {
  PipePlan pl = SuperBatch<Launch>::plan(c, n, sp, in_direct, out_direct);
  { int rc = ensure_pipe(c, pl.nchunks(), pl.dev_tot, pl.in_ring, pl.out_ring); if (rc) return rc; }
  SuperBatch<Launch> sb{std::move(pl), c, n, sp, in_direct, out_direct, launch};
  { int rc = sb.map_pinned_and_open(); if (rc) return rc; }
  *chunks_out += (u32)sb.nchunks();
  sb.g_in.resize(sb.nchunks()); sb.g_out.resize(sb.nchunks());
  static const bool trace = [] { const char* e = getenv("BJJ_PIPE_TRACE"); return e && e[0] == '1'; }();
  sb.tr.begin(trace, sb.nchunks());
  sb.tr.mark(0, c->s_in);   // t = 0
  int rc = sb.body();
  sb.tr.step("all chunks finished", sb.nchunks());
  if (!rc && sp.exact) { rc = sp.exact->finish(sp.out[0]); sb.tr.step("exact list finished on the host", sb.nchunks()); }
  sb.tr.end(sb, !rc);
  if (rc) sb.drain_after_error();
  if (sp.secret) sb.wipe_secret_staging();
  return rc;
}
// The body allocates (chunk schedule, copy groups, the workers' queue): a std::bad_alloc must not cross the extern "C" boundary,
// and nothing may still be copying into the caller's memory or out of the rings when the call returns (ADVICE r05).
template <typename Launch>
static int run_super_batch(bjj_ctx* c, size_t n, const PipeSpec& sp, const bool* in_direct, const bool* out_direct, Launch& launch, u32* chunks_out) {
  try {
    return run_super_batch_body(c, n, sp, in_direct, out_direct, launch, chunks_out);
  } catch (...) {
    // only the allocations at the head of the body can throw (the chunk schedule, the copy groups, the timing marks): no worker
    // holds a task yet (CopyPool::submit does not throw), the device has at most a list reset queued
    hipDeviceSynchronize();
    (void)hipGetLastError();
    return set_err(BJJ_E_NOMEM, "host-pointer pipeline: out of host memory");
  }
}
// Short calls on pinned memory without copies (PipeSpec::small_direct_max): as long as the entry point's short-call kernel is the one that runs
static size_t small_direct_items(size_t kernel_max) { return kernel_max < 256 ? kernel_max : 256; }
template <typename Launch>
static int run_pipelined(bjj_ctx* c, size_t n, const PipeSpec& sp, Launch launch) {
  ENTER_DEVICE(c->device);
  { int rc = ensure_pipe(c, 0, 0, 0, 0); if (rc) return rc; }   // streams, the chunk schedule, the knobs
  // ---- which arrays are pinned (copied directly) and which go through the pinned rings
  bool in_direct[4], out_direct[4];
  u32 n_direct = 0, n_staged = 0;
  size_t per_item = 0;
  for (int i = 0; i < sp.n_in; i++) { in_direct[i] = !c->force_staged && host_range_pinned(sp.in[i], n * sp.in_stride[i]); (in_direct[i] ? n_direct : n_staged)++; per_item += sp.in_stride[i]; }
  for (int i = 0; i < sp.n_out; i++) { out_direct[i] = !c->force_staged && host_range_pinned(sp.out[i], n * sp.out_stride[i]); (out_direct[i] ? n_direct : n_staged)++; per_item += sp.out_stride[i]; }
  per_item += sp.extra_dev_per_item;
  // ---- super-batches: what fits into the device staging budget at once (2^20 verifications are 202 MB)
  const size_t cap = pipe_super_batch_cap(c->pipe_budget, per_item, c->pipe_chunk);
  if (!cap) return set_err(BJJ_E_HIP, "host-pointer pipeline: not initialised (chunk size 0)");   // the loop below would never advance
  u32 chunks = 0;
  int rc = BJJ_OK;
  c->in_pipeline = true;
  for (size_t lo = 0; lo < n && !rc; lo += cap) {
    const size_t cnt = n - lo < cap ? n - lo : cap;
    PipeSpec sub = sp;
    for (int i = 0; i < sp.n_in; i++) sub.in[i] = sp.in[i] + lo * sp.in_stride[i];
    for (int i = 0; i < sp.n_out; i++) sub.out[i] = sp.out[i] + lo * sp.out_stride[i];
    rc = run_super_batch(c, cnt, sub, in_direct, out_direct, launch, &chunks);
  }
  c->in_pipeline = false;
  c->k1_half_now = false;
  c->last_host_direct = n_direct; c->last_host_staged = n_staged; c->last_host_chunks = chunks;
  if (!sp.zero_copy_out && !sp.small_direct_max) c->last_host_zero_copy &= ~1u;
  if (!sp.zero_copy_in && !sp.small_direct_max) c->last_host_zero_copy &= ~2u;
  // the call has synchronised for the caller: a verify / variable-base workgroup that gave up waiting for a table slot makes
  // it an error here, not at some later bjj_sync (ADVICE r04).  Only the pipeline's OWN streams have been waited for: while a
  // device-pointer launch of the caller is still in flight on one of the sets, its workgroups are popping and pushing the rings --
  // reading them now could miss an error that comes later (and clear rings_used, so that bjj_sync would skip the check), and
  // rebuilding one would hand a slot out twice.  The check then stays pending for the next synchronising call (ADVICE r05).
  if (!rc) {
    bool busy = false;
    for (const ScratchSet& S : c->set)
      if (S.have_last && hipEventQuery(S.ev_last) == hipErrorNotReady) busy = true;
    (void)hipGetLastError();
    if (!busy) rc = ctx_check_slot_queues(c, "host-pointer call");
  }
  return rc;
}
