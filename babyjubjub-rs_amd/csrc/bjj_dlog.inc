// ---- batched small-range discrete logarithms (k_dlog.hip, dlog.hpp, include/bjj_hip_dlog.h); included by bjj_hip.hip -----------------
// The default table width: of the tables measured (16, 20, 22, 24 baby bits) the one with the fastest 32-bit search -- 29.2 .. 31.1 ms
// for 2^20 items against 120.4 .. 127.0 ms at 22 bits, for 512 MiB instead of 128 (DESIGN.md section 13, profiles/dlog.txt).
#define BJJ_DLOG_DEFAULT_BABY_BITS 24
static_assert(BJJ_DLOG_MAX_GIANT_BITS == BJJ_DLOG_GIANT_BITS, "include/bjj_hip_dlog.h and dlog.hpp disagree");
// violated conditions of the finished table: entries not found under their own y, slots with a value out of range, and one more
// when the occupied slots do not number 2^b + 1
static int dlog_run_check(bjj_ctx* c, const bjj_dlog_table* t, unsigned long long* bad, const char* who) {
  unsigned long long h[2] = {0, 0};
  { int rc = device_counters(c, 2, h, who, [&](unsigned long long* d_bad) {
      return bjjk::dlog_check_table(c->stream, c->cus * 8, t->slots, t->params, t->b, d_bad); });
    if (rc) return rc; }
  *bad = h[0] + (h[1] != dlog_entries(t->b) ? 1ull : 0ull);
  return BJJ_OK;
}
int bjj_dlog_table_create(bjj_ctx* c, const uint8_t* point_xy, int baby_bits, bjj_dlog_table** out) {
  CHECK_CTX(c, "bjj_dlog_table_create");
  if (!out) return set_err(BJJ_E_INVALID, "bjj_dlog_table_create: out is NULL");
  if (baby_bits != 0 && (baby_bits < BJJ_DLOG_MIN_BABY_BITS || baby_bits > BJJ_DLOG_MAX_BABY_BITS))
    return set_err(BJJ_E_INVALID, "bjj_dlog_table_create: baby_bits must be 0 (default, 24) or 4..28");
  const int b = baby_bits ? baby_bits : BJJ_DLOG_DEFAULT_BABY_BITS;
  u32 xy[16];
  if (point_xy) {
    memcpy(xy, point_xy, 64);
    if (!point_words_on_curve(xy)) return set_err(BJJ_E_INVALID, "bjj_dlog_table_create: the point is not on the curve");
  }
  ENTER_DEVICE(c->device);
  bjj_dlog_table* t = new (std::nothrow) bjj_dlog_table();
  if (!t) return set_err(BJJ_E_NOMEM, "bjj_dlog_table_create: out of host memory");
  t->ctx = c; t->b = b;
  // the small block first: the order of the point is known before the table is asked for
  u32 hp[DLOG_PARAM_WORDS];
  hipError_t e = t->params.grow(DLOG_PARAM_WORDS * sizeof(u32), NO_WAIT);
  if (e != hipSuccess) { (void)hipGetLastError(); delete t; return set_err(BJJ_E_NOMEM, "bjj_dlog_table_create: cannot allocate the table"); }
  e = bjjk::dlog_setup_table(c->stream, t->params, b, point_xy ? xy : nullptr);
  if (e == hipSuccess) e = hipMemcpyAsync(hp, t->params, sizeof(hp), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) { delete t; return set_err(BJJ_E_HIP, std::string("bjj_dlog_table_create: setup failed: ") + hipGetErrorString(e)); }
  if (hp[DLOG_P_SMALL] != 0) {
    delete t;
    return set_err(BJJ_E_INVALID, "bjj_dlog_table_create: 8 * G is the identity (a base of order <= 8 has no unique logarithms)");
  }
  memcpy(t->base_xy, hp + DLOG_P_XY, 64);
  const size_t bytes = (size_t)dlog_slots(b) * sizeof(unsigned long long);
  DevBlock<unsigned long long> d_failed;
  e = t->slots.grow(bytes, NO_WAIT);
  if (e == hipSuccess) e = d_failed.grow(sizeof(unsigned long long), NO_WAIT);
  if (e != hipSuccess) {
    (void)hipGetLastError(); delete t;
    return set_err(BJJ_E_NOMEM, "bjj_dlog_table_create: cannot allocate the table (" + std::to_string(bytes >> 20) + " MB)");
  }
  unsigned long long failed = 1;
  e = hipMemsetAsync(t->slots, 0, bytes, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_failed, 0, sizeof(unsigned long long), c->stream);
  if (e == hipSuccess) e = bjjk::dlog_build_table(c->stream, t->slots, t->params, b, d_failed);
  if (e == hipSuccess) e = hipMemcpyAsync(&failed, d_failed, sizeof(failed), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) { delete t; return set_err(BJJ_E_HIP, std::string("bjj_dlog_table_create: table build failed: ") + hipGetErrorString(e)); }
  unsigned long long bad = 1;   // a handle that exists is a table that passed (the rule of bjj_base_create)
  { int rc = dlog_run_check(c, t, &bad, "bjj_dlog_table_create"); if (rc) { delete t; return rc; } }
  if (failed != 0 || bad != 0) {
    delete t;
    return set_err(BJJ_E_HIP, "bjj_dlog_table_create: the table failed its self-check (" + std::to_string(bad + failed) + " conditions)");
  }
  try { c->user_dlogs.add(t); } catch (...) { delete t; return set_err(BJJ_E_NOMEM, "bjj_dlog_table_create: out of host memory"); }
  *out = t;
  return BJJ_OK;
}
int bjj_dlog_table_free(bjj_ctx* c, bjj_dlog_table* t) {
  CHECK_CTX(c, "bjj_dlog_table_free");
  if (!t) return BJJ_OK;
  if (!c->user_dlogs.owns(t)) return set_err(BJJ_E_INVALID, "bjj_dlog_table_free: not a table of this context");
  ENTER_DEVICE(c->device);
  { int rc = ctx_wait_enqueued(c); if (rc) return rc; }   // launches that read the table
  c->user_dlogs.drop(t);
  return BJJ_OK;
}
int bjj_dlog_table_info(const bjj_dlog_table* t, int* baby_bits, uint64_t* entries, uint64_t* table_bytes) {
  if (!t) return set_err(BJJ_E_INVALID, "bjj_dlog_table_info: table is NULL");
  if (baby_bits) *baby_bits = t->b;
  if (entries) *entries = dlog_entries(t->b);
  if (table_bytes) *table_bytes = (uint64_t)t->slots.bytes;
  return BJJ_OK;
}
int bjj_dlog_table_check(bjj_ctx* c, const bjj_dlog_table* t, uint64_t* n_bad) {
  CHECK_CTX(c, "bjj_dlog_table_check");
  if (!t || !n_bad) return set_err(BJJ_E_INVALID, "bjj_dlog_table_check: NULL argument");
  if (!c->user_dlogs.owns(t)) return set_err(BJJ_E_INVALID, "bjj_dlog_table_check: not a table of this context");
  ENTER_DEVICE(c->device);
  unsigned long long bad = 0;
  { int rc = dlog_run_check(c, t, &bad, "bjj_dlog_table_check"); if (rc) return rc; }
  *n_bad = (uint64_t)bad;
  return BJJ_OK;
}
int bjj_dlog_table_base(const bjj_dlog_table* t, uint8_t* out_xy) {
  if (!t || !out_xy) return set_err(BJJ_E_INVALID, "bjj_dlog_table_base: NULL argument");
  memcpy(out_xy, t->base_xy, 64);
  return BJJ_OK;
}
int bjj_dlog_max_range_bits(const bjj_dlog_table* t) { return t ? dlog_max_range_bits(t->b) : -1; }

// argument checks of both forms, in an order that lets the first three answer without a device or a live context
static int dlog_check_args(bjj_ctx* c, const bjj_dlog_table* t, size_t n, int range_bits, const char* who) {
  if (!c) return set_err(BJJ_E_INVALID, std::string(who) + ": ctx is NULL");
  if (!t) return set_err(BJJ_E_INVALID, std::string(who) + ": table is NULL");
  if (range_bits < 1 || range_bits > dlog_max_range_bits(BJJ_DLOG_MAX_BABY_BITS))
    return set_err(BJJ_E_INVALID, std::string(who) + ": range_bits must be 1 .. baby_bits + 1 + BJJ_DLOG_MAX_GIANT_BITS");
  if (!c->user_dlogs.owns(t)) return set_err(BJJ_E_INVALID, std::string(who) + ": table is not a dlog table of this context");
  if (range_bits > dlog_max_range_bits(t->b))
    return set_err(BJJ_E_INVALID, std::string(who) + ": range_bits must be 1 .. " + std::to_string(dlog_max_range_bits(t->b)) + " for this table");
  CHECK_N(n);
  return BJJ_OK;
}
// The launches of one call.  A launch covers `items` consecutive items and giant steps s0 .. s1 - 1 with items * (s1 - s0) <=
// the context's bound and s1 - s0 <= BJJ_DLOG_LAUNCH_STEPS_PER_ITEM: as many steps as the bound allows for all n items, at most
// that cap, and where even BJJ_DLOG_LAUNCH_STEPS_MIN steps of all items exceed the bound, fewer items per launch.  A later launch
// finds an item's state in ok[i] (BJJ_DLOG_IN_FLIGHT = go on; the launch with the last step writes 0 instead) and walks to its first
// step by a 16-bit ladder, so nothing but the outputs lives between launches.
static hipError_t dlog_enqueue(bjj_ctx* c, hipStream_t st, const bjj_dlog_table* t, const uint8_t* pts, size_t n, int range_bits,
                               unsigned long long* out_m, uint8_t* ok) {
  const uint64_t nsteps = dlog_steps(t->b, range_bits), bound = c->dlog_launch_steps;
  uint64_t steps = bound / n;
  if (steps < BJJ_DLOG_LAUNCH_STEPS_MIN) steps = BJJ_DLOG_LAUNCH_STEPS_MIN;
  if (steps > BJJ_DLOG_LAUNCH_STEPS_PER_ITEM) steps = BJJ_DLOG_LAUNCH_STEPS_PER_ITEM;
  if (steps > nsteps) steps = nsteps;
  uint64_t items = bound / steps;
  if (items > n) items = n;
  for (uint64_t i0 = 0; i0 < n; i0 += items) {
    const uint64_t cnt = n - i0 < items ? n - i0 : items;
    for (uint64_t s0 = 0; s0 < nsteps; s0 += steps) {
      const uint64_t s1 = s0 + steps < nsteps ? s0 + steps : nsteps;
      const hipError_t e = bjjk::dlog_search(st, t->slots, t->params, t->b, pts + i0 * 64, (size_t)cnt, range_bits, (uint32_t)s0, (uint32_t)s1,
                                             s1 == nsteps, out_m + i0, ok + i0);
      if (e != hipSuccess) return e;
    }
  }
  return hipSuccess;
}
int bjj_dlog_dev(bjj_ctx* c, const bjj_dlog_table* t, const void* d_pts_xy, size_t n, int range_bits, void* d_out_m, void* d_ok, void* stream) {
  { int rc = dlog_check_args(c, t, n, range_bits, "bjj_dlog_dev"); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  if (!d_pts_xy || !d_out_m || !aligned16(d_pts_xy) || !aligned16(d_out_m))
    return set_err(BJJ_E_INVALID, "bjj_dlog_dev: NULL or not 16-byte aligned device pointer");
  if (!d_ok) return set_err(BJJ_E_INVALID, "bjj_dlog_dev: d_ok is NULL");
  DEV_ENTER(c, stream);
  LAUNCHCK_S(dlog_enqueue(c, st, t, (const uint8_t*)d_pts_xy, n, range_bits, (unsigned long long*)d_out_m, (uint8_t*)d_ok), "bjj_dlog_dev");
  DEV_LEAVE(c);
}
// Synchronous (Staged): the records, then the logarithms and the verdicts
int bjj_dlog(bjj_ctx* c, const bjj_dlog_table* t, const uint8_t* pts_xy, size_t n, int range_bits, uint64_t* out_m, uint8_t* ok) {
  { int rc = dlog_check_args(c, t, n, range_bits, "bjj_dlog"); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  if (!pts_xy || !out_m || !ok) return set_err(BJJ_E_INVALID, "bjj_dlog: NULL buffer");
  ENTER_DEVICE(c->device);
  Staged G(c, "bjj_dlog");
  const int i_pts = G.in(pts_xy, n, 64), i_m = G.out(out_m, n, 8), i_ok = G.out(ok, n, 1);
  { int rc = G.begin(G.S->bases_io, "device staging"); if (rc) return rc; }
  LAUNCHCK_S(dlog_enqueue(c, G.st, t, G.dev(i_pts), n, range_bits, (unsigned long long*)G.dev(i_m), G.dev(i_ok)), "bjj_dlog");
  return G.finish();
}
