// ---- signed point sums over CSR segments (k_point_sum.hip, point_sum.hpp, include/bjj_hip_point_sum.h); included by bjj_hip.hip --------
// argument checks of both forms, before any allocation
static int point_sum_check(bjj_ctx* c, size_t n, size_t m, const char* who) {
  if (!c) return set_err(BJJ_E_INVALID, std::string(who) + ": ctx is NULL");
  CHECK_N(n);
  if (m >> 32) return set_err(BJJ_E_INVALID, std::string(who) + ": at most 2^32 - 1 segments per call");
  if (m == 0 && n) return set_err(BJJ_E_INVALID, std::string(who) + ": m == 0 requires n == 0");
  return BJJ_OK;
}
static int ensure_point_sum(ScratchSet* S, size_t bytes, const char* who) {
  if (S->msm.grow(bytes) == hipSuccess) return BJJ_OK;
  (void)hipGetLastError();
  return set_err(BJJ_E_NOMEM, std::string(who) + ": cannot allocate " + std::to_string(bytes >> 20) + " MB of point-sum scratch");
}
int bjj_point_sum_dev(bjj_ctx* c, const void* d_pts, const void* d_neg, size_t n, const void* d_offsets, size_t m, void* d_out,
                      void* d_first_off_curve, void* stream) {
  { int rc = point_sum_check(c, n, m, "bjj_point_sum_dev"); if (rc) return rc; }
  if (m == 0) return BJJ_OK;
  if (n) CHECK_PTR(d_pts, "bjj_point_sum_dev");
  CHECK_PTR(d_offsets, "bjj_point_sum_dev"); CHECK_PTR(d_out, "bjj_point_sum_dev"); CHECK_PTR(d_first_off_curve, "bjj_point_sum_dev");
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  ENTER_DEVICE(c->device);
  ScratchSet* S = pick_set(c, st);
  const bjjk::PointSumLayout L = bjjk::point_sum_layout(n);
  { int rc = ensure_point_sum(S, L.bytes, "bjj_point_sum_dev"); if (rc) return rc; }
  { int rc = set_enter(c, S, st); if (rc) return rc; }
  LAUNCHCK(bjjk::point_sum(st, L, (const uint8_t*)d_pts, (const uint8_t*)d_neg, n, (const uint64_t*)d_offsets, m, S->msm, (uint8_t*)d_out,
                           (unsigned long long*)d_first_off_curve),
           "bjj_point_sum_dev");
  return set_leave(c, S, st);
}
// Synchronous.  The offsets are checked here, before anything is enqueued; the inputs are copied once, straight from the caller's
// arrays (pinned or pageable), into the set's block behind the scratch that L lays out, and the results come back the same way.
int bjj_point_sum(bjj_ctx* c, const uint8_t* pts, const uint8_t* neg, size_t n, const uint64_t* offsets, size_t m, uint8_t* out_xy,
                  int64_t* out_first_off_curve) {
  { int rc = point_sum_check(c, n, m, "bjj_point_sum"); if (rc) return rc; }
  if (m == 0) return BJJ_OK;
  if (!offsets || !out_xy || !out_first_off_curve || (n && !pts)) return set_err(BJJ_E_INVALID, "bjj_point_sum: NULL buffer");
  if (offsets[0] != 0) return set_err(BJJ_E_INVALID, "bjj_point_sum: offsets[0] must be 0");
  for (size_t s = 0; s < m; s++)
    if (offsets[s] > offsets[s + 1]) return set_err(BJJ_E_INVALID, "bjj_point_sum: offsets decrease at segment " + std::to_string(s));
  if (offsets[m] != n) return set_err(BJJ_E_INVALID, "bjj_point_sum: offsets[m] must equal n");
  hipStream_t st = c->stream;
  ENTER_DEVICE(c->device);
  ScratchSet* S = pick_set(c, st);
  const bjjk::PointSumLayout L = bjjk::point_sum_layout(n);
  const size_t o_off = L.bytes, o_pts = o_off + up256((m + 1) * 8), o_neg = o_pts + up256(n * 64), o_out = o_neg + up256(neg ? n : 0),
               o_st = o_out + up256(m * 64);
  { int rc = ensure_point_sum(S, o_st + up256(m * 8), "bjj_point_sum"); if (rc) return rc; }
  { int rc = set_enter(c, S, st); if (rc) return rc; }
  uint8_t* blk = S->msm;
  HIPCK(hipMemcpyAsync(blk + o_off, offsets, (m + 1) * 8, hipMemcpyHostToDevice, st));
  if (n) HIPCK(hipMemcpyAsync(blk + o_pts, pts, n * 64, hipMemcpyHostToDevice, st));
  if (n && neg) HIPCK(hipMemcpyAsync(blk + o_neg, neg, n, hipMemcpyHostToDevice, st));
  LAUNCHCK(bjjk::point_sum(st, L, blk + o_pts, neg ? blk + o_neg : nullptr, n, (const uint64_t*)(blk + o_off), m, blk, blk + o_out,
                           (unsigned long long*)(blk + o_st)),
           "bjj_point_sum");
  HIPCK(hipMemcpyAsync(out_xy, blk + o_out, m * 64, hipMemcpyDeviceToHost, st));
  HIPCK(hipMemcpyAsync(out_first_off_curve, blk + o_st, m * 8, hipMemcpyDeviceToHost, st));
  { int rc = set_leave(c, S, st); if (rc) return rc; }
  HIPCK(hipStreamSynchronize(st));
  return BJJ_OK;
}
