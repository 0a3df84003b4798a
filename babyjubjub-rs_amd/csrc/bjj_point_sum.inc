// ---- signed point sums over CSR segments (k_point_sum.hip, point_sum.hpp, include/bjj_hip_point_sum.h); included by bjj_hip.hip --------
// argument checks of both forms, before any allocation
static int point_sum_check(bjj_ctx* c, size_t n, size_t m, const char* who) {
  if (!c) return set_err(BJJ_E_INVALID, std::string(who) + ": ctx is NULL");
  CHECK_N(n);
  if (m >> 32) return set_err(BJJ_E_INVALID, std::string(who) + ": at most 2^32 - 1 segments per call");
  if (m == 0 && n) return set_err(BJJ_E_INVALID, std::string(who) + ": m == 0 requires n == 0");
  return BJJ_OK;
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
  { int rc = grow_block(S->msm, L.bytes, "bjj_point_sum_dev", "point-sum scratch"); if (rc) return rc; }
  { int rc = set_enter(c, S, st); if (rc) return rc; }
  LAUNCHCK(bjjk::point_sum(st, L, (const uint8_t*)d_pts, (const uint8_t*)d_neg, n, (const uint64_t*)d_offsets, m, S->msm, (uint8_t*)d_out,
                           (unsigned long long*)d_first_off_curve),
           "bjj_point_sum_dev");
  return set_leave(c, S, st);
}
// Synchronous (Staged).  The offsets are checked here, before anything is enqueued; offsets, points and signs lie behind the scratch
// that L lays out, the results and the status words behind them.
int bjj_point_sum(bjj_ctx* c, const uint8_t* pts, const uint8_t* neg, size_t n, const uint64_t* offsets, size_t m, uint8_t* out_xy,
                  int64_t* out_first_off_curve) {
  { int rc = point_sum_check(c, n, m, "bjj_point_sum"); if (rc) return rc; }
  if (m == 0) return BJJ_OK;
  if (!offsets || !out_xy || !out_first_off_curve || (n && !pts)) return set_err(BJJ_E_INVALID, "bjj_point_sum: NULL buffer");
  if (offsets[0] != 0) return set_err(BJJ_E_INVALID, "bjj_point_sum: offsets[0] must be 0");
  for (size_t s = 0; s < m; s++)
    if (offsets[s] > offsets[s + 1]) return set_err(BJJ_E_INVALID, "bjj_point_sum: offsets decrease at segment " + std::to_string(s));
  if (offsets[m] != n) return set_err(BJJ_E_INVALID, "bjj_point_sum: offsets[m] must equal n");
  const bjjk::PointSumLayout L = bjjk::point_sum_layout(n);
  ENTER_DEVICE(c->device);
  Staged G(c, "bjj_point_sum", L.bytes);
  const int i_off = G.in(offsets, m + 1, 8), i_pts = G.in(pts, n, 64), i_neg = G.in_opt(neg, n, 1);
  const int i_out = G.out(out_xy, m, 64), i_st = G.out(out_first_off_curve, m, 8);
  { int rc = G.begin(G.S->msm, "point-sum scratch", true); if (rc) return rc; }
  LAUNCHCK(bjjk::point_sum(G.st, L, G.dev(i_pts), G.dev(i_neg), n, (const uint64_t*)G.dev(i_off), m, G.blk, G.dev(i_out),
                           (unsigned long long*)G.dev(i_st)),
           "bjj_point_sum");
  return G.finish();
}
