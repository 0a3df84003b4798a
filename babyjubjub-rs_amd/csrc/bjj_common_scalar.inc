// ---- one scalar, many points (k_common_scalar.hip, common_scalar.hpp, include/bjj_hip_common_scalar.h); included by bjj_hip.hip -------
// BJJ_COMMON_FORM (read once at bjj_init): "naf" / "0" forces the table-free form, "table" / "1" the table form; anything else, or
// unset: the multiplication count of common_scalar.hpp decides per call.
static int common_form_from_env() {
  const char* e = getenv("BJJ_COMMON_FORM");
  if (!e) return -1;
  if (!strcmp(e, "naf") || !strcmp(e, "0")) return CS_FORM_NAF;
  if (!strcmp(e, "table") || !strcmp(e, "1")) return CS_FORM_TABLE;
  return -1;
}
// the three multiples of the group order scalar_mod_order reads; nothing else of the constant block is needed on the host
static const Consts& common_host_consts() {
  static const Consts K = [] {
    Consts k{};
    k.ORDER = Fr BJJ_K_ORDER; k.ORDER2 = Fr BJJ_K_ORDER2; k.ORDER4 = Fr BJJ_K_ORDER4;
    return k;
  }();
  return K;
}
// The scalar is read, reduced mod 8l and recoded here, before the call returns; what is left of it on the stack is wiped -- the
// plan by its destructor, on every return path of the function that holds it.
struct CommonPlan {
  CsDigits D;
  int form;
  ~CommonPlan() { secure_bzero(this, sizeof(*this)); }
};
static void common_plan(const bjj_ctx* c, const uint8_t* scalar, bool negate, CommonPlan* P) {
  u32 raw[8];
  memcpy(raw, scalar, 32);
  CsDigits naf, w5;
  const int wn = cs_recode(raw, negate, CS_FORM_NAF, &naf, common_host_consts());
  const int ww = cs_recode(raw, negate, CS_FORM_TABLE, &w5, common_host_consts());
  P->form = c->common_form >= 0 ? c->common_form : cs_choose_form(wn, ww);
  P->D = P->form == CS_FORM_TABLE ? w5 : naf;
  secure_bzero(raw, sizeof(raw)); secure_bzero(&naf, sizeof(naf)); secure_bzero(&w5, sizeof(w5));
}
// One launch on `st` with the set S entered.  The table form works in K2's per-lane tables and takes its slots from K2's queue,
// which holds one slot per workgroup K2 can have resident: bjj_init has checked that this kernel cannot have more.
static hipError_t common_enqueue(bjj_ctx* c, ScratchSet* S, hipStream_t st, const CommonPlan& P, int epi, const uint8_t* pts, const uint8_t* add,
                                 size_t n, uint8_t* out, uint8_t* ok) {
  if (P.form == CS_FORM_TABLE) c->rings_used = true;
  c->last_common_form = P.form;
  return bjjk::mul_common(st, P.form, epi, P.D, pts, add, n, out, ok, S->scratch, S->vb_tables, S->slotq2, S->slot_cap2 | ((u32)c->xccs << 16));
}
static int common_check(bjj_ctx* c, const void* scalar, size_t n, const char* who) {
  if (!c) return set_err(BJJ_E_INVALID, std::string(who) + ": ctx is NULL");
  if (!scalar) return set_err(BJJ_E_INVALID, std::string(who) + ": the scalar is NULL");
  CHECK_N(n);
  return BJJ_OK;
}
#define COMMON_DEV_PTR(p, who) \
  if (!(p) || !aligned16(p)) return set_err(BJJ_E_INVALID, std::string(who) + ": NULL or not 16-byte aligned device pointer")

static int mul_common_dev_impl(bjj_ctx* c, const uint8_t* scalar, const void* d_pts, const void* d_add, int subtract, size_t n, void* d_out,
                               void* d_ok, void* stream, int epi, const char* who) {
  { int rc = common_check(c, scalar, n, who); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  COMMON_DEV_PTR(d_pts, who);
  if (epi != bjjk::COMMON_SUBGROUP) COMMON_DEV_PTR(d_out, who);
  if (d_add && !aligned16(d_add)) return set_err(BJJ_E_INVALID, std::string(who) + ": not 16-byte aligned device pointer");
  if (!d_ok) return set_err(BJJ_E_INVALID, std::string(who) + ": d_ok is NULL");
  CommonPlan P;
  common_plan(c, scalar, subtract != 0, &P);
  SET_ENTER(c, stream, n, false);
  LAUNCHCK_S(common_enqueue(c, S, st, P, epi, (const uint8_t*)d_pts, (const uint8_t*)d_add, n, (uint8_t*)d_out, (uint8_t*)d_ok), who);
  SET_LEAVE(c);
}
int bjj_mul_common_dev(bjj_ctx* c, const uint8_t* scalar, const void* d_pts_xy, const void* d_add_xy, int subtract, size_t n, void* d_out_xy,
                       void* d_ok, void* stream) {
  return mul_common_dev_impl(c, scalar, d_pts_xy, d_add_xy, subtract, n, d_out_xy, d_ok, stream, bjjk::COMMON_POINT, "bjj_mul_common_dev");
}
// l as 32 little-endian bytes: the scalar of the subgroup check
static void common_l_bytes(uint8_t out[32]) {
  u32 w[8];
  fr_to_words(Fr BJJ_K_L, w);
  memcpy(out, w, 32);
}
int bjj_in_subgroup_dev(bjj_ctx* c, const void* d_pts_xy, size_t n, void* d_ok, void* stream) {
  uint8_t l[32];
  common_l_bytes(l);
  return mul_common_dev_impl(c, l, d_pts_xy, nullptr, 0, n, nullptr, d_ok, stream, bjjk::COMMON_SUBGROUP, "bjj_in_subgroup_dev");
}
// Synchronous host forms (Staged): the points and the addends (when given), then the results (but for the subgroup check) and the verdicts
static int mul_common_host_impl(bjj_ctx* c, const uint8_t* scalar, const uint8_t* pts, const uint8_t* add, int subtract, size_t n, uint8_t* out,
                                uint8_t* ok, int epi, const char* who) {
  { int rc = common_check(c, scalar, n, who); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  const bool point = epi != bjjk::COMMON_SUBGROUP;
  if (!pts || !ok || (point && !out)) return set_err(BJJ_E_INVALID, std::string(who) + ": NULL buffer");
  CommonPlan P;
  common_plan(c, scalar, subtract != 0, &P);
  ENTER_DEVICE(c->device);
  Staged G(c, who);
  { int rc = ensure_scratch(c, G.S, n); if (rc) return rc; }
  const int i_pts = G.in(pts, n, 64), i_add = G.in_opt(add, n, 64), i_out = G.out_opt(point ? out : nullptr, n, 64), i_ok = G.out(ok, n, 1);
  { int rc = G.begin(G.S->bases_io, "device staging"); if (rc) return rc; }
  LAUNCHCK_S(common_enqueue(c, G.S, G.st, P, epi, G.dev(i_pts), G.dev(i_add), n, G.dev(i_out), G.dev(i_ok)), who);
  { int rc = G.finish(); if (rc) return rc; }
  return ctx_check_slot_queues(c, who);
}
int bjj_mul_common(bjj_ctx* c, const uint8_t* scalar, const uint8_t* pts_xy, const uint8_t* add_xy, int subtract, size_t n, uint8_t* out_xy,
                   uint8_t* ok) {
  return mul_common_host_impl(c, scalar, pts_xy, add_xy, subtract, n, out_xy, ok, bjjk::COMMON_POINT, "bjj_mul_common");
}
int bjj_in_subgroup(bjj_ctx* c, const uint8_t* pts_xy, size_t n, uint8_t* ok) {
  uint8_t l[32];
  common_l_bytes(l);
  return mul_common_host_impl(c, l, pts_xy, nullptr, 0, n, nullptr, ok, bjjk::COMMON_SUBGROUP, "bjj_in_subgroup");
}

// ---- decryption in one call: M_i = C2_i - sk * C1_i into the set's block, then the launch chain of bjj_dlog_dev over it ---------------
static int decrypt_check(bjj_ctx* c, const bjj_dlog_table* t, const uint8_t* sk, size_t n, int range_bits, const char* who) {
  if (!c) return set_err(BJJ_E_INVALID, std::string(who) + ": ctx is NULL");
  if (!sk) return set_err(BJJ_E_INVALID, std::string(who) + ": sk is NULL");
  return dlog_check_args(c, t, n, range_bits, who);
}
static int decrypt_block(ScratchSet* S, size_t n, const char* who) {
  if (S->common_m.grow(n * 64) == hipSuccess) return BJJ_OK;
  (void)hipGetLastError();
  return set_err(BJJ_E_NOMEM, std::string(who) + ": cannot allocate " + std::to_string((n * 64) >> 20) + " MB for the decrypted points");
}
int bjj_elgamal_decrypt_dev(bjj_ctx* c, const bjj_dlog_table* t, const uint8_t* sk, const void* d_c1_xy, const void* d_c2_xy, size_t n,
                            int range_bits, void* d_out_m, void* d_ok, void* stream) {
  const char* who = "bjj_elgamal_decrypt_dev";
  { int rc = decrypt_check(c, t, sk, n, range_bits, who); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  COMMON_DEV_PTR(d_c1_xy, who); COMMON_DEV_PTR(d_c2_xy, who); COMMON_DEV_PTR(d_out_m, who);
  if (!d_ok) return set_err(BJJ_E_INVALID, std::string(who) + ": d_ok is NULL");
  CommonPlan P;
  common_plan(c, sk, true, &P);
  SET_ENTER(c, stream, n, false);
  { int rc = decrypt_block(S, n, who); if (rc) return rc; }
  LAUNCHCK_S(common_enqueue(c, S, st, P, bjjk::COMMON_DECRYPT, (const uint8_t*)d_c1_xy, (const uint8_t*)d_c2_xy, n, S->common_m, nullptr), who);
  LAUNCHCK_S(dlog_enqueue(c, st, t, S->common_m, n, range_bits, (unsigned long long*)d_out_m, (uint8_t*)d_ok), who);
  SET_LEAVE(c);
}
int bjj_elgamal_decrypt(bjj_ctx* c, const bjj_dlog_table* t, const uint8_t* sk, const uint8_t* c1_xy, const uint8_t* c2_xy, size_t n,
                        int range_bits, uint64_t* out_m, uint8_t* ok) {
  const char* who = "bjj_elgamal_decrypt";
  { int rc = decrypt_check(c, t, sk, n, range_bits, who); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  if (!c1_xy || !c2_xy || !out_m || !ok) return set_err(BJJ_E_INVALID, std::string(who) + ": NULL buffer");
  CommonPlan P;
  common_plan(c, sk, true, &P);
  ENTER_DEVICE(c->device);
  Staged G(c, who);   // C1 and C2, then the logarithms and the verdicts
  { int rc = ensure_scratch(c, G.S, n); if (rc) return rc; }
  { int rc = decrypt_block(G.S, n, who); if (rc) return rc; }
  const int i_c1 = G.in(c1_xy, n, 64), i_c2 = G.in(c2_xy, n, 64), i_m = G.out(out_m, n, 8), i_ok = G.out(ok, n, 1);
  { int rc = G.begin(G.S->bases_io, "device staging"); if (rc) return rc; }
  LAUNCHCK_S(common_enqueue(c, G.S, G.st, P, bjjk::COMMON_DECRYPT, G.dev(i_c1), G.dev(i_c2), n, G.S->common_m, nullptr), who);
  LAUNCHCK_S(dlog_enqueue(c, G.st, t, G.S->common_m, n, range_bits, (unsigned long long*)G.dev(i_m), G.dev(i_ok)), who);
  { int rc = G.finish(); if (rc) return rc; }
  return ctx_check_slot_queues(c, who);
}
