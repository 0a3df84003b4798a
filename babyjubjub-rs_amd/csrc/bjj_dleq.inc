// ---- a P + b Q, and Chaum-Pedersen proofs of discrete-log equality (k_dleq.hip, dleq.hpp, include/bjj_hip_dleq.h); included by bjj_hip.hip ----
// The kernels with per-lane tables are grid-strided over one resident set of workgroups and index the set's table block by global
// lane, two raw tables each: the block must hold cus * lanes_dleq lanes of them (it only ever grows; K2 and verify use a prefix).
static int dleq_tables(bjj_ctx* c, ScratchSet* S) {
  HIPCK(S->vb_tables.grow((size_t)c->cus * (size_t)c->lanes_dleq * BJJ_DLEQ_LANE_WORDS * sizeof(u32)));
  return BJJ_OK;
}
// l and the multiples of 8l: what scalar_mod_l and scalar_mod_order read of the constant block on the host
static const Consts& dleq_host_consts() {
  static const Consts K = [] {
    Consts k{};
    k.ORDER = Fr BJJ_K_ORDER; k.ORDER2 = Fr BJJ_K_ORDER2; k.ORDER4 = Fr BJJ_K_ORDER4; k.L = Fr BJJ_K_L;
    return k;
  }();
  return K;
}
// the tag as the kernels hash it: Montgomery form, reduced mod r by the conversion (what the kernels apply to a record)
static Fr dleq_tag(const uint8_t* tag) {
  u32 w[8];
  memcpy(w, tag, 32);
  return fr_to_mont_words(w);
}
#define DLEQ_DEV_PTR(p, who) \
  if (!(p) || !aligned16(p)) return set_err(BJJ_E_INVALID, std::string(who) + ": NULL or not 16-byte aligned device pointer")
// a scratch-set entry that also sizes the per-lane tables (SET_ENTER with dleq_tables before the set is entered)
#define DLEQ_SET_ENTER(c, stream, n)                                      \
  hipStream_t st = (stream) ? (hipStream_t)(stream) : (c)->stream;        \
  ENTER_DEVICE((c)->device);                                              \
  ScratchSet* S = pick_set((c), st);                                      \
  { int rc_ = ensure_scratch((c), S, (n)); if (rc_) return rc_;           \
    rc_ = dleq_tables((c), S); if (rc_) return rc_;                       \
    rc_ = set_enter((c), S, st); if (rc_) return rc_; }

// ---- bjj_mul_pair ------------------------------------------------------------------------------------------------------------------
static int mul_pair_check(bjj_ctx* c, size_t n, const char* who) {
  if (!c) return set_err(BJJ_E_INVALID, std::string(who) + ": ctx is NULL");
  CHECK_N(n);
  return BJJ_OK;
}
static hipError_t mul_pair_enqueue(bjj_ctx* c, ScratchSet* S, hipStream_t st, const void* p, const void* a, const void* q, const void* b,
                                   const void* add, size_t n, void* out, void* ok) {
  const PairArgs A = {(const uint8_t*)p, (const uint8_t*)q, (const uint8_t*)a, (const uint8_t*)b, (const uint8_t*)add};
  return bjjk::mul_pair(st, c->cus, c->lanes_dleq, A, n, (uint8_t*)out, (uint8_t*)ok, S->scratch, S->vb_tables);
}
int bjj_mul_pair_dev(bjj_ctx* c, const void* d_p_xy, const void* d_a, const void* d_q_xy, const void* d_b, const void* d_add_xy, size_t n,
                     void* d_out_xy, void* d_ok, void* stream) {
  const char* who = "bjj_mul_pair_dev";
  { int rc = mul_pair_check(c, n, who); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  DLEQ_DEV_PTR(d_p_xy, who); DLEQ_DEV_PTR(d_a, who); DLEQ_DEV_PTR(d_q_xy, who); DLEQ_DEV_PTR(d_b, who); DLEQ_DEV_PTR(d_out_xy, who);
  if (d_add_xy && !aligned16(d_add_xy)) return set_err(BJJ_E_INVALID, std::string(who) + ": not 16-byte aligned device pointer");
  if (!d_ok) return set_err(BJJ_E_INVALID, std::string(who) + ": d_ok is NULL");
  DLEQ_SET_ENTER(c, stream, n);
  LAUNCHCK_S(mul_pair_enqueue(c, S, st, d_p_xy, d_a, d_q_xy, d_b, d_add_xy, n, d_out_xy, d_ok), who);
  SET_LEAVE(c);
}
// Synchronous (Staged): P, a, Q, b and the addends (when given), then the results and the verdicts
int bjj_mul_pair(bjj_ctx* c, const uint8_t* p_xy, const uint8_t* a, const uint8_t* q_xy, const uint8_t* b, const uint8_t* add_xy, size_t n,
                 uint8_t* out_xy, uint8_t* ok) {
  const char* who = "bjj_mul_pair";
  { int rc = mul_pair_check(c, n, who); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  if (!p_xy || !a || !q_xy || !b || !out_xy || !ok) return set_err(BJJ_E_INVALID, std::string(who) + ": NULL buffer");
  ENTER_DEVICE(c->device);
  Staged G(c, who);
  { int rc = ensure_scratch(c, G.S, n); if (rc) return rc; }
  { int rc = dleq_tables(c, G.S); if (rc) return rc; }
  const int i_p = G.in(p_xy, n, 64), i_a = G.in(a, n, 32), i_q = G.in(q_xy, n, 64), i_b = G.in(b, n, 32), i_add = G.in_opt(add_xy, n, 64);
  const int i_out = G.out(out_xy, n, 64), i_ok = G.out(ok, n, 1);
  { int rc = G.begin(G.S->bases_io, "device staging"); if (rc) return rc; }
  LAUNCHCK_S(mul_pair_enqueue(c, G.S, G.st, G.dev(i_p), G.dev(i_a), G.dev(i_q), G.dev(i_b), G.dev(i_add), n, G.dev(i_out), G.dev(i_ok)), who);
  return G.finish();
}

// ---- bjj_dleq_verify ---------------------------------------------------------------------------------------------------------------
// argument checks of both forms; fills the two table descriptors and the tag
static int dleq_verify_check(bjj_ctx* c, const bjj_base* g, const bjj_base* pk, const uint8_t* tag, size_t n, const char* who, DleqVerifyArgs* A) {
  if (!c) return set_err(BJJ_E_INVALID, std::string(who) + ": ctx is NULL");
  if (!pk) return set_err(BJJ_E_INVALID, std::string(who) + ": pk is NULL (a missing key is not B8)");
  if (!c->user_bases.owns(pk)) return set_err(BJJ_E_INVALID, std::string(who) + ": pk is not a base of this context");
  if (g && !c->user_bases.owns(g)) return set_err(BJJ_E_INVALID, std::string(who) + ": g is not a base of this context");
  if (!tag) return set_err(BJJ_E_INVALID, std::string(who) + ": tag is NULL");
  CHECK_N(n);
  memset(A, 0, sizeof(*A));
  A->b[0] = base_desc(c, g);
  A->b[1] = base_desc(c, pk);
  A->tag = dleq_tag(tag);
  return BJJ_OK;
}
static hipError_t dleq_verify_enqueue(bjj_ctx* c, ScratchSet* S, hipStream_t st, DleqVerifyArgs& A, const void* c1, const void* d, const void* a,
                                      const void* b, const void* z, size_t n, void* ok) {
  A.c1 = (const uint8_t*)c1; A.d = (const uint8_t*)d; A.a = (const uint8_t*)a; A.b_xy = (const uint8_t*)b; A.z = (const uint8_t*)z;
  return bjjk::dleq_verify(st, c->cus, c->lanes_dleq, A, n, (uint8_t*)ok, S->vb_tables);
}
int bjj_dleq_verify_dev(bjj_ctx* c, const bjj_base* g, const bjj_base* pk, const uint8_t* tag, const void* d_c1_xy, const void* d_d_xy,
                        const void* d_a_xy, const void* d_b_xy, const void* d_z, size_t n, void* d_ok, void* stream) {
  const char* who = "bjj_dleq_verify_dev";
  DleqVerifyArgs A;
  { int rc = dleq_verify_check(c, g, pk, tag, n, who, &A); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  DLEQ_DEV_PTR(d_c1_xy, who); DLEQ_DEV_PTR(d_d_xy, who); DLEQ_DEV_PTR(d_a_xy, who); DLEQ_DEV_PTR(d_b_xy, who); DLEQ_DEV_PTR(d_z, who);
  if (!d_ok) return set_err(BJJ_E_INVALID, std::string(who) + ": d_ok is NULL");
  DLEQ_SET_ENTER(c, stream, n);
  LAUNCHCK_S(dleq_verify_enqueue(c, S, st, A, d_c1_xy, d_d_xy, d_a_xy, d_b_xy, d_z, n, d_ok), who);
  SET_LEAVE(c);
}
// Synchronous (Staged): C1, D, A, B and z, then the verdicts
int bjj_dleq_verify(bjj_ctx* c, const bjj_base* g, const bjj_base* pk, const uint8_t* tag, const uint8_t* c1_xy, const uint8_t* d_xy,
                    const uint8_t* a_xy, const uint8_t* b_xy, const uint8_t* z, size_t n, uint8_t* ok) {
  const char* who = "bjj_dleq_verify";
  DleqVerifyArgs A;
  { int rc = dleq_verify_check(c, g, pk, tag, n, who, &A); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  if (!c1_xy || !d_xy || !a_xy || !b_xy || !z || !ok) return set_err(BJJ_E_INVALID, std::string(who) + ": NULL buffer");
  ENTER_DEVICE(c->device);
  Staged G(c, who);
  { int rc = ensure_scratch(c, G.S, n); if (rc) return rc; }
  { int rc = dleq_tables(c, G.S); if (rc) return rc; }
  const int i_c1 = G.in(c1_xy, n, 64), i_d = G.in(d_xy, n, 64), i_a = G.in(a_xy, n, 64), i_b = G.in(b_xy, n, 64), i_z = G.in(z, n, 32);
  const int i_ok = G.out(ok, n, 1);
  { int rc = G.begin(G.S->bases_io, "device staging"); if (rc) return rc; }
  LAUNCHCK_S(dleq_verify_enqueue(c, G.S, G.st, A, G.dev(i_c1), G.dev(i_d), G.dev(i_a), G.dev(i_b), G.dev(i_z), n, G.dev(i_ok)), who);
  return G.finish();
}

// ---- bjj_dleq_prove ----------------------------------------------------------------------------------------------------------------
// What the host prepares of a call, before it returns: sk' = sk mod l (the kernel arguments of the last launch, and recoded for the
// shared-scalar launch) and the tag.  Wiped by its destructor on every return path of the function that holds it.
struct DleqProvePlan {
  CommonPlan P;
  DleqRespondArgs R;
  BasesArgs B;
  ~DleqProvePlan() { secure_bzero(&R, sizeof(R)); }
};
static int dleq_prove_check(bjj_ctx* c, const bjj_base* g, const uint8_t* sk, const uint8_t* tag, size_t n, const char* who, DleqProvePlan* L) {
  if (!c) return set_err(BJJ_E_INVALID, std::string(who) + ": ctx is NULL");
  if (g && !c->user_bases.owns(g)) return set_err(BJJ_E_INVALID, std::string(who) + ": g is not a base of this context");
  if (!sk) return set_err(BJJ_E_INVALID, std::string(who) + ": sk is NULL");
  if (!tag) return set_err(BJJ_E_INVALID, std::string(who) + ": tag is NULL");
  CHECK_N(n);
  memset(&L->R, 0, sizeof(L->R));
  memset(&L->B, 0, sizeof(L->B));
  u32 raw[8];
  memcpy(raw, sk, 32);
  scalar_mod_l(raw, L->R.sk, dleq_host_consts());
  common_plan(c, (const uint8_t*)L->R.sk, false, &L->P);   // sk' < l: the reduction mod 8l of the recoding leaves it alone
  secure_bzero(raw, sizeof(raw));
  L->R.tag = dleq_tag(tag);
  L->B.t = 1;
  L->B.b[0] = base_desc(c, g);
  return BJJ_OK;
}
// The chain on `st` with the set S entered; no synchronisation between the launches.  z holds w' = w mod l from the first launch to the last.
static int dleq_prove_enqueue(bjj_ctx* c, ScratchSet* S, hipStream_t st, DleqProvePlan& L, const void* c1, const void* w, size_t n, void* d,
                              void* a, void* b, void* z, void* ok, const char* who) {
  const uint8_t* pts = (const uint8_t*)c1;
  LAUNCHCK_S(bjjk::dleq_nonce(st, grid_for(c, n, c->occ_dleq_respond), (const uint8_t*)w, n, (uint8_t*)z), who);
  LAUNCHCK_S(common_enqueue(c, S, st, L.P, bjjk::COMMON_POINT, pts, nullptr, n, (uint8_t*)d, (uint8_t*)ok), who);          // D = sk' C1, ok = 1 / 2
  L.B.b[0].scalars = (const uint8_t*)z;
  LAUNCHCK_S(bjjk::mul_bases(st, c->cus, c->lanes_bases, L.B, n, (uint8_t*)a, S->scratch), who);                            // A = w' G
  int kv = 0;
  { int rc = var_base_form(c, S, st, n, &kv); if (rc) return rc; }
  // B = w' C1; an off-curve C1 is skipped (no list, no exact kernel: the last launch zeroes the item)
  LAUNCHCK_S(bjjk::mul_var_base_main(st, c->cus, c->lanes_var, kv, pts, (const uint8_t*)z, 8, n, (uint8_t*)b, S->scratch, S->vb_tables, nullptr,
                                     S->slotq2, S->slot_cap2 | ((u32)c->xccs << 16)), who);
  L.R.c1 = pts; L.R.d = (uint8_t*)d; L.R.a = (uint8_t*)a; L.R.b_xy = (uint8_t*)b; L.R.z = (uint8_t*)z;
  LAUNCHCK_S(bjjk::dleq_respond(st, grid_for(c, n, c->occ_dleq_respond), L.R, n, (const uint8_t*)ok), who);
  return BJJ_OK;
}
int bjj_dleq_prove_dev(bjj_ctx* c, const bjj_base* g, const uint8_t* sk, const uint8_t* tag, const void* d_c1_xy, const void* d_w, size_t n,
                       void* d_d_xy, void* d_a_xy, void* d_b_xy, void* d_z, void* d_ok, void* stream) {
  const char* who = "bjj_dleq_prove_dev";
  DleqProvePlan L;
  { int rc = dleq_prove_check(c, g, sk, tag, n, who, &L); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  DLEQ_DEV_PTR(d_c1_xy, who); DLEQ_DEV_PTR(d_w, who); DLEQ_DEV_PTR(d_d_xy, who); DLEQ_DEV_PTR(d_a_xy, who); DLEQ_DEV_PTR(d_b_xy, who);
  DLEQ_DEV_PTR(d_z, who);
  if (!d_ok) return set_err(BJJ_E_INVALID, std::string(who) + ": d_ok is NULL");
  SET_ENTER(c, stream, n, false);
  { int rc = dleq_prove_enqueue(c, S, st, L, d_c1_xy, d_w, n, d_d_xy, d_a_xy, d_b_xy, d_z, d_ok, who); if (rc) return rc; }
  SET_LEAVE(c);
}
// Synchronous (Staged): C1 and w, then D, A, B, z and the verdicts
int bjj_dleq_prove(bjj_ctx* c, const bjj_base* g, const uint8_t* sk, const uint8_t* tag, const uint8_t* c1_xy, const uint8_t* w, size_t n,
                   uint8_t* d_xy, uint8_t* a_xy, uint8_t* b_xy, uint8_t* z, uint8_t* ok) {
  const char* who = "bjj_dleq_prove";
  DleqProvePlan L;
  { int rc = dleq_prove_check(c, g, sk, tag, n, who, &L); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  if (!c1_xy || !w || !d_xy || !a_xy || !b_xy || !z || !ok) return set_err(BJJ_E_INVALID, std::string(who) + ": NULL buffer");
  ENTER_DEVICE(c->device);
  Staged G(c, who);
  { int rc = ensure_scratch(c, G.S, n); if (rc) return rc; }
  const int i_c1 = G.in(c1_xy, n, 64), i_w = G.in(w, n, 32);
  const int i_d = G.out(d_xy, n, 64), i_a = G.out(a_xy, n, 64), i_b = G.out(b_xy, n, 64), i_z = G.out(z, n, 32), i_ok = G.out(ok, n, 1);
  { int rc = G.begin(G.S->bases_io, "device staging"); if (rc) return rc; }
  { int rc = dleq_prove_enqueue(c, G.S, G.st, L, G.dev(i_c1), G.dev(i_w), n, G.dev(i_d), G.dev(i_a), G.dev(i_b), G.dev(i_z), G.dev(i_ok), who);
    if (rc) return rc; }
  { int rc = G.finish(); if (rc) return rc; }
  return ctx_check_slot_queues(c, who);
}
