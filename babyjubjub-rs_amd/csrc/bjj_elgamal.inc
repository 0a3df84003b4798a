// ---- encryption and re-randomisation in one launch (k_elgamal.hip, elgamal.hpp, include/bjj_hip_elgamal.h); included by bjj_hip.hip ----
// argument checks of both forms; fills the three chain descriptors: r over G, m over G (the short chain), r over PK
static int elgamal_check(bjj_ctx* c, const bjj_base* g, const bjj_base* pk, const void* add_c1, const void* add_c2, size_t n, const char* who,
                         ElgamalArgs* A) {
  if (!c) return set_err(BJJ_E_INVALID, std::string(who) + ": ctx is NULL");
  if (!pk) return set_err(BJJ_E_INVALID, std::string(who) + ": pk is NULL (a missing key is not B8)");
  if (!c->user_bases.owns(pk)) return set_err(BJJ_E_INVALID, std::string(who) + ": pk is not a base of this context");
  if (g && !c->user_bases.owns(g)) return set_err(BJJ_E_INVALID, std::string(who) + ": g is not a base of this context");
  if (!add_c1 != !add_c2) return set_err(BJJ_E_INVALID, std::string(who) + ": the add arrays come both or neither");
  CHECK_N(n);
  memset(A, 0, sizeof(*A));
  const BaseDesc G = base_desc(c, g), P = base_desc(c, pk);
  A->b[0] = EgChain{G.table, G.W, G.nwin, G.mod_l ? EG_R_MOD_L : EG_R_MOD_ORDER};
  A->b[1] = EgChain{G.table, G.W, elgamal_nwin_m(G.W), EG_M};
  A->b[2] = EgChain{P.table, P.W, P.nwin, EG_R_MOD_ORDER};
  return BJJ_OK;
}
// One launch on `st`; the set's scratch holds two records per item.
static hipError_t elgamal_enqueue(bjj_ctx* c, ScratchSet* S, hipStream_t st, ElgamalArgs& A, const void* m, const void* r, const void* add_c1,
                                  const void* add_c2, size_t n, void* out_c1, void* out_c2, void* ok) {
  A.m = (const uint64_t*)m; A.r = (const uint8_t*)r; A.add_c1 = (const uint8_t*)add_c1; A.add_c2 = (const uint8_t*)add_c2;
  return bjjk::elgamal_encrypt(st, c->cus, c->lanes_elgamal, A, n, (uint8_t*)out_c1, (uint8_t*)out_c2, (uint8_t*)ok, S->scratch);
}
#define ELGAMAL_DEV_OPT(p, who) \
  if ((p) && !aligned16(p)) return set_err(BJJ_E_INVALID, std::string(who) + ": not 16-byte aligned device pointer")

int bjj_elgamal_encrypt_dev(bjj_ctx* c, const bjj_base* g, const bjj_base* pk, const void* d_m, const void* d_r, const void* d_add_c1_xy,
                            const void* d_add_c2_xy, size_t n, void* d_out_c1_xy, void* d_out_c2_xy, void* d_ok, void* stream) {
  const char* who = "bjj_elgamal_encrypt_dev";
  ElgamalArgs A;
  { int rc = elgamal_check(c, g, pk, d_add_c1_xy, d_add_c2_xy, n, who, &A); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  CHECK_PTR(d_r, who); CHECK_PTR(d_out_c1_xy, who); CHECK_PTR(d_out_c2_xy, who);
  ELGAMAL_DEV_OPT(d_m, who); ELGAMAL_DEV_OPT(d_add_c1_xy, who); ELGAMAL_DEV_OPT(d_add_c2_xy, who);
  if (d_add_c1_xy && !d_ok) return set_err(BJJ_E_INVALID, std::string(who) + ": d_ok is NULL (required with add arrays)");
  SET_ENTER(c, stream, 2 * n, false);
  LAUNCHCK_S(elgamal_enqueue(c, S, st, A, d_m, d_r, d_add_c1_xy, d_add_c2_xy, n, d_out_c1_xy, d_out_c2_xy, d_ok), who);
  SET_LEAVE(c);
}
// Synchronous (Staged): m, r and the two add arrays as given, then the two point arrays and the verdicts
int bjj_elgamal_encrypt(bjj_ctx* c, const bjj_base* g, const bjj_base* pk, const uint64_t* m, const uint8_t* r, const uint8_t* add_c1_xy,
                        const uint8_t* add_c2_xy, size_t n, uint8_t* out_c1_xy, uint8_t* out_c2_xy, uint8_t* ok) {
  const char* who = "bjj_elgamal_encrypt";
  ElgamalArgs A;
  { int rc = elgamal_check(c, g, pk, add_c1_xy, add_c2_xy, n, who, &A); if (rc) return rc; }
  if (n == 0) return BJJ_OK;
  if (!r || !out_c1_xy || !out_c2_xy) return set_err(BJJ_E_INVALID, std::string(who) + ": NULL buffer");
  if (add_c1_xy && !ok) return set_err(BJJ_E_INVALID, std::string(who) + ": ok is NULL (required with add arrays)");
  ENTER_DEVICE(c->device);
  Staged G(c, who);
  { int rc = ensure_scratch(c, G.S, 2 * n); if (rc) return rc; }
  const int i_m = G.in_opt(m, n, 8), i_r = G.in(r, n, 32), i_a1 = G.in_opt(add_c1_xy, n, 64), i_a2 = G.in_opt(add_c2_xy, n, 64);
  const int i_c1 = G.out(out_c1_xy, n, 64), i_c2 = G.out(out_c2_xy, n, 64), i_ok = G.out_opt(ok, n, 1);
  { int rc = G.begin(G.S->bases_io, "device staging"); if (rc) return rc; }
  LAUNCHCK_S(elgamal_enqueue(c, G.S, G.st, A, G.dev(i_m), G.dev(i_r), G.dev(i_a1), G.dev(i_a2), n, G.dev(i_c1), G.dev(i_c2), G.dev(i_ok)), who);
  return G.finish();
}
