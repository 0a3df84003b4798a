// DEBUG HARNESS (tests only): the per-item body of bjj_k_*_verify_set and the per-thread bodies of the set's build and check kernels
// (csrc/signer_set.hpp, what k_signer_set.hip launches) on the CPU with limb / value-bound assertions and a gather policy that
// refuses a slot outside the table it reads -- a stand-alone program, so that it also runs under AddressSanitizer and
// UndefinedBehaviorSanitizer as it is (tests/test_signer_set_host.py builds it twice).  Not linked into libbjj_hip.so.
//
// stdin:  "K <count>" and <count> lines "<x> <y>"  the keys (hex, on the curve; coordinates >= r are reduced)
//         "I <count>" and <count> lines "<idx> <rx> <ry> <s> <msg>" (hex; idx any 32-bit value): the items
// Tables: the set's at W = 4 and W = 5, each ONE allocation built by set_window_base / set_fill_chain thread by thread; B8 at W = 4
// as a CONTEXT's table (mod l, fixed_nwin windows).
// stdout: "check <table> <bad>"      set_check_entry summed over the set (tables 0, 1), the B8 table's induction check (table 2)
//         "tform <W> <signer> <ok>"  window 0 of that signer holds 2x'y in its third word, window 1 does not
//         "e <W> <i> <verdict>"      EdDSA verdict of item i over the set of width W
//         "s <W> <i> <verdict>"      Schnorr verdict
#define BJJ_DEBUG_BOUNDS 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../babyjubjub-rs_amd/csrc/signer_set.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
using namespace bjj;
static const Consts K = {
    BJJ_K_A, BJJ_K_D, BJJ_K_F, BJJ_K_FINV_PLAIN, BJJ_K_FINV, BJJ_K_L_R1, BJJ_K_L_R2, BJJ_K_DP, BJJ_K_D2P, BJJ_K_DPINV, BJJ_K_B8X, BJJ_K_B8Y, BJJ_K_TS_G, BJJ_K_HALFQ,
    BJJ_K_ORDER, BJJ_K_ORDER2, BJJ_K_ORDER4, BJJ_K_L, BJJ_K_L2, BJJ_K_L4,
    BJJ_K_POSEIDON_CF, BJJ_K_POSEIDON_KP, BJJ_K_POSEIDON_SP, BJJ_K_POSEIDON_AL, BJJ_K_POSEIDON_M, BJJ_K_POSEIDON_CAB,
    BJJ_K_TS_NEG, BJJ_K_TS_HALF, BJJ_K_TS_HASH};

struct Words { alignas(16) u32 w[8]; };
static bool parse_hex(const char* s, Words& out) {
  const size_t len = strlen(s);
  if (len == 0 || len > 64) return false;
  memset(out.w, 0, sizeof(out.w));
  for (size_t i = 0; i < len; i++) {
    const char c = s[len - 1 - i];
    const int v = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
    if (v < 0) return false;
    out.w[i / 8] |= (u32)v << (4 * (i % 8));
  }
  return true;
}
static bool read_words(Words* out, size_t count) {
  char tok[80];
  for (size_t i = 0; i < count; i++)
    if (scanf("%79s", tok) != 1 || !parse_hex(tok, out[i])) return false;
  return true;
}
static bool read_header(const char* name, size_t& count) {
  char tok[80];
  return scanf("%79s %zu", tok, &count) == 2 && !strcmp(tok, name) && count <= 100000;
}
static u32* aligned(std::vector<u32>& v) { return (u32*)(((uintptr_t)v.data() + 15) & ~(uintptr_t)15); }

// GatherPerLane that knows the extent of the two tables an item reads: a slot past the end of the table in use ends the program
struct GatherBounded {
  struct Pending { Niels e; };
  static constexpr int kBuffers = 2;
  const u32* table;
  const u32 *t0, *t1;
  size_t n0, n1;
  static int wave_max(int v) { return v; }
  void issue(size_t slot, Pending& p, int) const {
    const size_t limit = table == t0 ? n0 : table == t1 ? n1 : 0;
    if (slot >= limit) { fprintf(stderr, "gather out of bounds: slot %zu of %zu\n", slot, limit); abort(); }
    p.e = load_niels(table + slot * NIELS_WORDS);
  }
  Niels finish(Pending& p, int) const { return p.e; }
};

struct SetTable {
  int W = 0, nwin = 0;
  size_t k = 0, eps = 0;
  std::vector<u32> tv, bv;
  const u32* keys = nullptr;
  // thread by thread what build_signer_set launches: k * nwin window bases, then every chain
  void build(const u32* keys_, size_t k_, int W_, u32 chain) {
    keys = keys_; k = k_; W = W_; nwin = base_nwin(W); eps = (size_t)set_entries_per_signer(W);
    if (!set_slots_fit(k, W)) abort();
    tv.assign(k * eps * NIELS_WORDS + 4, 0xA5A5A5A5u);
    bv.assign(k * (size_t)nwin * NIELS_WORDS + 4, 0);
    for (u64 t = 0; t < k * (u64)nwin; t++) set_window_base(aligned(bv), keys, t, W, nwin, K);
    const u64 cpw = (fixed_stride(W) + chain - 1) / chain;
    for (u64 t = 0; t < k * (u64)nwin * cpw; t++) set_fill_chain(aligned(tv), aligned(bv), t, W, nwin, chain, K);
  }
  unsigned long long check() {
    unsigned long long bad = 0;
    for (u64 e = 0; e < k * eps; e++) bad += (unsigned long long)set_check_entry(aligned(tv), aligned(bv), keys, e, W, nwin, K);
    return bad;
  }
  // third word of entry (window j, digit 1) of signer s: 2x'y in window 0, 2D'x'y elsewhere
  bool tform_as_documented(size_t s) {
    bool ok = true;
    for (int j = 0; j < 2; j++) {
      const Niels e = load_niels(aligned(tv) + (s * eps + (size_t)j * fixed_stride(W) + 1) * NIELS_WORDS);
      const Fr dsq = fr_sub(fr_sqr(e.ypx), fr_sqr(e.ymx));
      const bool plain = fr_eq(dsq, fr_dbl(e.t2d)), withd = fr_eq(fr_mul(dsq, K.DP), fr_dbl(e.t2d));
      ok = ok && (j == 0 ? plain : withd);
    }
    return ok;
  }
};

int main() {
  size_t nk = 0, ni = 0;
  if (!read_header("K", nk) || nk == 0) { fprintf(stderr, "bad K line\n"); return 2; }
  std::vector<Words> kxy(2 * nk);
  if (!read_words(kxy.data(), 2 * nk)) { fprintf(stderr, "bad key\n"); return 2; }
  if (!read_header("I", ni)) { fprintf(stderr, "bad I line\n"); return 2; }
  std::vector<Words> items(5 * ni + 1);
  if (!read_words(items.data(), 5 * ni)) { fprintf(stderr, "bad item\n"); return 2; }

  std::vector<u32> keyv(nk * SET_KEY_WORDS + 4, 0);
  u32* keys = aligned(keyv);
  for (size_t j = 0; j < nk; j++) {
    u32 xy[16];
    memcpy(xy, kxy[2 * j].w, 32); memcpy(xy + 8, kxy[2 * j + 1].w, 32);
    const SignerPoint pk = signer_point(xy);
    if (!ref_on_curve(pk.x, pk.y, K)) { fprintf(stderr, "key %zu is not on the curve\n", j); return 2; }
    set_key_store(keys + j * SET_KEY_WORDS, pk);
  }
  SetTable T[2];
  T[0].build(keys, nk, 4, 3);
  T[1].build(keys, nk, 5, 8);
  // the context's B8 table, as tests/signer_emul builds it
  const int bw = 4, bnwin = fixed_nwin(bw);
  const size_t bstride = fixed_stride(bw);
  std::vector<u32> b8t(bstride * (size_t)bnwin * NIELS_WORDS + 4, 0), b8b((size_t)bnwin * NIELS_WORDS + 4, 0);
  for (int j = 0; j < bnwin; j++) store_niels(aligned(b8b) + (size_t)j * NIELS_WORDS, base_table_entry(K.B8X, K.B8Y, 1u, j, bw, K));
  for (int j = 0; j < bnwin; j++)
    fixed_table_chain(aligned(b8t), load_niels(aligned(b8b) + (size_t)j * NIELS_WORDS), (size_t)j * bstride, 0u, (u32)bstride, bw, K);
  unsigned long long b8bad = 0;
  for (int j = 0; j < bnwin; j++)
    for (size_t d = 0; d < bstride; d++) b8bad += (unsigned long long)base_table_check_slot(aligned(b8t), aligned(b8b), j, (u32)d, bw, bnwin, K.B8X, K.B8Y, K);
  for (int t = 0; t < 2; t++) printf("check %d %llu\n", t, T[t].check());
  printf("check 2 %llu\n", b8bad);
  for (int t = 0; t < 2; t++)
    for (size_t s = 0; s < nk; s++) printf("tform %d %zu %d\n", T[t].W, s, T[t].tform_as_documented(s) ? 1 : 0);

  for (int t = 0; t < 2; t++) {
    SetArgs A;
    memset(&A, 0, sizeof(A));
    A.T.table = aligned(T[t].tv); A.T.W = T[t].W; A.T.nwin = T[t].nwin; A.T.mod_l = 0;
    A.L.table = aligned(b8t); A.L.W = bw; A.L.nwin = bnwin; A.L.mod_l = 1;
    A.keys = keys; A.k = (u32)nk; A.eps = (u32)T[t].eps;
    const GatherBounded g = {A.T.table, A.T.table, A.L.table, nk * T[t].eps, bstride * (size_t)bnwin};
    for (size_t i = 0; i < ni; i++) {
      const Words* it = &items[5 * i];   // idx, then rx, ry read as ONE 64-byte record
      alignas(16) u32 r[16];
      memcpy(r, it[1].w, 32); memcpy(r + 8, it[2].w, 32);
      printf("e %d %zu %d\n", T[t].W, i, verify_set_item<false>(A, g, it[0].w[0], r, it[3].w, it[4].w, K));
      printf("s %d %zu %d\n", T[t].W, i, verify_set_item<true>(A, g, it[0].w[0], r, it[3].w, it[4].w, K));
    }
  }
  return 0;
}
