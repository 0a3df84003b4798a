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
#include "../emul_support.hpp"

struct SetTable {
  int W = 0, nwin = 0;
  size_t k = 0, eps = 0;
  Aligned<u32> tv, bv;
  const u32* keys = nullptr;
  // thread by thread what build_signer_set launches: k * nwin window bases, then every chain
  void build(const u32* keys_, size_t k_, int W_, u32 chain) {
    keys = keys_; k = k_; W = W_; nwin = base_nwin(W); eps = (size_t)set_entries_per_signer(W);
    if (!set_slots_fit(k, W)) abort();
    tv = Aligned<u32>(k * eps * NIELS_WORDS, 0xA5A5A5A5u);
    bv = Aligned<u32>(k * (size_t)nwin * NIELS_WORDS);
    for (u64 t = 0; t < k * (u64)nwin; t++) set_window_base(bv.p(), keys, t, W, nwin, K);
    const u64 cpw = (fixed_stride(W) + chain - 1) / chain;
    for (u64 t = 0; t < k * (u64)nwin * cpw; t++) set_fill_chain(tv.p(), bv.p(), t, W, nwin, chain, K);
  }
  unsigned long long check() {
    unsigned long long bad = 0;
    for (u64 e = 0; e < k * eps; e++) bad += (unsigned long long)set_check_entry(tv.p(), bv.p(), keys, e, W, nwin, K);
    return bad;
  }
  // third word of entry (window j, digit 1) of signer s: 2x'y in window 0, 2D'x'y elsewhere
  bool tform_as_documented(size_t s) {
    bool ok = true;
    for (int j = 0; j < 2; j++) {
      const Niels e = load_niels(tv.p() + (s * eps + (size_t)j * fixed_stride(W) + 1) * NIELS_WORDS);
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

  Aligned<u32> keyv(nk * SET_KEY_WORDS);
  u32* keys = keyv.p();
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
  HostTable b8;   // the context's B8 table, one chain per window
  b8.build(K.B8X, K.B8Y, 4, true, (u32)fixed_stride(4));
  for (int t = 0; t < 2; t++) printf("check %d %llu\n", t, T[t].check());
  printf("check 2 %llu\n", b8.check());
  for (int t = 0; t < 2; t++)
    for (size_t s = 0; s < nk; s++) printf("tform %d %zu %d\n", T[t].W, s, T[t].tform_as_documented(s) ? 1 : 0);

  for (int t = 0; t < 2; t++) {
    SetArgs A;
    memset(&A, 0, sizeof(A));
    A.T.table = T[t].tv.p(); A.T.W = T[t].W; A.T.nwin = T[t].nwin; A.T.mod_l = 0;
    A.L = b8.desc();
    A.keys = keys; A.k = (u32)nk; A.eps = (u32)T[t].eps;
    const GatherBounded<2> g = {A.T.table, {{A.T.table, nk * T[t].eps}, {A.L.table, b8.slots()}}};
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
