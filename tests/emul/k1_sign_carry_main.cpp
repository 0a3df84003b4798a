// DEBUG HARNESS (tests only; tests/test_k1_sign_carry_host.py): the sign-carrying recurrence of K1's overlap form (k_fixed.hip,
// BJJ_K1_SIGN_CARRY) on the CPU, as a stand-alone program (built with ASan + UBSan and BJJ_DEBUG_BOUNDS by the test, so that every
// fr_mul / fr_sub_lazy checks its operands' limb bounds).  It runs the functions the kernel runs -- niels_tform_state,
// ext_madd_state with its `flip`, ext_madd_forms (curve.hpp), scalar_mod_l_weak, digit_stream / digit_next (bjj_device.hpp) -- in
// the kernel's order, on table entries used exactly as stored, against fixed_base_mul on the same entries.
// Table entries: the window bases P_j = fixed_table_entry(1, j, W), digit k of a window by the table builder's own chain
// (fixed_table_chain with one link, from that base); the first entries built per width are compared with
// fixed_table_entry(k, j, W) itself.
// stdin:  "<W> <64 hex digits, most significant first>" per line
// stdout: "<W> <mismatches> <x of the result, 64 hex digits> <y>" per line; a failed bound aborts the program.
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <map>
#include <vector>
#include "../../babyjubjub-rs_amd/csrc/sign.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
#include "../emul_support.hpp"

// gather policy (bjj_device.hpp "gather policies") over a table that exists one entry at a time
struct Entries {
  int W = 0;
  std::vector<Niels> bases;
  std::map<size_t, Niels> memo;
  int checked = 0, bad = 0;
  void width(int w) {
    if (w == W) return;
    W = w; memo.clear(); bases.clear(); checked = 0;
    for (int j = 0; j < fixed_nwin(W); j++) bases.push_back(fixed_table_entry(1u, j, W, K));
  }
  const Niels& at(size_t slot) {
    auto it = memo.find(slot);
    if (it != memo.end()) return it->second;
    const size_t stride = fixed_stride(W);
    const int j = (int)(slot / stride);
    const u32 k = (u32)(slot % stride);
    alignas(16) u32 row[NIELS_WORDS] = {0};
    fixed_table_chain(row, bases[j], 0, k, 1, W, K);    // one link of the builder's chain, written as slot 0: T form
    Niels n = load_niels(row);
    if (j > 0) n.t2d = fr_canon(fr_mul(n.t2d, K.DP));   // windows beyond 0 store 2D'x'y (as fixed_base_accumulate converts)
    if (checked < 48) {
      checked++;
      if (!niels_limbs_equal(n, fixed_table_entry(k, j, W, K, j == 0))) bad++;
    }
    return memo.emplace(slot, n).first->second;
  }
};
static Entries g_entries;
struct GatherHost {
  struct Pending { Niels e; };
  static constexpr int kBuffers = 2;
  static int wave_max(int v) { return v; }
  void issue(size_t slot, Pending& p, int) const { p.e = g_entries.at(slot); }
  Niels finish(Pending& p, int) const { return p.e; }
};

// K1's overlap form with BJJ_K1_SIGN_CARRY, one item: R_0 = Q_0, R_j = (eps_j eps_{j-1}) R_{j-1} + Q_j, the result R_last (eps_last = +1)
static Ext sign_carry_mul(int W, int nwin, const u32 raw[8]) {
  u32 sc[8];
  scalar_mod_l_weak(raw, sc, K);
  DigitStream ds = digit_stream(sc, W);
  const GatherHost g;
  GatherHost::Pending p0, p;
  bool neg0, prev, neg;
  g.issue(digit_next(ds, neg0), p0, 0);
  g.issue(digit_next(ds, prev), p, 1);
  MaddState acc = niels_tform_state(g.finish(p0, 0), neg0 != prev, neg0 != prev);
  Niels cur = g.finish(p, 1);
  for (int j = 1; j + 1 < nwin; j++) {
    g.issue(digit_next(ds, neg), p, (j + 1) & 1);
    acc = ext_madd_forms(ext_madd_state(acc, cur, neg != prev));
    prev = neg;
    cur = g.finish(p, (j + 1) & 1);
  }
  if (prev) { fprintf(stderr, "negative top digit\n"); abort(); }   // eps_last = +1: no carry leaves the top window
  return ext_madd_state<false>(acc, cur);
}

static void affine_words(const Ext& p, u32 x[8], u32 y[8]) {   // canonical x', y of the a' = -1 curve
  const Fr zi = fr_inv(p.Z);
  fr_from_mont_words(fr_mul(p.X, zi), x);
  fr_from_mont_words(fr_mul(p.Y, zi), y);
}

int main() {
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    int W = 0;
    char tok[80];
    Words raw;
    if (sscanf(line, "%d %79s", &W, tok) != 2 || strlen(tok) != 64 || !parse_hex(tok, raw) || W < 4 || W > 28) { fprintf(stderr, "bad input line: %s", line); return 2; }
    g_entries.width(W);
    const int nwin = fixed_nwin(W);
    const Ext got = sign_carry_mul(W, nwin, raw.w);
    const Ext want = fixed_base_mul(GatherHost(), W, nwin, raw.w, K);
    u32 gx[8], gy[8], wx[8], wy[8];
    affine_words(got, gx, gy);
    affine_words(want, wx, wy);
    const int bad = (memcmp(gx, wx, 32) != 0) + (memcmp(gy, wy, 32) != 0) + g_entries.bad;
    printf("%d %d ", W, bad); print_hex(gx); printf(" "); print_hex(gy); printf("\n");
  }
  return 0;
}
