// DEBUG HARNESS (tests only): the three inversion cores of fr.hpp side by side on the CPU, with the bound assertions of
// fr_inv_k1 (growth of d and e, exact divisions, g == 0 at the end) enabled.  Not part of libbjj_hip.so.
// Inputs are RAW representatives: a 32-byte little-endian integer X < 2r, taken as the N-form limbs of a Montgomery-form
// value, exactly what K1's epilogue hands to the inversion.  Outputs are the canonical (fr_canon) limbs as 32 bytes.
#define BJJ_DEBUG_BOUNDS 1
#include <string.h>
#include <thread>
#include "../../babyjubjub-rs_amd/csrc/fr.hpp"
using namespace bjj;
static Fr load_raw(const uint8_t* b) { u32 w[8]; memcpy(w, b, 32); return fr_from_words(w); }
static void store_raw(uint8_t* b, const Fr& a) { u32 w[8]; fr_to_words(fr_canon(a), w); memcpy(b, w, 32); }
static bool same3(const Fr& x, uint8_t* o /* 32 bytes or null */) {
  uint8_t k[32], g[32], f[32];
  store_raw(k, fr_inv_k1(x)); store_raw(g, fr_inv_gcd(x)); store_raw(f, fr_inv_fermat(x));
  if (o) memcpy(o, k, 32);
  return memcmp(k, g, 32) == 0 && memcmp(k, f, 32) == 0;
}
static u64 splitmix64(u64& s) {
  u64 z = (s += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}
extern "C" {
// 1 when fr_inv_k1, fr_inv_gcd and fr_inv_fermat agree byte for byte after fr_canon; out = fr_inv_k1's bytes
int emul_inv_k1_one(const uint8_t* x, uint8_t* out) { return same3(load_raw(x), out) ? 1 : 0; }
// `count` SplitMix64 values below 2r (255 random bits, rejected when >= 2r), as 8 streams (seed + stream index) of count / 8
// values on 8 threads -- the Fermat side of the comparison is 381 checked multiplications per value.  Returns the number of
// disagreements and, in `first_bad`, a disagreeing input.
static void splitmix_stream(u64 seed, long count, long* bad, uint8_t* first_bad) {
  constexpr u32 R2c[NL] = {0x2u, 0x1e1f593fu, 0x1cb848a1u, 0x0fa121e6u, 0x0b0ba506u, 0x05b68181u, 0x014dc282u, 0x1cb84c68u, 0x0060c89cu};
  u64 s = seed;
  for (long n = 0; n < count;) {
    u64 q[4] = {splitmix64(s), splitmix64(s), splitmix64(s), splitmix64(s) >> 1};
    u32 w[8];
    memcpy(w, q, 32);
    const Fr x = fr_from_words(w);
    bool below = false;   // x < 2r ?
    for (int i = NL - 1; i >= 0; i--) {
      if (x.v[i] != R2c[i]) { below = x.v[i] < R2c[i]; break; }
    }
    if (!below) continue;
    n++;
    if (!same3(x, nullptr)) { if ((*bad)++ == 0) memcpy(first_bad, w, 32); }
  }
}
long emul_inv_k1_splitmix(unsigned long long seed, long count, uint8_t* first_bad) {
  constexpr int T = 8;
  long bad[T] = {0};
  uint8_t fb[T][32];
  std::thread th[T];
  for (int t = 0; t < T; t++) th[t] = std::thread(splitmix_stream, (u64)seed + (u64)t, count / T + (t < count % T ? 1 : 0), &bad[t], fb[t]);
  long total = 0;
  for (int t = 0; t < T; t++) {
    th[t].join();
    if (bad[t] && total == 0) memcpy(first_bad, fb[t], 32);
    total += bad[t];
  }
  return total;
}
}
