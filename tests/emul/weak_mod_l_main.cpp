// DEBUG HARNESS (tests only; tests/test_k1_weak_mod_l_host.py): scalar_mod_l_weak (bjj_device.hpp), the reduction K1's overlap
// form feeds its digit stream with, run on the CPU as a stand-alone program (built with ASan + UBSan by the test).
// stdin: one 256-bit integer per line, 64 hex digits, most significant first; a leading "D " asks for the digits too.
// stdout, per input:  <result, 64 hex digits> <number of failed digit checks over W = 4 .. 28>
//   a digit check fails when, over fixed_nwin(W) windows of digit_stream / digit_next, a slot lies outside its window's
//   fixed_stride(W) entries, the signed digits do not sum to the result, or a carry is left after the last window;
//   after a "D " input follow 25 lines  "W <W> <slot>:<neg> ..."  for the plain-integer model of the test.
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include "../../babyjubjub-rs_amd/csrc/sign.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
using namespace bjj;
static const Consts K = {
    BJJ_K_A, BJJ_K_D, BJJ_K_F, BJJ_K_FINV_PLAIN, BJJ_K_FINV, BJJ_K_L_R1, BJJ_K_L_R2, BJJ_K_DP, BJJ_K_D2P, BJJ_K_DPINV, BJJ_K_B8X, BJJ_K_B8Y, BJJ_K_TS_G, BJJ_K_HALFQ,
    BJJ_K_ORDER, BJJ_K_ORDER2, BJJ_K_ORDER4, BJJ_K_L, BJJ_K_L2, BJJ_K_L4,
    BJJ_K_POSEIDON_CF, BJJ_K_POSEIDON_KP, BJJ_K_POSEIDON_SP, BJJ_K_POSEIDON_AL, BJJ_K_POSEIDON_M, BJJ_K_POSEIDON_CAB,
    BJJ_K_TS_NEG, BJJ_K_TS_HALF, BJJ_K_TS_HASH};

static int hexval(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }

// one width: returns the number of failed checks; prints the digits when asked
static int check_width(const u32 sc[8], int W, bool print) {
  const int nwin = fixed_nwin(W);
  const size_t stride = fixed_stride(W);
  DigitStream ds = digit_stream(sc, W);
  long long acc[10] = {0};   // sum of sign * digit * 2^(W j), in 32-bit positions, not yet normalised
  int bad = 0;
  if (print) printf("W %d", W);
  for (int j = 0; j < nwin; j++) {
    bool neg;
    const size_t slot = digit_next(ds, neg);
    if (print) printf(" %zu:%d", slot, neg ? 1 : 0);
    if (slot < (size_t)j * stride || slot >= (size_t)(j + 1) * stride) { bad++; continue; }
    const unsigned long long dig = slot - (size_t)j * stride;   // <= 2^27
    const int bit = W * j, word = bit >> 5, off = bit & 31;
    const unsigned long long v = dig << off;                   // < 2^59
    const long long lo = (long long)(v & 0xffffffffull), hi = (long long)(v >> 32);
    acc[word] += neg ? -lo : lo;
    acc[word + 1] += neg ? -hi : hi;
  }
  if (print) printf("\n");
  if (ds.carry != 0) bad++;
  long long c = 0;
  for (int i = 0; i < 10; i++) {
    c += acc[i];
    const long long w = c & 0xffffffffll;
    c >>= 32;   // arithmetic: c may be negative
    if (w != (long long)(i < 8 ? sc[i] : 0u)) { bad++; break; }
  }
  if (c != 0) bad++;
  return bad;
}

int main() {
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    const char* p = line;
    bool print = false;
    if (p[0] == 'D' && p[1] == ' ') { print = true; p += 2; }
    alignas(16) u32 raw[8] = {0}, sc[8];
    int n = 0;
    for (; n < 64 && hexval(p[n]) >= 0; n++) {}
    if (n != 64) { fprintf(stderr, "bad input line: %s", line); return 2; }
    for (int i = 0; i < 64; i++) raw[7 - i / 8] |= (u32)hexval(p[i]) << (4 * (7 - i % 8));
    scalar_mod_l_weak(raw, sc, K);
    int bad = 0;
    for (int W = 4; W <= 28; W++) bad += check_width(sc, W, false);
    printf("%08x%08x%08x%08x%08x%08x%08x%08x %d\n", sc[7], sc[6], sc[5], sc[4], sc[3], sc[2], sc[1], sc[0], bad);
    if (print)
      for (int W = 4; W <= 28; W++) check_width(sc, W, true);
  }
  return 0;
}
