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
#include "../emul_support.hpp"

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
    Words raw;
    alignas(16) u32 sc[8];
    char tok[80];
    if (sscanf(p, "%79s", tok) != 1 || strlen(tok) != 64 || !parse_hex(tok, raw)) { fprintf(stderr, "bad input line: %s", line); return 2; }
    scalar_mod_l_weak(raw.w, sc, K);
    int bad = 0;
    for (int W = 4; W <= 28; W++) bad += check_width(sc, W, false);
    print_hex(sc); printf(" %d\n", bad);
    if (print)
      for (int W = 4; W <= 28; W++) check_width(sc, W, true);
  }
  return 0;
}
