// Stand-alone driver of the harness beside it, for -fsanitize=address,undefined (tests/test_point_sum_host.py): the mixed case of
// the CPU tests -- 300 multiples of B8 over the offsets 0 1 1 2 64 65 129 300, signs alternating in threes, one off-curve point --
// with tiles of 8 and 16, against a sequential fold of the same additions.  Prints "point_sum ok" and returns 0.
#include <stdio.h>
#include "point_sum_emul.cpp"

int main() {
  const size_t n = 300, m = 7;
  const unsigned long long offsets[m + 1] = {0, 1, 1, 2, 64, 65, 129, 300};
  Aligned<uint8_t> pts(n * 64);
  std::vector<uint8_t> neg(n);
  const Ext base = ext_from_ref_affine(K.B8X, K.B8Y, K);
  Ext acc = base;
  for (size_t i = 0; i < n; i++) {
    psum_store_result(pts.p() + i * 64, acc, fr_inv(acc.Z), K);
    acc = msm_add(acc, base, K);
    neg[i] = (i / 3) % 2 ? (uint8_t)(1 + i % 200) : 0;
  }
  const size_t bad = 100;
  pts.p()[bad * 64] ^= 1;
  Aligned<uint8_t> want(m * 64);
  for (size_t s = 0; s < m; s++) {
    Ext sum = ext_identity();
    for (size_t i = offsets[s]; i < offsets[s + 1]; i++) {
      bool on = false;
      const PsumLane a = psum_load_point(pts.p(), neg.data(), i, (const u64*)offsets, m, &on, K);
      if (on != (i != bad) || a.seg != s) { printf("point %zu: on %d segment %u\n", i, (int)on, a.seg); return 1; }
      sum = msm_add(sum, a.v, K);
    }
    psum_store_result(want.p() + s * 64, sum, fr_inv(sum.Z), K);
  }
  memset(want.p() + 5 * 64, 0, 64);   // the segment of the off-curve point
  for (int T : {8, 16}) {
    for (int pass = 0; pass < 2; pass++) {   // with the signs, and without them against a fold that ignores them
      std::vector<uint8_t> out(m * 64);
      long long st[m];
      const int rc = point_sum_emul_run(pts.p(), pass ? nullptr : neg.data(), n, offsets, m, T, out.data(), st);
      if (rc) { printf("tile %d: harness returned %d\n", T, rc); return 1; }
      for (size_t s = 0; s < m; s++)
        if (st[s] != (s == 5 ? (long long)bad : -1)) { printf("tile %d: status[%zu] = %lld\n", T, s, st[s]); return 1; }
      if (pass == 0 && memcmp(out.data(), want.p(), m * 64) != 0) { printf("tile %d: results differ from the fold\n", T); return 1; }
      if (out[1 * 64 + 32] != 1) { printf("tile %d: the empty segment is not the identity\n", T); return 1; }
    }
  }
  const unsigned long long garbage[4] = {0, 1ull << 40, 3, 300};
  std::vector<uint8_t> out(3 * 64);
  long long st[3];
  if (point_sum_emul_run(pts.p(), neg.data(), n, garbage, 3, 8, out.data(), st) != 0 || st[0] != -2 || st[2] != -2) return 1;
  printf("point_sum ok\n");
  return 0;
}
