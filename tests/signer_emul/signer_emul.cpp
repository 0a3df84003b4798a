// DEBUG HARNESS (tests only): the per-item body and the verdict step of bjj_k_verify_signer (csrc/signer.hpp, what k_signer.hip
// launches) on the CPU with limb / value-bound assertions -- a stand-alone program, so that it also runs under AddressSanitizer
// and UndefinedBehaviorSanitizer as it is (tests/test_signer_host.py builds it twice).  Not linked into libbjj_hip.so.
//
// stdin:  "P <x> <y>"                the signer's point (hex, on the curve)
//         "I <count>" and <count> lines "<rx> <ry> <s> <msg>" (hex, any 256-bit values): the items
//         "Z <count>" and <count> non-zero field elements: the projective scalings of the verdict cases
//         "V <count>" and <count> lines "<lx> <ly> <tx> <ty> <rx> <ry>": curve points l, t (reference curve, affine) and any R
// Tables: the signer's at W = 4 and W = 5 (mod 8l, base_nwin windows), B8 at W = 4 as a CONTEXT's table (mod l, fixed_nwin windows).
// stdout: "check <table> <bad>"      the induction check of the three tables (0 expected)
//         "e <W> <i> <verdict>"      EdDSA verdict of item i over the signer's table of width W
//         "s <W> <i> <verdict>"      Schnorr verdict
//         "v <i> <k> <verdict>"      signer_verdict of case i with T scaled by Z[k] and L by Z[(k + 1) % count]; k = count: unscaled
#define BJJ_DEBUG_BOUNDS 1
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../babyjubjub-rs_amd/csrc/signer.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
#include "../emul_support.hpp"

// (x, y) affine on the reference curve -> the internal curve's projective form scaled by z: what a table chain hands to the verdict
static Ext scaled(const Words& x, const Words& y, const Fr* z) {
  Ext e = ext_from_ref_affine(fr_to_mont_words(x.w), fr_to_mont_words(y.w), K);
  e.T = fr_zero();
  if (z) { e.X = fr_mul(e.X, *z); e.Y = fr_mul(e.Y, *z); e.Z = *z; }
  return e;
}

int main() {
  Words pxy[2];
  if (!read_tag("P") || !read_words(pxy, 2)) { fprintf(stderr, "bad P line\n"); return 2; }
  size_t ni = 0, nz = 0, nv = 0;
  if (!read_header("I", ni)) { fprintf(stderr, "bad I line\n"); return 2; }
  std::vector<Words> items(4 * ni + 1);
  if (!read_words(items.data(), 4 * ni)) { fprintf(stderr, "bad item\n"); return 2; }
  if (!read_header("Z", nz) || nz == 0) { fprintf(stderr, "bad Z line\n"); return 2; }
  std::vector<Words> zs(nz);
  if (!read_words(zs.data(), nz)) { fprintf(stderr, "bad scaling\n"); return 2; }
  if (!read_header("V", nv)) { fprintf(stderr, "bad V line\n"); return 2; }
  std::vector<Words> vc(6 * nv + 1);
  if (!read_words(vc.data(), 6 * nv)) { fprintf(stderr, "bad verdict case\n"); return 2; }

  u32 xy[16];
  memcpy(xy, pxy[0].w, 32); memcpy(xy + 8, pxy[1].w, 32);
  const SignerPoint pk = signer_point(xy);
  if (!ref_on_curve(pk.x, pk.y, K)) { fprintf(stderr, "P is not on the curve\n"); return 2; }
  HostTable T[3];
  T[0].build(pk.x, pk.y, 4, false, 3);
  T[1].build(pk.x, pk.y, 5, false, 8);
  T[2].build(K.B8X, K.B8Y, 4, true, 8);
  for (int i = 0; i < 3; i++) printf("check %d %llu\n", i, T[i].check());

  for (int t = 0; t < 2; t++) {
    SignerArgs A;
    A.T = T[t].desc(); A.L = T[2].desc(); A.pk = pk;
    for (size_t i = 0; i < ni; i++) {
      const Words* it = &items[4 * i];   // rx, ry are read as ONE 64-byte record
      alignas(16) u32 r[16];
      memcpy(r, it[0].w, 32); memcpy(r + 8, it[1].w, 32);
      printf("e %d %zu %d\n", T[t].W, i, verify_signer_item<false>(A, GatherPerLane{A.T.table}, r, it[2].w, it[3].w, K));
      printf("s %d %zu %d\n", T[t].W, i, verify_signer_item<true>(A, GatherPerLane{A.T.table}, r, it[2].w, it[3].w, K));
    }
  }

  std::vector<Fr> z(nz);
  for (size_t k = 0; k < nz; k++) z[k] = fr_to_mont_words(zs[k].w);
  for (size_t i = 0; i < nv; i++) {
    const Words* c = &vc[6 * i];
    const Fr rx = fr_to_mont_words(c[4].w), ry = fr_to_mont_words(c[5].w);
    for (size_t k = 0; k <= nz; k++) {
      const Ext L = scaled(c[0], c[1], k < nz ? &z[(k + 1) % nz] : nullptr);
      const Ext Tp = scaled(c[2], c[3], k < nz ? &z[k] : nullptr);
      printf("v %zu %zu %d\n", i, k, signer_verdict(L, Tp, rx, ry, K));
    }
  }
  return 0;
}
