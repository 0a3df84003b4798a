// Stand-alone driver of the harness beside it, for -fsanitize=address,undefined (tests/test_common_scalar_host.py): one mixed case --
// 40 multiples of B8 with an off-curve record and (0, 0) among them, addends of the same kind, a full-width and a short scalar, both
// signs, both forms -- where the two forms must agree byte for byte, k * P - k * P must be the identity, and the multiples of B8 must
// pass the subgroup check.  Prints "common_scalar ok" and returns 0.
#include <stdio.h>
#include "common_scalar_emul.cpp"

int main() {
  const size_t n = 40, bad = 17, zero = 29;
  std::vector<uint8_t> pts(n * 64), add(n * 64);
  const Ext base = ext_from_ref_affine(K.B8X, K.B8Y, K);
  const PNiels bn = ext_to_pniels(base, K);
  Ext acc = base;
  for (size_t i = 0; i < n; i++) {
    store_affine(pts.data() + i * 64, acc);
    acc = ext_add_pn(acc, bn);
    store_affine(add.data() + (n - 1 - i) * 64, acc);
  }
  pts[bad * 64] ^= 1;
  memset(pts.data() + zero * 64, 0, 64);
  add[3 * 64 + 32] ^= 2;
  uint8_t scalars[2][32];
  for (int i = 0; i < 32; i++) { scalars[0][i] = (uint8_t)(0xA5 ^ (i * 29)); scalars[1][i] = i < 8 ? (uint8_t)(0x3C + i) : 0; }
  for (const auto& k : scalars) {
    for (int sub = 0; sub < 2; sub++) {
      for (int with_add = 0; with_add < 2; with_add++) {
        std::vector<uint8_t> out[2] = {std::vector<uint8_t>(n * 64), std::vector<uint8_t>(n * 64)}, ok[2] = {std::vector<uint8_t>(n), std::vector<uint8_t>(n)};
        for (int form = 0; form < 2; form++) {
          const int rc = cs_emul_mul(k, pts.data(), with_add ? add.data() : nullptr, sub, n, form, out[form].data(), ok[form].data());
          if (rc) { printf("form %d: harness returned %d\n", form, rc); return 1; }
        }
        if (out[0] != out[1] || ok[0] != ok[1]) { printf("the two forms disagree (sub %d, add %d)\n", sub, with_add); return 1; }
        for (size_t i = 0; i < n; i++) {
          const bool off = i == bad || i == zero || (with_add && i == 3);
          if (ok[0][i] != (off ? 2 : 1)) { printf("ok[%zu] = %d\n", i, ok[0][i]); return 1; }
        }
        if (!with_add) {   // k * P - k * P: the product as the addend of the opposite sign
          std::vector<uint8_t> back(n * 64), okb(n);
          if (cs_emul_mul(k, pts.data(), out[0].data(), !sub, n, 1, back.data(), okb.data())) return 1;
          for (size_t i = 0; i < n; i++) {
            if (i == bad || i == zero) continue;
            uint8_t id[64] = {0};
            id[32] = 1;
            if (memcmp(back.data() + i * 64, id, 64) != 0) { printf("item %zu: k P - k P is not the identity\n", i); return 1; }
          }
        }
      }
    }
  }
  for (int form = 0; form < 2; form++) {
    std::vector<uint8_t> ok(n);
    if (cs_emul_subgroup(pts.data(), n, form, ok.data())) return 1;
    for (size_t i = 0; i < n; i++)
      if (ok[i] != ((i == bad || i == zero) ? 2 : 1)) { printf("subgroup[%zu] = %d\n", i, ok[i]); return 1; }
  }
  printf("common_scalar ok\n");
  return 0;
}
