// Stand-alone driver of the harness beside it, for -fsanitize=address,undefined (tests/test_elgamal_host.py): one mixed case over
// small tables -- B8 as a context holds it (W = 4), 5 * B8 + nothing else as a caller's generator (W = 5) and two keys (W = 4, 5) --
// with the edge values of m, full-width values of r, and add arrays that hold an off-curve record and (0, 0).  Checked here without
// any oracle: the ciphertexts are homomorphic byte for byte (Enc(m, r) + Enc(m', r') = Enc(m + m', r + r') while nothing wraps),
// adding the negated result gives the identity, m == NULL equals m = 0, a call in place equals the call out of place, and a bad
// addend refuses its own item only.  Prints "elgamal ok" and returns 0.
#include <stdio.h>
#include "elgamal_emul.cpp"

static std::vector<uint8_t> negated(const std::vector<uint8_t>& pts) {   // (x, y) -> (r - x, y); x == 0 stays
  std::vector<uint8_t> out(pts);
  for (size_t i = 0; i < pts.size() / 64; i++) {
    alignas(16) u32 w[8];
    memcpy(w, pts.data() + i * 64, 32);
    const Fr x = fr_to_mont_words(w);
    fr_from_mont_words(fr_canon(fr_neg(x)), w);
    memcpy(out.data() + i * 64, w, 32);
  }
  return out;
}
static std::vector<uint8_t> multiple_of_b8(u32 k) {
  Ext acc = ext_identity();
  const PNiels bn = ext_to_pniels(ext_from_ref_affine(K.B8X, K.B8Y, K), K);
  for (u32 i = 0; i < k; i++) acc = ext_add_pn(acc, bn);
  std::vector<uint8_t> out(64);
  store_affine(out.data(), acc);
  return out;
}
#define CHECK(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

int main() {
  const int g_ctx = eg_emul_table(nullptr, 4);
  const int g_own = eg_emul_table(multiple_of_b8(5).data(), 5);
  const int pk4 = eg_emul_table(multiple_of_b8(11).data(), 4);
  const int pk5 = eg_emul_table(multiple_of_b8(3).data(), 5);
  CHECK(g_ctx >= 0 && g_own >= 0 && pk4 >= 0 && pk5 >= 0, "tables: %d %d %d %d", g_ctx, g_own, pk4, pk5);
  const size_t n = 12, off = 5, zero = 9;
  std::vector<uint64_t> m(n), m2(n), msum(n);
  std::vector<uint8_t> r(n * 32), r2(n * 32), rsum(n * 32);
  const uint64_t edges[] = {0, 1, 8, 9, 16, 17, 1ull << 63, ~0ull, 0x8888888888888888ull, 0x9999999999999999ull, 0x4210842108421084ull, 0x5294a5294a5294a5ull};
  for (size_t i = 0; i < n; i++) {
    m[i] = edges[i] >> 1; m2[i] = edges[n - 1 - i] >> 1; msum[i] = m[i] + m2[i];   // halves: the sum stays below 2^64
    unsigned carry = 0;
    for (int b = 0; b < 32; b++) {
      const uint8_t x = b < 31 ? (uint8_t)(0xA5 ^ (i * 37 + b * 29)) : 0x01, y = b < 31 ? (uint8_t)(0x3C + i * 11 + b * 7) : 0x02;   // < 2^250: no reduction, no wrap
      r[i * 32 + b] = x; r2[i * 32 + b] = y;
      const unsigned s = x + y + carry;
      rsum[i * 32 + b] = (uint8_t)s; carry = s >> 8;
    }
  }
  const int gs[2] = {g_ctx, g_own}, pks[2] = {pk4, pk5};
  for (int gi = 0; gi < 2; gi++) {
    for (int pi = 0; pi < 2; pi++) {
      const int g = gs[gi], pk = pks[pi];
      std::vector<uint8_t> a1(n * 64), a2(n * 64), b1(n * 64), b2(n * 64), s1(n * 64), s2(n * 64), ok(n), id1(n * 64), id2(n * 64);
      CHECK(eg_emul_encrypt(g, pk, m.data(), r.data(), nullptr, nullptr, n, 0, a1.data(), a2.data(), ok.data()) == 0, "plain call");
      for (size_t i = 0; i < n; i++) CHECK(ok[i] == 1, "ok[%zu] = %d without add arrays", i, ok[i]);
      CHECK(eg_emul_encrypt(g, pk, m.data(), r.data(), nullptr, nullptr, n, 0, b1.data(), b2.data(), nullptr) == 0 && a1 == b1 && a2 == b2, "ok == NULL");
      // homomorphic: Enc(m2, r2) added to Enc(m, r) is Enc(m + m2, r + r2)
      CHECK(eg_emul_encrypt(g, pk, m2.data(), r2.data(), a1.data(), a2.data(), n, 0, b1.data(), b2.data(), ok.data()) == 0, "add call");
      CHECK(eg_emul_encrypt(g, pk, msum.data(), rsum.data(), nullptr, nullptr, n, 0, s1.data(), s2.data(), nullptr) == 0, "sum call");
      CHECK(b1 == s1 && b2 == s2, "Enc(m, r) + Enc(m', r') differs from Enc(m + m', r + r') (g %d, pk %d)", gi, pi);
      // in place equals out of place
      CHECK(eg_emul_encrypt(g, pk, m2.data(), r2.data(), a1.data(), a2.data(), n, 1, s1.data(), s2.data(), ok.data()) == 0 && b1 == s1 && b2 == s2, "in place");
      // the negated result as the addend: the identity, twice
      const std::vector<uint8_t> n1 = negated(a1), n2 = negated(a2);
      CHECK(eg_emul_encrypt(g, pk, m.data(), r.data(), n1.data(), n2.data(), n, 0, id1.data(), id2.data(), ok.data()) == 0, "negated call");
      for (size_t i = 0; i < n; i++) {
        uint8_t id[64] = {0};
        id[32] = 1;
        CHECK(!memcmp(id1.data() + i * 64, id, 64) && !memcmp(id2.data() + i * 64, id, 64) && ok[i] == 1, "item %zu: C - C is not the identity", i);
      }
      // m == NULL is m = 0; with add arrays: re-randomisation
      std::vector<uint64_t> zeros(n, 0);
      CHECK(eg_emul_encrypt(g, pk, nullptr, r2.data(), a1.data(), a2.data(), n, 0, b1.data(), b2.data(), ok.data()) == 0, "re-randomise");
      CHECK(eg_emul_encrypt(g, pk, zeros.data(), r2.data(), a1.data(), a2.data(), n, 0, s1.data(), s2.data(), ok.data()) == 0 && b1 == s1 && b2 == s2, "m == NULL");
      CHECK(b1 != a1 && b2 != a2, "re-randomisation left the ciphertexts as they were");
      // a bad addend refuses its own item only
      std::vector<uint8_t> x1(a1), x2(a2), c1(n * 64), c2(n * 64);
      x1[off * 64] ^= 1;
      memset(x2.data() + zero * 64, 0, 64);
      CHECK(eg_emul_encrypt(g, pk, nullptr, r2.data(), x1.data(), x2.data(), n, 0, c1.data(), c2.data(), ok.data()) == 0, "bad addends");
      for (size_t i = 0; i < n; i++) {
        const bool bad = i == off || i == zero;
        uint8_t z[64] = {0};
        CHECK(ok[i] == (bad ? 2 : 1), "ok[%zu] = %d", i, ok[i]);
        CHECK(!memcmp(c1.data() + i * 64, bad ? z : b1.data() + i * 64, 64) && !memcmp(c2.data() + i * 64, bad ? z : b2.data() + i * 64, 64), "item %zu beside a bad addend", i);
      }
    }
  }
  eg_emul_free_tables();
  printf("elgamal ok\n");
  return 0;
}
