// Stand-alone driver of the harness beside it, for -fsanitize=address,undefined (tests/test_dleq_host.py): one mixed case over small
// tables -- B8 as a context holds it (W = 4) and 5 * B8 as a caller's generator (W = 5), with the keys 11 * G of both (W = 5, 4).
// Checked here without any oracle: a P + b P equals (a + b) P + 0 P while nothing wraps, adding the negated result gives the identity,
// a bad point refuses its own item only; every proof the prover's chain makes is accepted, with the prover's D equal to sk * C1 by
// the joint loop; a flipped bit of z, A or B, z = 2^256 - 1, another item's C1, another tag and the other generator's key table are
// rejected; an off-curve C1 is 2 on both sides.  Prints "dleq ok" and returns 0.
#include <stdio.h>
#include "dleq_emul.cpp"

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
  const size_t n = 10, off = 4;
  // ---- bjj_mul_pair ----
  std::vector<uint8_t> P(n * 64), a(n * 32), b(n * 32), ab(n * 32), zero(n * 32, 0);
  for (size_t i = 0; i < n; i++) {
    const std::vector<uint8_t> p = multiple_of_b8((u32)(3 * i + 1));
    memcpy(P.data() + i * 64, p.data(), 64);
    unsigned carry = 0;
    for (int k = 0; k < 32; k++) {
      const uint8_t x = k < 31 ? (uint8_t)(0xA5 ^ (i * 37 + k * 29)) : 0x01, y = k < 31 ? (uint8_t)(0x3C + i * 11 + k * 7) : 0x02;   // < 2^250: no reduction, no wrap
      a[i * 32 + k] = x; b[i * 32 + k] = y;
      const unsigned s = x + y + carry;
      ab[i * 32 + k] = (uint8_t)s; carry = s >> 8;
    }
  }
  std::vector<uint8_t> o1(n * 64), o2(n * 64), o3(n * 64), ok(n);
  CHECK(dq_emul_pair(P.data(), a.data(), P.data(), b.data(), nullptr, n, o1.data(), ok.data()) == 0, "pair call");
  for (size_t i = 0; i < n; i++) CHECK(ok[i] == 1, "pair ok[%zu] = %d", i, ok[i]);
  CHECK(dq_emul_pair(P.data(), ab.data(), P.data(), zero.data(), nullptr, n, o2.data(), ok.data()) == 0 && o1 == o2, "a P + b P differs from (a + b) P");
  const std::vector<uint8_t> minus = negated(o1);
  CHECK(dq_emul_pair(P.data(), a.data(), P.data(), b.data(), minus.data(), n, o3.data(), ok.data()) == 0, "negated addend");
  for (size_t i = 0; i < n; i++) {
    uint8_t id[64] = {0};
    id[32] = 1;
    CHECK(!memcmp(o3.data() + i * 64, id, 64) && ok[i] == 1, "item %zu: S - S is not the identity", i);
  }
  {
    std::vector<uint8_t> bad(P), add(o1);
    bad[off * 64] ^= 1;
    memset(add.data() + 7 * 64, 0, 64);
    CHECK(dq_emul_pair(P.data(), a.data(), P.data(), b.data(), o1.data(), n, o2.data(), ok.data()) == 0, "good points");
    CHECK(dq_emul_pair(P.data(), a.data(), bad.data(), b.data(), add.data(), n, o3.data(), ok.data()) == 0, "bad points");
    for (size_t i = 0; i < n; i++) {
      const bool refused = i == off || i == 7;
      uint8_t z[64] = {0};
      CHECK(ok[i] == (refused ? 2 : 1), "pair ok[%zu] = %d beside a bad point", i, ok[i]);
      CHECK(!memcmp(o3.data() + i * 64, refused ? z : o2.data() + i * 64, 64), "item %zu beside a bad point", i);
    }
  }
  // ---- prove and verify ----
  const int g_ctx = dq_emul_table(nullptr, 4);
  const int g_own = dq_emul_table(multiple_of_b8(5).data(), 5);
  const int pk_ctx = dq_emul_table(multiple_of_b8(11).data(), 5);
  const int pk_own = dq_emul_table(multiple_of_b8(55).data(), 4);
  CHECK(g_ctx >= 0 && g_own >= 0 && pk_ctx >= 0 && pk_own >= 0, "tables: %d %d %d %d", g_ctx, g_own, pk_ctx, pk_own);
  std::vector<uint8_t> sk(32, 0), tag(32, 0x5A);
  sk[0] = 11;
  const int gs[2] = {g_ctx, g_own}, pks[2] = {pk_ctx, pk_own};
  for (int s = 0; s < 2; s++) {
    std::vector<uint8_t> D(n * 64), A(n * 64), B(n * 64), z(n * 32), v(n), skD(n * 64), sks(n * 32, 0);
    std::vector<uint8_t> w(a);
    memset(w.data() + 2 * 32, 0, 32);                                   // w = 0: A = B = the identity
    memset(w.data() + 3 * 32, 0xFF, 32);                                // w = 2^256 - 1
    CHECK(dq_emul_prove(gs[s], sk.data(), tag.data(), P.data(), w.data(), n, D.data(), A.data(), B.data(), z.data(), ok.data()) == 0, "prove");
    for (size_t i = 0; i < n; i++) { CHECK(ok[i] == 1, "prove ok[%zu] = %d", i, ok[i]); sks[i * 32] = 11; }
    CHECK(dq_emul_pair(P.data(), sks.data(), P.data(), zero.data(), nullptr, n, skD.data(), v.data()) == 0 && skD == D, "the prover's D is not sk * C1");
    CHECK(dq_emul_verify(gs[s], pks[s], tag.data(), P.data(), D.data(), A.data(), B.data(), z.data(), n, v.data()) == 0, "verify");
    for (size_t i = 0; i < n; i++) CHECK(v[i] == 1, "set %d: proof %zu is not accepted (%d)", s, i, v[i]);
    CHECK(dq_emul_verify(gs[s], pks[1 - s], tag.data(), P.data(), D.data(), A.data(), B.data(), z.data(), n, v.data()) == 0, "verify, other key");
    for (size_t i = 0; i < n; i++) CHECK(v[i] == 0, "set %d: proof %zu passes against the other key's table", s, i);
    std::vector<uint8_t> tag2(tag);
    tag2[5] ^= 1;
    CHECK(dq_emul_verify(gs[s], pks[s], tag2.data(), P.data(), D.data(), A.data(), B.data(), z.data(), n, v.data()) == 0, "verify, other tag");
    for (size_t i = 0; i < n; i++) CHECK(v[i] == 0, "set %d: proof %zu passes under another tag", s, i);
    // one-field mutations, one per item
    std::vector<uint8_t> c1(P), d(D), aa(A), bb(B), zz(z);
    zz[0 * 32 + 9] ^= 4;                                                // a bit of z
    aa[1 * 64 + 3] ^= 1;                                                // a bit of A.x
    bb[2 * 64 + 40] ^= 2;                                               // a bit of B.y
    memcpy(c1.data() + 3 * 64, P.data() + 5 * 64, 64);                  // another item's C1
    c1[off * 64] ^= 1;                                                  // C1 off the curve
    memset(d.data() + 5 * 64, 0, 64);                                   // D = (0, 0)
    memset(zz.data() + 6 * 32, 0xFF, 32);                               // z = 2^256 - 1
    const uint8_t want[10] = {0, 0, 0, 0, 2, 2, 0, 1, 1, 1};
    CHECK(dq_emul_verify(gs[s], pks[s], tag.data(), c1.data(), d.data(), aa.data(), bb.data(), zz.data(), n, v.data()) == 0, "verify, mutated");
    for (size_t i = 0; i < n; i++) CHECK(v[i] == want[i], "set %d: mutated item %zu gives %d, not %d", s, i, v[i], want[i]);
    // the prover refuses an off-curve C1 alone, and zeroes its outputs
    std::vector<uint8_t> D2(n * 64), A2(n * 64), B2(n * 64), z2(n * 32);
    CHECK(dq_emul_prove(gs[s], sk.data(), tag.data(), c1.data(), w.data(), n, D2.data(), A2.data(), B2.data(), z2.data(), ok.data()) == 0, "prove, off-curve");
    for (size_t i = 0; i < n; i++) {
      uint8_t zr[64] = {0};
      CHECK(ok[i] == (i == off ? 2 : 1), "prove ok[%zu] = %d beside an off-curve C1", i, ok[i]);
      if (i == off) CHECK(!memcmp(D2.data() + i * 64, zr, 64) && !memcmp(A2.data() + i * 64, zr, 64) && !memcmp(B2.data() + i * 64, zr, 64) &&
                          !memcmp(z2.data() + i * 32, zr, 32), "the refused item's outputs are not zero");
      else if (i != 3) CHECK(!memcmp(D2.data() + i * 64, D.data() + i * 64, 64) && !memcmp(z2.data() + i * 32, z.data() + i * 32, 32), "item %zu beside an off-curve C1", i);
    }
  }
  dq_emul_free_tables();
  printf("dleq ok\n");
  return 0;
}
