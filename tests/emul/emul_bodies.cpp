// DEBUG HARNESS (tests only): executes the product's per-item kernel bodies
// (bjj_device.hpp) on the CPU with limb/value-bound assertions.  It exists to
// catch arithmetic-contract violations here, where there is no GPU; it is not a
// fallback and is not linked into libbjj_hip.so.
#define BJJ_DEBUG_BOUNDS 1
#include <string.h>
#include <stdlib.h>
#include <vector>
#include "../../babyjubjub-rs_amd/csrc/sign.hpp"
#include "../../babyjubjub-rs_amd/csrc/bjj_constants.inc"
#include "../devfuzz/scalar_ops.hpp"
using namespace bjj;
static const Consts K = BJJ_CONSTS_INIT;
static std::vector<u32> g_table, g_bases; static int g_W = 0, g_nwin = 0;
static u32* aligned16(std::vector<u32>& v) { return (u32*)(((uintptr_t)v.data() + 15) & ~(uintptr_t)15); }
// the table is built by the product's chain builder (what bjj_k_build_fixed_table runs per thread)
static void build_table(int W, u32 chain) {
  g_W = W; g_nwin = fixed_nwin(W);
  const size_t stride = fixed_stride(W), entries = stride * g_nwin;
  g_table.assign(entries * NIELS_WORDS + 4, 0);
  g_bases.assign((size_t)g_nwin * NIELS_WORDS + 4, 0);
  u32* t = aligned16(g_table); u32* bs = aligned16(g_bases);
  for (int j = 0; j < g_nwin; j++) store_niels(bs + (size_t)j * NIELS_WORDS, fixed_table_entry(1u, j, W, K));
  for (int j = 0; j < g_nwin; j++)
    for (size_t k0 = 0; k0 < stride; k0 += chain) {
      u32 cnt = (u32)(stride - k0 < chain ? stride - k0 : chain);
      fixed_table_chain(t, load_niels(bs + (size_t)j * NIELS_WORDS), (size_t)j * stride + k0, (u32)k0, cnt, W, K);
    }
}
static void ensure_table(int W) {
  if (g_W == W) return;
  build_table(W, 8);
}
static const u32* table_ptr() { return aligned16(g_table); }
static void ext_out(const Ext& p, uint8_t* out) {  // single-item affine epilogue
  alignas(16) u32 w[8];
  Fr zi = fr_inv(p.Z);
  Fr c1 = fr_mul(zi, fr_one_plain()), c2 = fr_mul(zi, K.FINV_PLAIN);
  constexpr u32 R1[NL] = {BJJ_N0, BJJ_N1, BJJ_N2, BJJ_N3, BJJ_N4, BJJ_N5, BJJ_N6, BJJ_N7, BJJ_N8};
  fr_to_words(fr_cond_sub_kr(fr_mul(p.X, c2), R1), w); memcpy(out, w, 32);
  fr_to_words(fr_cond_sub_kr(fr_mul(p.Y, c1), R1), w); memcpy(out + 32, w, 32);
}
extern "C" {
// the shift-register digit stream (DigitStream, what the kernels run) against the indexed definition (fixed_digit_slot):
// number of windows on which slot or sign differ, for one 32-byte scalar and one window width
int emul_digit_stream_mismatches(const uint8_t* scalar32, int W) {
  alignas(16) u32 sc[8];
  memcpy(sc, scalar32, 32);
  const int nwin = fixed_nwin(W);
  DigitStream ds = digit_stream(sc, W);
  u32 carry = 0;
  int bad = 0;
  for (int j = 0; j < nwin; j++) {
    bool n1, n2;
    const size_t a = digit_next(ds, n1), b = fixed_digit_slot(sc, j, W, carry, n2);
    bad += (a != b) || (n1 != n2);
  }
  return bad;
}
// builds the table with the chain builder, then (i) compares every entry with the independent per-entry ladder
// (fixed_table_entry) and (ii) runs the induction check the GPU runs; `corrupt` >= 0 flips one bit of that
// slot first so the test can see the check fire.  Returns mismatches in the high half, check failures in the low.
unsigned long long emul_table_selfcheck(int W, unsigned chain, long long corrupt_slot) {
  build_table(W, chain);
  g_W = 0;  // force a rebuild for later callers
  u32* t = aligned16(g_table); const u32* bs = aligned16(g_bases);
  const int nwin = fixed_nwin(W);
  const size_t stride = fixed_stride(W);
  unsigned long long mism = 0, bad = 0;
  for (int j = 0; j < nwin; j++)
    for (size_t k = 0; k < stride; k++)
      mism += !niels_limbs_equal(load_niels(t + ((size_t)j * stride + k) * NIELS_WORDS), fixed_table_entry((u32)k, j, W, K, j == 0));
  if (corrupt_slot >= 0) t[(size_t)corrupt_slot * NIELS_WORDS + 11] ^= 4u;
  for (int j = 0; j < nwin; j++)
    for (size_t k = 0; k < stride; k++) bad += fixed_table_check_slot(t, bs, j, (u32)k, W, nwin, K);
  return (mism << 32) | bad;
}
void emul_fixed_base(const uint8_t* scalar, int W, uint8_t* out) {
  ensure_table(W);
  alignas(16) u32 sc[8]; memcpy(sc, scalar, 32);
  ext_out(fixed_base_mul(table_ptr(), g_W, g_nwin, sc, K), out);
}
// the signer's constant-time option: the same multiplication through the scanning policy (every entry of a window is read)
void emul_fixed_base_scan(const uint8_t* scalar, int W, uint8_t* out) {
  ensure_table(W);
  alignas(16) u32 sc[8]; memcpy(sc, scalar, 32);
  ext_out(fixed_base_mul(GatherScan{table_ptr(), (u32)fixed_stride(g_W)}, g_W, g_nwin, sc, K), out);
}
// u * P1 + v * P2 through verify's joint double-and-add with EXACTLY nwin windows (P1, P2 on the curve; u, v < 2^(4 nwin - 1))
void emul_joint_mul(const uint8_t* p1, const uint8_t* p2, const uint8_t* u32b, const uint8_t* v32b, int nwin, uint8_t* out) {
  alignas(16) u32 w[8];
  Fr c[4];
  const uint8_t* src[4] = {p1, p1 + 32, p2, p2 + 32};
  for (int i = 0; i < 4; i++) { memcpy(w, src[i], 32); c[i] = fr_to_mont_words(w); }
  std::vector<u32> buf(2 * VB_TABLE_WORDS + 8);
  u32* tbl = aligned16(buf);
  vb_build_table(ext_from_ref_affine(c[0], c[1], K), tbl, K, true);
  vb_build_table(ext_from_ref_affine(c[2], c[3], K), tbl + VB_TABLE_WORDS, K, true);
  memcpy(w, u32b, 32); const Fr u = fr_from_words(w);
  memcpy(w, v32b, 32); const Fr v = fr_from_words(w);
  ext_out(joint_mul_windowed(tbl, tbl + VB_TABLE_WORDS, u, v, nwin, K), out);
}
void emul_var_base(const uint8_t* pt, const uint8_t* scalar, uint8_t* out) {
  alignas(16) u32 w[8], sc[8]; alignas(16) static u32 tbl[VB_TABLE_WORDS];
  memcpy(w, pt, 32); Fr x = fr_to_mont_words(w);
  memcpy(w, pt + 32, 32); Fr y = fr_to_mont_words(w);
  memcpy(sc, scalar, 32);
  ext_out(var_base_item(x, y, sc, tbl, K), out);
}
void emul_poseidon5(const uint8_t* in, uint8_t* out) {
  Fr h[5]; alignas(16) u32 w[8];
  for (int j = 0; j < 5; j++) { memcpy(w, in + 32 * j, 32); h[j] = fr_to_mont_words(w); }
  fr_from_mont_words(poseidon5(h, K), w); memcpy(out, w, 32);
}
void emul_blake512(const uint8_t* msg, int nbytes, uint8_t* out) {  // nbytes in {32, 64}
  alignas(16) u32 w[16], d[16]; memcpy(w, msg, nbytes); blake512_words(w, nbytes / 4, d); memcpy(out, d, 64);
}
void emul_scalar_key(const uint8_t* key, uint8_t* out) {
  alignas(16) u32 k[8], sk[8], pr[8], hi[8]; memcpy(k, key, 32); scalar_key_words(k, sk, pr, hi); memcpy(out, sk, 32);
}
int emul_sign(const uint8_t* key, const uint8_t* msg, int W, uint8_t* out_r, uint8_t* out_s) {
  ensure_table(W);
  alignas(16) u32 k[8], m[8], rx[8], ry[8], s[8]; memcpy(k, key, 32); memcpy(m, msg, 32);
  bool ok = sign_item(k, m, table_ptr(), g_W, g_nwin, rx, ry, s, K);
  if (!ok) { memset(out_r, 0, 64); memset(out_s, 0, 32); return 0; }
  memcpy(out_r, rx, 32); memcpy(out_r + 32, ry, 32); memcpy(out_s, s, 32); return 1;
}
int emul_sign_schnorr(const uint8_t* key, const uint8_t* msg, const uint8_t* nonce, int W, uint8_t* out_r, uint8_t* out_s) {
  ensure_table(W);
  alignas(16) u32 k[8], m[8], kn[SCHNORR_K_WORDS], rx[8], ry[8], s[SCHNORR_S_WORDS];
  memcpy(k, key, 32); memcpy(m, msg, 32); memcpy(kn, nonce, SCHNORR_K_WORDS * 4);
  bool ok = sign_schnorr_item(k, m, kn, table_ptr(), g_W, g_nwin, rx, ry, s, K);
  if (!ok) { memset(out_r, 0, 64); memset(out_s, 0, SCHNORR_S_WORDS * 4); return 0; }
  memcpy(out_r, rx, 32); memcpy(out_r + 32, ry, 32); memcpy(out_s, s, SCHNORR_S_WORDS * 4); return 1;
}
int emul_verify_schnorr(const uint8_t* pk, const uint8_t* r, const uint8_t* s, const uint8_t* msg, int W) {
  ensure_table(W);
  alignas(16) uint8_t b[192]; alignas(16) static u32 tbl[VB_VERIFY_WORDS];
  memcpy(b, pk, 64); memcpy(b + 64, r, 64); memcpy(b + 128, s, 32); memcpy(b + 160, msg, 32);
  VerifyIn in = {b, b + 64, b + 128, b + 160};
  return verify_schnorr_item(in, table_ptr(), g_W, g_nwin, tbl, K);
}
// (u, |v|, sign) of lattice_short_pair for a canonical kappa < l given as 32 LE bytes
int emul_short_pair(const uint8_t* kappa, uint8_t* u_out, uint8_t* v_out) {
  alignas(16) u32 w[8]; memcpy(w, kappa, 32);
  Fr u, vm; bool neg;
  lattice_short_pair(fr_from_words(w), u, vm, neg, K);
  fr_to_words(u, w); memcpy(u_out, w, 32);
  fr_to_words(vm, w); memcpy(v_out, w, 32);
  return neg ? 1 : 0;
}
// the scalar-arithmetic ops of tests/devfuzz/scalar_ops.hpp, the body the device harness runs (records as in sc_run there)
int emul_scalar_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, int nw) {
  if (op < 0 || op >= SC_NOPS || (op == SC_WIDE && (nw < 1 || nw > 1024))) return -1;
  const size_t wa = sc_a_words(op, nw), wb = sc_b_words(op), wo = sc_out_words(op);
  for (size_t i = 0; i < n; i++) sc_item(op, a + i * wa, b + i * wb, out + i * wo, nw, K);
  return 0;
}
int emul_decompress(const uint8_t* in, uint8_t* out) {
  alignas(16) u32 w[8], ox[8], oy[8]; memcpy(w, in, 32);
  bool ok = decompress_item(w, ox, oy, K);
  memcpy(out, ox, 32); memcpy(out + 32, oy, 32);
  return ok ? 1 : 0;
}
void emul_compress(const uint8_t* in, uint8_t* out) {
  alignas(16) u32 x[8], y[8], o[8]; memcpy(x, in, 32); memcpy(y, in + 32, 32);
  compress_item(x, y, o, K); memcpy(out, o, 32);
}
int emul_verify(const uint8_t* pk, const uint8_t* r, const uint8_t* s, const uint8_t* msg, int W) {
  ensure_table(W);
  alignas(16) uint8_t b[192]; alignas(16) static u32 tbl[VB_VERIFY_WORDS];
  memcpy(b, pk, 64); memcpy(b + 64, r, 64); memcpy(b + 128, s, 32); memcpy(b + 160, msg, 32);
  VerifyIn in = {b, b + 64, b + 128, b + 160};
  return verify_item(in, table_ptr(), g_W, g_nwin, tbl, K) ? 1 : 0;
}
}
