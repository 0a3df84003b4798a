// DEBUG HARNESS support (tests only): what the CPU harnesses under tests/*_emul and the stand-alone programs of tests/emul share.
// Header-only.  Include it AFTER the csrc header under test and bjj_constants.inc (and after BJJ_DEBUG_BOUNDS / BJJ_PNIELS_LAYOUT
// are defined); it brings namespace bjj in.  The sources tests/conftest.py builds itself (tests/emul/emul_bodies.cpp) do NOT
// include it: conftest's rebuild rule watches a fixed list of files, and this one is not on it.
//   K                          the constants, from the one initialiser beside struct Consts
//   Words, parse_hex, print_hex, read_words, read_header, read_tag      the stdin / stdout conventions of the stand-alone programs
//   Aligned<T>                 16-byte aligned storage
//   store_affine               a point as the 64-byte record the point-valued entries write
//   HostTable                  a fixed-base table in host memory, built and checked by the shipped bodies of csrc/bases.hpp
//   GatherBounded<N>           GatherPerLane that knows the extent of the N tables an item may read
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../babyjubjub-rs_amd/csrc/bases.hpp"
using namespace bjj;
static const Consts K = BJJ_CONSTS_INIT;

// ---- stdin: whitespace-separated tokens; a value is up to 64 hex digits, most significant first ------------------------------------
struct Words { alignas(16) u32 w[8]; };
static inline bool parse_hex(const char* s, Words& out) {
  const size_t len = strlen(s);
  if (len == 0 || len > 64) return false;
  memset(out.w, 0, sizeof(out.w));
  for (size_t i = 0; i < len; i++) {
    const char c = s[len - 1 - i];
    const int v = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
    if (v < 0) return false;
    out.w[i / 8] |= (u32)v << (4 * (i % 8));
  }
  return true;
}
static inline void print_hex(const u32 w[8]) {   // all 64 digits
  for (int i = 7; i >= 0; i--) printf("%08x", w[i]);
}
static inline bool read_words(Words* out, size_t count) {
  char tok[80];
  for (size_t i = 0; i < count; i++)
    if (scanf("%79s", tok) != 1 || !parse_hex(tok, out[i])) return false;
  return true;
}
static inline bool read_tag(const char* name) {   // "<name>", e.g. the "P" of a "P <x> <y>" line
  char tok[80];
  return scanf("%79s", tok) == 1 && !strcmp(tok, name);
}
static inline bool read_header(const char* name, size_t& count) {   // "<name> <count>"
  return read_tag(name) && scanf("%zu", &count) == 1 && count <= 100000;
}

// ---- memory ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
struct Aligned {   // 16-byte aligned storage (load_w8 / store_w8 / load_niels move 16-byte quarters)
  std::vector<T> v;
  Aligned() {}
  explicit Aligned(size_t n, T fill = T()) : v(n + 16 / sizeof(T) + 1, fill) {}
  T* p() { return (T*)(((uintptr_t)v.data() + 15) & ~(uintptr_t)15); }
};
static inline void store_affine(uint8_t* out, const Ext& p) {   // the plain affine epilogue: fr_inv per point
  u32 w[8];
  const Fr zi = fr_inv(p.Z);
  fr_from_mont_words(fr_mul(fr_mul(p.X, zi), K.FINV), w); memcpy(out, w, 32);
  fr_from_mont_words(fr_mul(p.Y, zi), w);                 memcpy(out + 32, w, 32);
}

// ---- a fixed-base table in host memory ------------------------------------------------------------------------------------------------
// The window bases by base_table_entry, the entries between them by fixed_table_chain in pieces of `chain` slots (what one thread
// of the build kernel fills), the induction check by base_table_check_slot: thread by thread what bjj_base_create launches.
struct HostTable {
  int W = 0, nwin = 0;
  bool ctx_b8 = false;   // the context's B8 table: fixed_nwin windows, scalars mod l; otherwise a caller's: base_nwin windows, mod 8l
  Fr bx, by;
  Aligned<u32> tv, bv;
  u32* t() { return tv.p(); }
  size_t slots() const { return fixed_stride(W) * (size_t)nwin; }
  void build(const Fr& x, const Fr& y, int W_, bool ctx_b8_, u32 chain) {
    W = W_; ctx_b8 = ctx_b8_; bx = x; by = y;
    nwin = ctx_b8 ? fixed_nwin(W) : base_nwin(W);
    const size_t stride = fixed_stride(W);
    tv = Aligned<u32>(slots() * NIELS_WORDS);
    bv = Aligned<u32>((size_t)nwin * NIELS_WORDS);
    for (int j = 0; j < nwin; j++) store_niels(bv.p() + (size_t)j * NIELS_WORDS, base_table_entry(bx, by, 1u, j, W, K));
    for (int j = 0; j < nwin; j++)
      for (size_t k0 = 0; k0 < stride; k0 += chain) {
        const u32 cnt = (u32)(stride - k0 < chain ? stride - k0 : chain);
        fixed_table_chain(t(), load_niels(bv.p() + (size_t)j * NIELS_WORDS), (size_t)j * stride + k0, (u32)k0, cnt, W, K);
      }
  }
  // failed slots of the induction check anchored at (ax, ay); the table's own point: 0 expected
  unsigned long long check(const Fr& ax, const Fr& ay) {
    unsigned long long bad = 0;
    for (int j = 0; j < nwin; j++)
      for (size_t k = 0; k < fixed_stride(W); k++) bad += (unsigned long long)base_table_check_slot(t(), bv.p(), j, (u32)k, W, nwin, ax, ay, K);
    return bad;
  }
  unsigned long long check() { return check(bx, by); }
  // every step-th stored entry against the independent per-entry ladder base_table_entry: the number that differ
  unsigned long long entry_mismatches(size_t step) {
    unsigned long long mism = 0;
    const size_t stride = fixed_stride(W);
    for (size_t s = 0; s < slots(); s += step) {
      const int j = (int)(s / stride);
      mism += !niels_limbs_equal(load_niels(t() + s * NIELS_WORDS), base_table_entry(bx, by, (u32)(s % stride), j, W, K, j == 0));
    }
    return mism;
  }
  BaseDesc desc() {
    BaseDesc d;
    memset(&d, 0, sizeof(d));
    d.table = t(); d.W = W; d.nwin = nwin; d.mod_l = ctx_b8 ? 1 : 0;
    return d;
  }
};

// GatherPerLane that knows the extent of the N tables an item reads: a slot past the end of the table in use ends the program
template <int N>
struct GatherBounded {
  struct Pending { Niels e; };
  struct Extent { const u32* table; size_t slots; };
  static constexpr int kBuffers = 2;
  const u32* table;
  Extent ext[N];
  static int wave_max(int v) { return v; }
  void issue(size_t slot, Pending& p, int) const {
    size_t limit = 0;
    for (int i = N - 1; i >= 0; i--)
      if (table == ext[i].table) limit = ext[i].slots;
    if (slot >= limit) { fprintf(stderr, "gather out of bounds: slot %zu of %zu\n", slot, limit); abort(); }
    p.e = load_niels(table + slot * NIELS_WORDS);
  }
  Niels finish(Pending& p, int) const { return p.e; }
};
