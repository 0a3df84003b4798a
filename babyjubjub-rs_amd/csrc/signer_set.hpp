// Verification against a SET of signers' fixed-base tables, by per-item index (include/bjj_hip_signer_set.h): the per-item body of
// bjj_k_*_verify_set and the per-thread bodies of the set's build and check kernels.  __host__ __device__ like signer.hpp, so that
// tests/signer_set_emul runs exactly this code on the CPU.
//
// Layout: the tables of all k signers lie in ONE allocation, signer j at entry offset j * E with E = nwin * (2^(W-1) + 1), each in
// the format of a bjj_base table (bases.hpp: base_nwin(W) windows, scalar mod 8l, window 0 of EVERY signer in T form).  The table
// pointer a wave gathers through stays wave-uniform -- the base of the allocation, in the kernel arguments -- and a lane adds
// idx * E to every slot number of its signer chain (GatherSlotOffset).  Slot numbers travel between the lanes as 32-bit words
// (GatherCoopLds::issue), hence k * E <= 2^32 (set_slots_fit); the byte address is formed in 64 bits from the slot.
// Beside the tables: the k keys as the hash takes them (Montgomery form, converted once at create time), SET_KEY_WORDS words each.
#pragma once
#include "signer.hpp"

#define BJJ_SET_BAD_SIGNER 3   // BJJ_VERIFY_BAD_SIGNER of include/bjj_hip_signer_set.h

namespace bjj {

constexpr int SET_KEY_WORDS = 20;   // x (9 limbs), y (9 limbs), 2 words of padding: five 16-byte loads per item

// entries per signer, and the limit the 32-bit slot words set on a set of k signers
BJJ_HD u64 set_entries_per_signer(int W) { return (u64)base_nwin(W) * (u64)fixed_stride(W); }
BJJ_HD bool set_slots_fit(u64 k, int W) { return k >= 1 && k <= ((u64)1 << 32) / set_entries_per_signer(W); }

// What bjj_k_*_verify_set knows of a call besides the item arrays; travels in the kernel arguments.  T: the descriptor of signer
// 0's table = the base of the allocation, L: the context's B8 table, keys: k records of SET_KEY_WORDS words, eps: entries per signer.
struct SetArgs { BaseDesc T, L; const u32* keys; u32 k, eps; };

BJJ_HD void set_key_store(u32* rec, const SignerPoint& p) {
  for (int i = 0; i < NL; i++) { rec[i] = p.x.v[i]; rec[NL + i] = p.y.v[i]; }
  rec[2 * NL] = 0; rec[2 * NL + 1] = 0;
}
BJJ_HD SignerPoint set_key_load(const u32* rec) {
  const U4* q = (const U4*)rec;
  const U4 a = q[0], b = q[1], c = q[2], d = q[3], e = q[4];
  SignerPoint p;
  p.x = Fr{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x}};
  p.y = Fr{{c.y, c.z, c.w, d.x, d.y, d.z, d.w, e.x, e.y}};
  return p;
}

// A gather policy (bjj_device.hpp "gather policies") that is Inner with a per-lane offset added to every slot: the table pointer,
// the staging areas and the cross-lane exchange are Inner's, so the wave still gathers through ONE pointer.
template <class Inner>
struct GatherSlotOffset : Inner {
  size_t off;
  BJJ_HD void issue(size_t slot, typename Inner::Pending& p, int buf) const { Inner::issue(slot + off, p, buf); }
};
template <class Inner>
BJJ_HD GatherSlotOffset<Inner> gather_slot_offset(const Inner& g, size_t off) {
  GatherSlotOffset<Inner> r{g, off};
  return r;
}

// ---- build and check: three launches for the whole set, whatever k ---------------------------------------------------------
// Thread t of the window-bases launch: P_{s,j} = 2^(W j) * key_s for (s, j) = (t / nwin, t % nwin), into bases[s * nwin + j].
BJJ_HD void set_window_base(u32* bases, const u32* keys, u64 t, int W, int nwin, const Consts& K) {
  const u64 s = t / (u64)nwin;
  const int j = (int)(t % (u64)nwin);
  const SignerPoint p = set_key_load(keys + s * SET_KEY_WORDS);
  store_niels(bases + t * NIELS_WORDS, base_table_entry(p.x, p.y, 1u, j, W, K));
}
// Thread t of the fill launch: chain c of window j of signer s, t = (s * nwin + j) * cpw + c.  fixed_table_chain decides T form by
// "slot0 lies in window 0", so it is handed the signer's OWN table and a slot number inside it: window 0 of every signer comes out
// in T form, which is what table_chains (bases.hpp) assumes of a chain's first entry.
BJJ_HD void set_fill_chain(u32* table, const u32* bases, u64 t, int W, int nwin, u32 chain, const Consts& K) {
  const u64 stride = fixed_stride(W), cpw = (stride + chain - 1) / chain;
  const u64 sj = t / cpw, k0 = (t % cpw) * chain;
  const u64 s = sj / (u64)nwin, j = sj % (u64)nwin;
  const u32 cnt = (u32)(stride - k0 < chain ? stride - k0 : chain);
  fixed_table_chain(table + s * (u64)nwin * stride * NIELS_WORDS, load_niels(bases + sj * NIELS_WORDS), (size_t)(j * stride + k0), (u32)k0,
                    cnt, W, K);
}
// Entry e of the whole set (e < k * E): base_table_check_slot on the signer's own table, anchored at the signer's own key.
BJJ_HD int set_check_entry(const u32* table, const u32* bases, const u32* keys, u64 e, int W, int nwin, const Consts& K) {
  const u64 stride = fixed_stride(W), eps = (u64)nwin * stride;
  const u64 s = e / eps, r = e % eps;
  const SignerPoint p = set_key_load(keys + s * SET_KEY_WORDS);
  return base_table_check_slot(table + s * eps * NIELS_WORDS, bases + s * (u64)nwin * NIELS_WORDS, (int)(r / stride), (u32)(r % stride), W,
                               nwin, p.x, p.y, K);
}

// ---- one item ---------------------------------------------------------------------------------------------------------------
// signer_item_verdict (signer.hpp) with the key and the table chosen by the item's index: verdict 0 / 1 (EdDSA), 0 / 1 / 2 (SCHNORR),
// or BJJ_SET_BAD_SIGNER for an index >= k.  Such an item runs the arithmetic on signer 0 -- the cooperative gather needs every lane
// of the wave, and nothing outside the set is read -- and its result is overridden at the end, before the msg > Q override is
// looked at.  The signer chain gathers through g with the lane's slot offset idx * eps (< 2^32: set_slots_fit), the B8 chain
// through g as it is.
template <bool SCHNORR, class G>
BJJ_HD int verify_set_item(const SetArgs& A, const G& g, u32 idx, const void* r, const void* s, const void* msg, const Consts& K) {
  const bool bad_idx = idx >= A.k;
  const u32 j = bad_idx ? 0u : idx;
  const int verdict = signer_item_verdict<SCHNORR>(A.T, A.L, set_key_load(A.keys + (size_t)j * SET_KEY_WORDS),
                                                   gather_slot_offset(g, (size_t)j * A.eps), g, r, s, msg, K);
  return bad_idx ? BJJ_SET_BAD_SIGNER : verdict;
}

}  // namespace bjj
