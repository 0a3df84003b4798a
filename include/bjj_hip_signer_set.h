/* bjj_hip_signer_set.h -- signature verification against a SET of signers' fixed-base tables, chosen per item by an index
 * (extension of bjj_hip_signer.h, same library).
 *
 * bjj_eddsa_verify_signer serves one key per call.  A rollup operator, an oracle feed with N reporters or an attestation service
 * with several issuers has a known set of keys -- a handful to tens of thousands -- and batches that mix their signatures in
 * arrival order.  A signer set holds the tables of all k keys in ONE device allocation; item i names its key by signer_idx[i], and
 * the batch is verified in one launch from table gathers alone, without sorting it by key.
 *
 * bjj_signer_set_create   synchronous.  pks_xy: k 64-byte records (x, y) on the HOST; coordinates >= r are reduced mod r.
 *     Duplicates, the identity and points of small order are valid keys.  window_bits: 0 (= 8) or 4..16, anything else is
 *     BJJ_E_INVALID (a wider table per key is what bjj_base_create is for).  n_windows = ceil(255 / window_bits); a signer's table
 *     has the entry format of a bjj_base table and takes n_windows * (2^(window_bits-1) + 1) * 128 bytes: 528 KB at 8 bits, so
 *     4 096 signers take 2.2 GB and 65 536 take 34.6 GB.  k >= 1 and k * n_windows * (2^(window_bits-1) + 1) <= 2^32, otherwise
 *     BJJ_E_INVALID -- checked before any point is looked at and before anything is allocated.  A key that is not on the curve:
 *     BJJ_E_INVALID, *out is not written, and *out_first_off_curve (when not NULL) receives the smallest such index; it receives -1
 *     on success.  BJJ_E_NOMEM when the device refuses the allocation.  Every table has passed its induction check, anchored at its
 *     own key, when the call returns.  The context owns the set: bjj_signer_set_free waits for the context's enqueued work and
 *     releases it (NULL set: BJJ_OK), bjj_free releases what is left.  The keys of a set are fixed.
 * bjj_signer_set_info     any out pointer may be NULL.  table_bytes = k * n_windows * (2^(window_bits-1) + 1) * 128.
 * bjj_signer_set_check    *n_bad = the number of violated conditions of the induction check over all k tables (0 = sound).
 *
 * bjj_eddsa_verify_set / bjj_schnorr_verify_set   ok[i] is byte for byte what bjj_eddsa_verify / bjj_schnorr_verify writes for
 *     pk = pks[signer_idx[i]] -- the key that is hashed is its record reduced mod r -- for every input those accept: any 256-bit s
 *     (unreduced); msg > Q gives 0 (EdDSA) or 2 (Schnorr), msg == Q wraps to 0; R coordinates >= r are reduced; R may be off the
 *     curve, of small order, the identity or (0, 0) (the argument of bjj_hip_signer.h, per key).
 *     signer_idx[i] >= k is DATA, not an error: ok[i] = BJJ_VERIFY_BAD_SIGNER, the call still returns BJJ_OK, and nothing outside
 *     the set is read.
 *     signer_idx: n uint32, r_xy: n 64-byte records, s and msg: n 32-byte little-endian records, ok: n bytes.
 *     A NULL array (n > 0), a NULL set, a set of another context or a freed one: BJJ_E_INVALID; a rejected call writes nothing.
 *     n == 0 is BJJ_OK and looks at nothing.  The host form is synchronous: one copy in per array, one launch, one copy out (pinned
 *     or pageable arrays, identical results).  The _dev form follows the *_dev contract of bjj_hip.h: every input pointer 16-byte
 *     aligned (d_ok: any non-NULL address), enqueued on `stream` (NULL = the context's stream), no synchronisation.  There is no
 *     per-call scratch, so calls on different streams share nothing and run at once.  A set must outlive the calls that use it. */
#ifndef BJJ_HIP_SIGNER_SET_H
#define BJJ_HIP_SIGNER_SET_H

#include "bjj_hip_signer.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bjj_signer_set bjj_signer_set;
#define BJJ_VERIFY_BAD_SIGNER 3   /* ok[i] when signer_idx[i] >= the set's size */

int bjj_signer_set_create(bjj_ctx* ctx, const uint8_t* pks_xy /* k*64 */, size_t k, int window_bits, bjj_signer_set** out,
                          int64_t* out_first_off_curve /* may be NULL */);
int bjj_signer_set_free(bjj_ctx* ctx, bjj_signer_set* set);
int bjj_signer_set_info(const bjj_signer_set* set, uint64_t* n_signers, int* window_bits, int* n_windows, uint64_t* table_bytes);
int bjj_signer_set_check(bjj_ctx* ctx, const bjj_signer_set* set, uint64_t* n_bad);

int bjj_eddsa_verify_set(bjj_ctx* ctx, const bjj_signer_set* set, const uint32_t* signer_idx /* n */, const uint8_t* r_xy /* n*64 */,
                         const uint8_t* s /* n*32 */, const uint8_t* msg /* n*32 */, size_t n, uint8_t* ok /* n */);
int bjj_eddsa_verify_set_dev(bjj_ctx* ctx, const bjj_signer_set* set, const void* d_signer_idx, const void* d_r_xy, const void* d_s,
                             const void* d_msg, size_t n, void* d_ok, void* stream);
/* ok: 0 / 1 / 2 as bjj_schnorr_verify, or 3 */
int bjj_schnorr_verify_set(bjj_ctx* ctx, const bjj_signer_set* set, const uint32_t* signer_idx /* n */, const uint8_t* r_xy /* n*64 */,
                           const uint8_t* s /* n*32 */, const uint8_t* msg /* n*32 */, size_t n, uint8_t* ok /* n */);
int bjj_schnorr_verify_set_dev(bjj_ctx* ctx, const bjj_signer_set* set, const void* d_signer_idx, const void* d_r_xy, const void* d_s,
                               const void* d_msg, size_t n, void* d_ok, void* stream);

#ifdef __cplusplus
}
#endif
#endif
