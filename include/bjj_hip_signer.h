/* bjj_hip_signer.h -- signature verification against ONE signer's fixed-base table (extension of bjj_hip_bases.h, same library).
 *
 * bjj_eddsa_verify spends most of its time on (8 hm) * pk, a variable-base multiplication with a per-lane table.  A caller who
 * checks many signatures under one key -- a rollup operator, an oracle feed, an attestation service -- builds the key's table once
 * with bjj_base_create and then verifies with table gathers only: one Poseidon permutation, 8 hm * pk over the signer's table,
 * s * B8 over the context's own table, the reference's last addition and a comparison.  No inversion, no second code path.
 *
 * ok[i] is byte for byte what bjj_eddsa_verify / bjj_schnorr_verify writes when pk_xy is the signer's point repeated n times,
 * for every input those accept: any 256-bit s (unreduced); msg > Q gives 0 (EdDSA) or 2 (Schnorr), msg == Q wraps to 0 as there;
 * R coordinates >= r are reduced mod r; R may be off the curve, of small order, the identity or (0, 0) -- the verdict is the
 * reference's (verify, src/lib.rs:395-412; verify_schnorr, :375-385) in every case.  The public key that is hashed is the base's
 * point reduced mod r, the value its table was built from.  Why this holds without replaying the reference: the base is ON the
 * curve (bjj_base_create refuses any other point), so l = s * B8 and t = 8 hm * pk are canonical points however they are
 * evaluated, and PointProjective::add (:88-131) is homogeneous in its second operand, so R + t may be taken with t projective
 * and compared with l by cross-multiplication.
 *
 * signer   a base of THIS context, of any window_bits bjj_base_create accepts; the B8 side uses the context's own table.
 *          NULL, a base of another context or a freed one: BJJ_E_INVALID.
 * r_xy     n 64-byte records (R.x, R.y), s and msg n 32-byte little-endian records, ok n bytes.
 * A NULL array (n > 0) is BJJ_E_INVALID; a rejected call writes nothing.  n == 0 is BJJ_OK and looks at nothing.
 * The host form is synchronous: one copy in per array, one launch, one copy out (pinned or pageable arrays, identical results);
 * it is not the chunked pipeline of bjj_eddsa_verify.  The _dev form follows the *_dev contract of bjj_hip.h: every input pointer
 * 16-byte aligned (d_ok: any non-NULL address, as in bjj_eddsa_verify_dev), enqueued on `stream` (NULL = the context's stream),
 * no synchronisation.  The kernel uses no per-call scratch, so calls on different streams share nothing and run at once.
 * A base must outlive the calls that use it (bjj_base_free waits). */
#ifndef BJJ_HIP_SIGNER_H
#define BJJ_HIP_SIGNER_H

#include "bjj_hip_bases.h"

#ifdef __cplusplus
extern "C" {
#endif

int bjj_eddsa_verify_signer(bjj_ctx* ctx, const bjj_base* signer, const uint8_t* r_xy /* n*64 */, const uint8_t* s /* n*32 */,
                            const uint8_t* msg /* n*32 */, size_t n, uint8_t* ok /* n */);
int bjj_eddsa_verify_signer_dev(bjj_ctx* ctx, const bjj_base* signer, const void* d_r_xy, const void* d_s, const void* d_msg,
                                size_t n, void* d_ok, void* stream);
/* ok: 0 / 1 / 2 as bjj_schnorr_verify */
int bjj_schnorr_verify_signer(bjj_ctx* ctx, const bjj_base* signer, const uint8_t* r_xy /* n*64 */, const uint8_t* s /* n*32 */,
                              const uint8_t* msg /* n*32 */, size_t n, uint8_t* ok /* n */);
int bjj_schnorr_verify_signer_dev(bjj_ctx* ctx, const bjj_base* signer, const void* d_r_xy, const void* d_s, const void* d_msg,
                                  size_t n, void* d_ok, void* stream);

#ifdef __cplusplus
}
#endif
#endif
