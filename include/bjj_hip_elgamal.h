/* bjj_hip_elgamal.h -- exponential-ElGamal encryption to one public key and re-randomisation, one launch per call (extension of
 * bjj_hip.h, same library).
 *
 * A ciphertext of m under PK is (C1, C2) = (r * G, m * G + r * PK).  Composed from the older calls that is bjj_mul_fixed_base(r) or
 * bjj_mul_bases({g}, {r}) for C1 and bjj_mul_bases({g, pk}, {m, r}) for C2: r is reduced and recoded twice, two launches, two
 * inversion passes, and m -- below 2^64, or bjj_dlog could not give it back -- walks every window of G's table.  Here one kernel
 * runs the r-chain over G, a SHORT m-chain over G (ceil(65 / W) windows) and the r-chain over PK, and one inversion pass finishes
 * both points.  With add arrays it computes C' = C + Enc(m, r): re-randomisation (m == NULL), re-encryption before publication,
 * adding a public delta to an encrypted balance, accumulating into a running ciphertext.
 *
 * Results.  For every item, with A1 = add_c1_xy[i] and A2 = add_c2_xy[i] (both the identity (0, 1) when the add arrays are NULL):
 *       out_c1_xy[i] = A1 + r * G
 *       out_c2_xy[i] = A2 + m * G + r * PK
 *     as canonical affine bytes: out_c1 is byte for byte bjj_point_add(A1, bjj_mul_bases({g}, {r})), out_c2 byte for byte
 *     bjj_point_add(A2, bjj_mul_bases({g, pk}, {m as a 32-byte scalar, r})); without add arrays they are the two bjj_mul_bases
 *     results themselves.  That is the argument of bjj_hip_bases.h: the bases are on the curve, the curve's addition law is
 *     complete, and the canonical affine coordinates of a point are unique.
 * Scalars.  r is 32 little-endian bytes of ANY 256-bit value per item; it is reduced mod l for the context's B8 table and mod 8l
 *     for a caller's table, exactly as bjj_mul_bases treats each base.  m is any uint64_t per item.  m == NULL is m = 0 for every
 *     item and the m-chain is not run at all (with add arrays: re-randomisation).
 * Handles.  g == NULL is the context's B8 table; otherwise g is a base of this context (bjj_base_create; the G of
 *     bjj_dlog_table_create).  pk is a base of this context for the recipient's key; pk == NULL is BJJ_E_INVALID: a missing key
 *     is not B8.  A base of another context, or a freed one, is BJJ_E_INVALID.
 * Add arrays.  Both or neither; one alone is BJJ_E_INVALID.  Coordinates >= r are reduced mod r.  An A1 or A2 that fails the curve
 *     equation -- this includes (0, 0), the error output of bjj_point_sum and of the other calls -- gives
 *       ok[i] = BJJ_ELGAMAL_OFF_CURVE   out_c1_xy[i] = out_c2_xy[i] = (0, 0)
 *     and disturbs no other item; every other item gets ok[i] = BJJ_ELGAMAL_OK.  ok is required with add arrays.  Without them it
 *     may be NULL; if given, it is filled with BJJ_ELGAMAL_OK.
 * Arguments.  n == 0 is BJJ_OK and touches nothing.  A NULL ctx is BJJ_E_INVALID and is answered before any device is touched; a
 *     NULL pk, r, out_c1_xy or out_c2_xy with n > 0 is BJJ_E_INVALID.  A rejected call writes nothing.
 * Host form.  Synchronous and single-launch: one copy in per array given (up to four), the launch, one copy out per output
 *     array (up to three).  Pinned and pageable memory give identical results.  There is no chunked pipeline.
 * _dev form.  The *_dev contract of bjj_hip.h: every array except d_ok 16-byte aligned (d_ok: any address), enqueued on `stream`
 *     (NULL = the context's stream), no synchronisation; one scratch set per stream.  d_out_c1_xy == d_add_c1_xy TOGETHER WITH
 *     d_out_c2_xy == d_add_c2_xy (exactly equal pointers) is allowed: in-place re-randomisation.  Any other overlap between the
 *     arrays of a call is undefined.
 * NOT CONSTANT TIME, like bjj_mul_bases: the table reads depend on the digits of r and m.  These calls do not look at
 *     bjj_set_signer_constant_time.  Do not use them where the memory access pattern of a call is visible to a party that must
 *     not learn r or m. */
#ifndef BJJ_HIP_ELGAMAL_H
#define BJJ_HIP_ELGAMAL_H

#include "bjj_hip.h"
#include "bjj_hip_bases.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BJJ_ELGAMAL_OK        1
#define BJJ_ELGAMAL_OFF_CURVE 2

int bjj_elgamal_encrypt(bjj_ctx* ctx, const bjj_base* g /* NULL = B8 */, const bjj_base* pk, const uint64_t* m /* n, or NULL = all 0 */,
                        const uint8_t* r /* n*32 */, const uint8_t* add_c1_xy, const uint8_t* add_c2_xy /* n*64 each, both or neither */,
                        size_t n, uint8_t* out_c1_xy /* n*64 */, uint8_t* out_c2_xy /* n*64 */, uint8_t* ok /* n */);
int bjj_elgamal_encrypt_dev(bjj_ctx* ctx, const bjj_base* g /* NULL = B8 */, const bjj_base* pk, const void* d_m, const void* d_r,
                            const void* d_add_c1_xy, const void* d_add_c2_xy, size_t n, void* d_out_c1_xy, void* d_out_c2_xy, void* d_ok,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif
