/* bjj_hip_common_scalar.h -- one scalar, many points: out_i = A_i +- k * P_i with ONE k for the whole call, the prime-order-subgroup
 * check l * P = identity, and exponential-ElGamal decryption in one call (extension of bjj_hip.h, same library).
 *
 * bjj_mul_var_base takes a scalar per item.  Several server-side workloads have one scalar for all of them: an auditor or wallet
 * trial-decrypting every ciphertext with its one key, a trustee's partial decryptions sk_j * C1_i in threshold ElGamal, ECDH of one
 * secret against many peers, cofactor clearing (8 * P), and the subgroup check public keys and ciphertext components need before
 * they are summed (circomlib's inSubgroup).  With one scalar per launch every digit is the same for all lanes: the host recodes it
 * once, zero digits and leading zeros cost nothing (8 * P is three doublings), a subtraction is a sign flip of the digits, and
 * the subgroup check needs no inversion at all.
 *
 * The scalar.  `scalar` and `sk` are 32 little-endian bytes of ANY value below 2^256, always on the HOST, in the _dev forms too.  The
 *     scalar is read, reduced mod 8l (the group order) and recoded into signed digits before the call returns; the digits travel to
 *     the kernel in its arguments -- no device allocation, no copy -- and the caller may overwrite the scalar as soon as the call
 *     returns.  k == 0 (mod 8l) gives A_i.
 *     NOT CONSTANT TIME: the duration of a launch depends on the scalar's length and on its digit pattern (a zero digit is a doubling,
 *     a non-zero one a doubling and an addition; the loop starts at the top digit), and the form of the kernel is chosen from the
 *     digits.  This is the opposite of bjj_set_signer_constant_time, which these calls do not look at.  Do not use them where the
 *     time of a call is visible to a party that must not learn the scalar.
 *
 * bjj_mul_common / bjj_mul_common_dev   for each item, P = pts_xy[i] and A = add_xy[i] (add_xy == NULL: A = the identity (0, 1)),
 *     coordinates >= r reduced mod r:
 *       P or A fails the curve equation (this includes (0, 0))     ok[i] = BJJ_COMMON_OFF_CURVE   out[i] = (0, 0)
 *       otherwise                                                  ok[i] = BJJ_COMMON_OK          out[i] = A + k * P  (subtract == 0)
 *                                                                                                       or  A - k * P  (subtract != 0)
 *     as canonical affine bytes: byte for byte bjj_point_add(A, +-bjj_mul_var_base(P, k)).  This holds for every on-curve input, the
 *     points of order 1, 2, 4, 8 and points outside the prime-order subgroup included (the curve's addition law is complete).
 * bjj_in_subgroup / bjj_in_subgroup_dev   the same kernel with the constant k = l and a projective comparison in place of the
 *     inversion; one byte per item and no point output:
 *       ok[i] = 1   P is on the curve and l * P = identity (P is in the prime-order subgroup; the identity is)
 *       ok[i] = 0   P is on the curve and l * P is another point (one of order 2, 4 or 8)
 *       ok[i] = 2   P fails the curve equation
 * bjj_elgamal_decrypt / bjj_elgamal_decrypt_dev   m_i from (C1_i, C2_i) = (r * G, m * G + r * PK) under sk, PK = sk * G, `table` the
 *     bjj_dlog_table of G (bjj_hip_dlog.h): M_i = C2_i - sk * C1_i goes into a block the context owns (per stream, like its other
 *     scratch), and the launches of bjj_dlog_dev run over that block into out_m / ok.  An off-curve C1_i or C2_i makes M_i = (0, 0),
 *     which the logarithm reports as BJJ_DLOG_OFF_CURVE with UINT64_MAX; every other item gets exactly what bjj_dlog gives for M_i --
 *     never a false answer, a wrong key gives BJJ_DLOG_NOT_IN_RANGE -- with the same range_bits rules and the same cutting into launches
 *     (BJJ_DLOG_LAUNCH_STEPS).  A NULL table, a table of another context or a freed one is BJJ_E_INVALID.
 *
 * Arguments.  n == 0 is BJJ_OK and touches nothing.  A NULL ctx, a NULL scalar, or a NULL required array with n > 0 is
 *     BJJ_E_INVALID (add_xy may be NULL); a rejected call writes nothing, and a NULL ctx is answered before any device is touched.
 *     The host forms are synchronous: one copy in per array, the launches, one copy out per output array (pinned or pageable arrays,
 *     identical results); there is no chunked pipeline.  The _dev forms follow the *_dev contract of bjj_hip.h: the point arrays and
 *     d_out_m 16-byte aligned, d_ok any non-NULL address, enqueued on `stream` (NULL = the context's stream), no synchronisation.
 *
 * The two forms of the kernel.  Table-free: plain non-adjacent form, P stays in registers, one mixed addition per non-zero digit.
 *     Table: width-5 non-adjacent form over {P, 3P, .., 15P} in the lane's variable-base table.  The host counts field
 *     multiplications for both recodings and takes the cheaper one, per call: 8 * P and short scalars run table-free.  The
 *     environment variable BJJ_COMMON_FORM (read once at bjj_init; "naf" or "0" = table-free, "table" or "1" = table) forces one form
 *     for every call of the context: for A/B measurements and tests.  The results do not depend on the form. */
#ifndef BJJ_HIP_COMMON_SCALAR_H
#define BJJ_HIP_COMMON_SCALAR_H

#include "bjj_hip.h"
#include "bjj_hip_dlog.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BJJ_COMMON_OK        1
#define BJJ_COMMON_OFF_CURVE 2

int bjj_mul_common(bjj_ctx* ctx, const uint8_t* scalar /* 32, HOST */, const uint8_t* pts_xy /* n*64 */, const uint8_t* add_xy /* n*64 or NULL */,
                   int subtract, size_t n, uint8_t* out_xy /* n*64 */, uint8_t* ok /* n */);
int bjj_mul_common_dev(bjj_ctx* ctx, const uint8_t* scalar /* 32, HOST */, const void* d_pts_xy, const void* d_add_xy, int subtract, size_t n,
                       void* d_out_xy, void* d_ok, void* stream);
int bjj_in_subgroup(bjj_ctx* ctx, const uint8_t* pts_xy /* n*64 */, size_t n, uint8_t* ok /* n */);
int bjj_in_subgroup_dev(bjj_ctx* ctx, const void* d_pts_xy, size_t n, void* d_ok, void* stream);
int bjj_elgamal_decrypt(bjj_ctx* ctx, const bjj_dlog_table* table, const uint8_t* sk /* 32, HOST */, const uint8_t* c1_xy /* n*64 */,
                        const uint8_t* c2_xy /* n*64 */, size_t n, int range_bits, uint64_t* out_m /* n */, uint8_t* ok /* n */);
int bjj_elgamal_decrypt_dev(bjj_ctx* ctx, const bjj_dlog_table* table, const uint8_t* sk /* 32, HOST */, const void* d_c1_xy,
                            const void* d_c2_xy, size_t n, int range_bits, void* d_out_m, void* d_ok, void* stream);

#ifdef __cplusplus
}
#endif
#endif
