/* bjj_hip_bases.h -- reusable fixed-base tables for caller-chosen points (extension of bjj_hip.h, same library).
 *
 * bjj_mul_fixed_base owes its speed to a window table precomputed for ONE point, B8.  A caller who multiplies another point by
 * many scalars -- a public key (ElGamal, ECDH, h * A of one signer), the generators of a Pedersen commitment -- builds such a
 * table once with bjj_base_create and then runs
 *   out[i] = sum_{j < t} scalars[j][i] * P_j                       i = 0 .. n - 1,  1 <= t <= BJJ_MAX_BASES
 * over t tables in ONE launch.  out[i] is byte for byte the reference fold: k * P = Point::mul_scalar (src/lib.rs:149-164) per
 * term, the sum PointProjective::add (src/lib.rs:88-131) folded from (0, 1, 1), then .affine() (src/lib.rs:70-85).  The argument
 * is bjj_msm's (bjj_hip.h): every base is ON the curve (bjj_base_create refuses any other point), so the addition law is complete
 * (A a square, D a non-square), the group has order 8l (so k mod 8l is exact) and canonical affine coordinates are unique: any
 * correct evaluation gives the bytes of the fold in any order, and of bjj_mul_var_base followed by bjj_point_add.
 *
 * bjj_base_create   synchronous, like bjj_init.  point_xy: one 64-byte record; coordinates >= r are reduced mod r.  A point that
 *                   fails A x^2 + y^2 = 1 + D x^2 y^2 is BJJ_E_INVALID and *out is not written (a table handle is not a per-item
 *                   outcome, and there is no exact-replay path for a table).  The identity and the small-order points are valid
 *                   bases.  window_bits: 0 (= 16) or 4..28, anything else BJJ_E_INVALID; BJJ_E_NOMEM when the table does not fit.
 *                   The table has the layout of the B8 table -- signed digits, 2^(W-1) + 1 entries of 128 bytes per window --
 *                   with n_windows = ceil(255 / W) and scalars reduced mod 8l: a curve point has an order that divides 8l, not
 *                   l, and 8l < 2^254 leaves the top window at most W - 1 bits, so it absorbs the last carry.  The finished
 *                   table is proved entry by entry (the induction check of bjj_check_table, anchored at the caller's point)
 *                   before the call returns: BJJ_E_HIP if any condition is violated.  The context owns the table:
 *                   bjj_base_free releases it, bjj_free releases what is left.
 * bjj_base_free     waits for the work the context has enqueued, then releases the table.  NULL base: BJJ_OK.
 * bjj_base_info     window_bits, n_windows, table_bytes = (2^(W-1) + 1) * n_windows * 128 (any of the three may be NULL).
 * bjj_base_check    runs the induction check again; *n_bad = number of violated conditions (0 = sound).
 * bjj_mul_bases     bases[j] == NULL means the context's own B8 table (scalar reduced mod l, the context's window_bits):
 *                   bases = {NULL} gives the bytes of bjj_mul_fixed_base, {NULL, pk} with scalars {m, r} is the second ElGamal
 *                   component m * B8 + r * PK.  The same base may appear more than once.  t outside 1..BJJ_MAX_BASES, a NULL
 *                   array, a NULL scalars[j] or a base of another context: BJJ_E_INVALID.  n == 0 is BJJ_OK and touches
 *                   nothing.  Scalars are 32-byte little-endian records, any 256-bit value.  The pointer arrays are read on
 *                   the host during the call and no pointer is kept past return.
 *                   The host form is synchronous: one copy in, one launch, one copy out (pinned or pageable arrays, identical
 *                   results); it is not the chunked pipeline of bjj_mul_fixed_base.  The _dev form follows the *_dev contract
 *                   of bjj_hip.h: d_scalars is a HOST array of t device pointers, every device pointer 16-byte aligned,
 *                   enqueued on `stream` (NULL = the context's stream), no synchronisation; one scratch set per stream, so
 *                   two calls on two streams run at once.  A base must outlive the calls that use it (bjj_base_free waits). */
#ifndef BJJ_HIP_BASES_H
#define BJJ_HIP_BASES_H

#include "bjj_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bjj_base bjj_base;
#define BJJ_MAX_BASES 8

int bjj_base_create(bjj_ctx* ctx, const uint8_t* point_xy /* 64 */, int window_bits, bjj_base** out);
int bjj_base_free(bjj_ctx* ctx, bjj_base* base);
int bjj_base_info(const bjj_base* base, int* window_bits, int* n_windows, uint64_t* table_bytes);
int bjj_base_check(bjj_ctx* ctx, const bjj_base* base, uint64_t* n_bad);
int bjj_mul_bases(bjj_ctx* ctx, const bjj_base* const* bases /* t, NULL = B8 */, int t,
                  const uint8_t* const* scalars /* t pointers, each n*32 */, size_t n, uint8_t* out_xy /* n*64 */);
int bjj_mul_bases_dev(bjj_ctx* ctx, const bjj_base* const* bases, int t, const void* const* d_scalars /* host array of t device pointers */,
                      size_t n, void* d_out_xy, void* stream);

#ifdef __cplusplus
}
#endif
#endif
