/* bjj_hip_point_sum.h -- signed point sums over CSR segments in one call (extension of bjj_hip.h, same library).
 *
 * m results from ONE point array, an optional sign array and m + 1 offsets (CSR segments),
 *   Q_s = sum_{i in [offsets[s], offsets[s+1])} +-P_i        s = 0 .. m - 1
 * where term i is subtracted when neg[i] != 0, with -(x, y) = (-x, y); neg == NULL adds every term.  This is the whole of
 * additive homomorphism: a tally is a sum of ciphertexts per candidate, a balance credits minus debits, an aggregated key a sum of
 * public keys, C2 - sk * C1 a signed sum of two terms.
 * Parity: every Q_s is byte for byte what bjj_msm_batch (bjj_hip_msm_batch.h) returns for the same points and offsets with the
 * scalar 1 for an added term and 8l - 1 for a subtracted one (every curve point has an order dividing 8l, and 8l - 1 < 2^256) --
 * that is, the fold of PointProjective::add (src/lib.rs:88-131) from (0, 1, 1) followed by .affine() (src/lib.rs:70-85).  The
 * addition law is complete on the curve and canonical affine coordinates are unique, so the bytes do not depend on the order in
 * which the library associates the terms.  Coordinates >= r are treated exactly as bjj_msm_batch treats them.  The identity,
 * points of small order, duplicates and P, -P pairs are ordinary inputs.
 * Inputs: n points (64-byte records), n sign bytes or NULL, m + 1 offsets (uint64, host byte order) with offsets[0] == 0,
 * offsets[s] <= offsets[s+1], offsets[m] == n.  Outputs: m 64-byte results, m int64 status words.
 *   empty segment   out[s] = the identity (0, 1), status[s] = -1.
 *   off-curve       spoils only its own segment: out[s] = (0, 0), status[s] = the SMALLEST offending index as a position in the
 *                   whole pts array, whether the term is added or subtracted; otherwise status[s] = -1.  The return code stays 0
 *                   and nothing carries over to the next call.
 *   m == 0          requires n == 0 (else BJJ_E_INVALID); nothing is read or written, BJJ_OK.
 *   limits          n < 2^32 and m < 2^32 (BJJ_E_INVALID otherwise).  Nothing is sorted, so bjj_msm_batch's bound on the number
 *                   of segments does not apply.
 *   NULL            a NULL ctx or a NULL required array (everything but neg; pts_xy only when n > 0): BJJ_E_INVALID, nothing
 *                   is written.
 *   bad offsets     host form: checked on the host before anything is enqueued, BJJ_E_INVALID.  Device form: the offsets are
 *                   device data and the call does not synchronise, so a violation is reported as DATA: every status word = -2,
 *                   every result (0, 0), return code 0.  No content of the offsets array makes the library touch memory
 *                   outside the caller's arrays (every lane's segment is clamped to [0, m - 1]).
 * Cost: one pass over the points (each record is read once, checked, negated and added), one inversion per written result,
 * batched per workgroup, and a few short passes over per-tile partial sums.  Scratch: 320 bytes per 256 points (two partial sums
 * per tile) plus a smaller list for the later levels; BJJ_E_NOMEM when the device cannot provide it.  The host form is synchronous
 * and copies the caller's arrays (pinned or pageable, identical results) once to the device and the results once back; the _dev
 * form follows the *_dev contract of bjj_hip.h (d_pts_xy, d_offsets, d_out_xy and d_first_off_curve 16-byte aligned, d_neg any
 * address; enqueued on `stream`, NULL = the context's stream, no synchronisation; one scratch set per stream, so two calls on two
 * streams run at once). */
#ifndef BJJ_HIP_POINT_SUM_H
#define BJJ_HIP_POINT_SUM_H

#include "bjj_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int bjj_point_sum(bjj_ctx* ctx, const uint8_t* pts_xy /* n*64 */, const uint8_t* neg /* n bytes, or NULL */, size_t n,
                  const uint64_t* offsets /* m+1 */, size_t m, uint8_t* out_xy /* m*64 */, int64_t* out_first_off_curve /* m */);
int bjj_point_sum_dev(bjj_ctx* ctx, const void* d_pts_xy, const void* d_neg /* or NULL */, size_t n,
                      const void* d_offsets /* (m+1) uint64 */, size_t m, void* d_out_xy, void* d_first_off_curve, void* stream);

#ifdef __cplusplus
}
#endif
#endif
