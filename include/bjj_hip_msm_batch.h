/* bjj_hip_msm_batch.h -- many independent multi-scalar multiplications in one call (extension of bjj_hip.h, same library).
 *
 * Batched multi-scalar multiplication: m results from ONE point array, ONE scalar array and m + 1 offsets (CSR segments),
 *   Q_s = sum_{i in [offsets[s], offsets[s+1])} k_i * P_i        s = 0 .. m - 1
 * where every Q_s is byte for byte what bjj_msm returns for that slice of the arrays: the fold of Point::mul_scalar
 * (src/lib.rs:149-164) with PointProjective::add (src/lib.rs:88-131) from (0, 1, 1), then .affine() (src/lib.rs:70-85) -- see the
 * block above bjj_msm in bjj_hip.h.  One Pedersen commitment per matrix row, one aggregated key per committee, one linear
 * combination per proof: the m sums share one launch chain (the segment number is part of the bucket sort key) instead of
 * paying bjj_msm's fixed ~1.3 ms per sum.
 * Inputs: n points (64-byte records), n scalars (32-byte records, any 256-bit value), m + 1 offsets (uint64, host byte order)
 * with offsets[0] == 0, offsets[s] <= offsets[s+1], offsets[m] == n.  Outputs: m 64-byte results, m int64 status words.
 *   empty segment   out[s] = the identity (0, 1), status[s] = -1.
 *   off-curve       spoils only its own segment: out[s] = (0, 0), status[s] = the SMALLEST offending index as a position in the
 *                   whole pts array (for m == 1: bjj_msm's status word); every other segment is what it is without that point's
 *                   segment; otherwise status[s] = -1.  The return code stays 0 and nothing carries over to the next call.
 *   m == 0          requires n == 0 (else BJJ_E_INVALID); nothing is read or written, BJJ_OK.
 *   window_bits     0 = the library picks the bucket width c from the mean segment length n / m (the same value in both
 *                   forms: the bytes never depend on it); 4..20 forces c; anything else is BJJ_E_INVALID.
 *   limits          n < 2^32, and the sort key (s W + j) B + |d| - 1 has 31 bits: m * W * B < 2^31 with W = ceil(255 / c),
 *                   B = 2^(c-1) -- BJJ_E_INVALID otherwise (checked before any allocation; window_bits = 0 narrows c to fit,
 *                   which allows up to 2^22 - 1 segments per call).
 *   bad offsets     host form: checked on the host before anything is enqueued, BJJ_E_INVALID.  Device form: the offsets are
 *                   device data and the call does not synchronise, so a violation is reported as DATA: every status word = -2,
 *                   every result (0, 0), return code 0.  No content of the offsets array makes the library touch memory
 *                   outside the caller's arrays (every lane's segment is clamped to [0, m - 1]).
 * Scratch: bjj_msm's per-item part (about n * (164 + 8 W) bytes) plus 172 * m * W * B bytes for the buckets and their
 * counters; BJJ_E_NOMEM when the device cannot provide it.  The host form is synchronous and copies the caller's arrays
 * (pinned or pageable, identical results) once to the device; the _dev form follows the *_dev contract of bjj_hip.h (16-byte
 * aligned device pointers, enqueued on `stream`, NULL = the context's stream, no synchronisation; one scratch set per stream, so
 * two calls on two streams run at once). */
#ifndef BJJ_HIP_MSM_BATCH_H
#define BJJ_HIP_MSM_BATCH_H

#include "bjj_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int bjj_msm_batch(bjj_ctx* ctx, const uint8_t* pts_xy /* n*64 */, const uint8_t* scalars /* n*32 */, size_t n,
                  const uint64_t* offsets /* m+1 */, size_t m, int window_bits,
                  uint8_t* out_xy /* m*64 */, int64_t* out_first_off_curve /* m */);
int bjj_msm_batch_dev(bjj_ctx* ctx, const void* d_pts_xy, const void* d_scalars, size_t n,
                      const void* d_offsets /* (m+1) uint64 */, size_t m, int window_bits,
                      void* d_out_xy /* m*64 */, void* d_first_off_curve /* m int64 */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
