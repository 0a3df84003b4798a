/* bjj_hip_dlog.h -- batched small-range discrete logarithms: m from P = m * G, 0 <= m < 2^range_bits (extension of bjj_hip.h,
 * same library).
 *
 * Exponential ElGamal over BabyJubJub encrypts a small value m -- a balance, a vote count, a 32-bit amount -- as
 * (C1, C2) = (r * B8, m * B8 + r * PK); bjj_mul_bases (bjj_hip_bases.h) computes the second component.  Decryption is
 * M = C2 - sk * C1, which bjj_mul_var_base and bjj_point_add do, and then m from M = m * B8: a discrete logarithm that is feasible
 * because m is small.  The same step recovers v from v * G for any generator a caller uses, e.g. a Pedersen G.  The method is
 * baby-step giant-step: a hash table of j * G for j = 0 .. 2^baby_bits, keyed on y -- on this curve -(x, y) = (-x, y), so one
 * lookup answers for +j and -j, a span of 2^(baby_bits+1) values -- and at most 2^(range_bits - baby_bits - 1) giant steps per item.
 *
 * bjj_dlog_table_create  synchronous, like bjj_base_create.  point_xy: one 64-byte record (x, y) on the HOST, coordinates >= r are
 *     reduced mod r; NULL means B8.  baby_bits: 0 (= the default, 24: a 512 MiB table, the fastest 32-bit search of the widths
 *     measured -- 2^20 logarithms in 31 ms, against 127 ms with 22 bits and 128 MiB) or 4..28, anything else is BJJ_E_INVALID.
 *     A point that fails the curve equation is BJJ_E_INVALID, and so is a base G with 8 * G = identity: the identity and the seven other points of
 *     order <= 8.  Every accepted base therefore has order >= l > 2^250, far above any range this header admits, so m * G = P has
 *     AT MOST ONE solution in range: every answer of bjj_dlog is unique.  On BJJ_E_INVALID *out is not written.  BJJ_E_NOMEM when
 *     the device refuses the allocation.  The table has passed bjj_dlog_table_check when the call returns: BJJ_E_HIP if any condition
 *     is violated.  The context owns the table: bjj_dlog_table_free waits for the context's enqueued work and releases it (NULL
 *     table: BJJ_OK), bjj_free releases what is left.  A table of another context or a freed one is BJJ_E_INVALID in every call.
 * bjj_dlog_table_info    any out pointer may be NULL.  entries = 2^baby_bits + 1; table_bytes = 2^(baby_bits+5): 2^(baby_bits+2)
 *     slots of 8 bytes, a quarter full (128 MiB at 22 bits, 512 MiB at 24, 8 GiB at 28).
 * bjj_dlog_table_check   for every j in 0 .. 2^baby_bits, j * G recomputed from the base point by double-and-add is looked up and
 *     must answer exactly j; the occupied slots must number `entries` and hold values in range.  *n_bad = violated conditions.
 * bjj_dlog_table_base    the table's base point, 64 bytes, coordinates reduced.
 * bjj_dlog_max_range_bits  baby_bits + 1 + BJJ_DLOG_MAX_GIANT_BITS (41 at 24 bits, 45 at 28), or -1 for a NULL table.  The cap
 *     bounds the work of one item: an item that is not in range costs 2^(range_bits - baby_bits - 1) <= 2^16 giant steps of 18
 *     field multiplications each, and a call costs n times that; a wider range wants a wider table, not a longer walk.
 *
 * bjj_dlog / bjj_dlog_dev   for each item, P = the record with coordinates reduced mod r:
 *       P fails the curve equation (this includes (0, 0))          ok[i] = BJJ_DLOG_OFF_CURVE     out_m[i] = UINT64_MAX
 *       an m in [0, 2^range_bits) with m * G = P exists            ok[i] = BJJ_DLOG_FOUND         out_m[i] = that m
 *       neither                                                    ok[i] = BJJ_DLOG_NOT_IN_RANGE  out_m[i] = UINT64_MAX
 *     Never a false answer: a hash hit is a candidate only, and every reported m has been confirmed on the device by recomputing
 *     the baby step j * G and comparing it with P - c * G (c the centre of the giant step, m = c +- j) in full-width x and y.
 *     range_bits: 1 .. bjj_dlog_max_range_bits(table), anything else BJJ_E_INVALID; it may be smaller than baby_bits (a hit
 *     with m >= 2^range_bits is then "not in range").  pts_xy: n 64-byte records, out_m: n uint64, ok: n bytes.
 *     n == 0 is BJJ_OK and touches nothing.  A NULL array with n > 0, a NULL table or a NULL ctx is BJJ_E_INVALID; a rejected call
 *     writes nothing.  The host form is synchronous: one copy in, the launches, one copy out per output array (pinned or pageable
 *     arrays, identical results).  The _dev form follows the *_dev contract of bjj_hip.h: d_pts_xy and d_out_m 16-byte aligned,
 *     d_ok any non-NULL address, enqueued on `stream` (NULL = the context's stream), no synchronisation.  The search keeps its
 *     state in registers and in the two output arrays -- no scratch -- so calls on different streams share nothing and run at once.
 *     A long call is cut into consecutive launches: no launch performs more than 2^27 giant steps over all its items (29 ms of
 *     the whole chip, measured on an idle card) and none walks an item further than 512 steps (29 ms for a launch of few items too:
 *     a workgroup's step takes the same time whatever the rest of the chip does).  The environment variable BJJ_DLOG_LAUNCH_STEPS
 *     (an integer >= 64, read once at bjj_init) sets another bound for the first of the two.  The results do not depend on either.
 *     Between the launches of a _dev call d_ok holds 0xFF for the items still being walked; the last launch leaves none.
 *     A table must outlive the calls that use it (bjj_dlog_table_free waits). */
#ifndef BJJ_HIP_DLOG_H
#define BJJ_HIP_DLOG_H

#include "bjj_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bjj_dlog_table bjj_dlog_table;
#define BJJ_DLOG_NOT_IN_RANGE 0
#define BJJ_DLOG_FOUND        1
#define BJJ_DLOG_OFF_CURVE    2
#define BJJ_DLOG_MAX_GIANT_BITS 16

int bjj_dlog_table_create(bjj_ctx* ctx, const uint8_t* point_xy /* 64, NULL = B8 */, int baby_bits, bjj_dlog_table** out);
int bjj_dlog_table_free(bjj_ctx* ctx, bjj_dlog_table* table);
int bjj_dlog_table_info(const bjj_dlog_table* table, int* baby_bits, uint64_t* entries, uint64_t* table_bytes);
int bjj_dlog_table_check(bjj_ctx* ctx, const bjj_dlog_table* table, uint64_t* n_bad);
int bjj_dlog_table_base(const bjj_dlog_table* table, uint8_t* out_xy /* 64 */);
int bjj_dlog_max_range_bits(const bjj_dlog_table* table);
int bjj_dlog(bjj_ctx* ctx, const bjj_dlog_table* table, const uint8_t* pts_xy /* n*64 */, size_t n, int range_bits,
             uint64_t* out_m /* n */, uint8_t* ok /* n */);
int bjj_dlog_dev(bjj_ctx* ctx, const bjj_dlog_table* table, const void* d_pts_xy, size_t n, int range_bits,
                 void* d_out_m, void* d_ok, void* stream);

#ifdef __cplusplus
}
#endif
#endif
