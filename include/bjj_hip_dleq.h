/* bjj_hip_dleq.h -- a*P + b*Q with a point and a scalar of the item's own for both terms, and Chaum-Pedersen proofs of correct ElGamal
 * decryption built on it (extension of bjj_hip.h, same library).
 *
 * A trustee's partial decryption D = sk * C1 (bjj_mul_common) is accepted only with a proof that it was made with the key behind
 * PK = sk * G: a proof of discrete-log equality log_G PK = log_C1 D.  The proof of one item is (A, B, z):
 *       prover      w random,  A = w * G,  B = w * C1,  c = H(tag, C1, D, A, B),  z = w + c * sk  (mod l)
 *       verifier    c = H(tag, C1, D, A, B),  z * G == A + c * PK  and  z * C1 == B + c * D
 *       H           c = Poseidon5(Poseidon5(tag, C1.x, C1.y, D.x, D.y), A.x, A.y, B.x, B.y), the bjj_poseidon5 permutation (t = 6),
 *                   taken as an integer below r
 * The primitive underneath is general and has an entry of its own, bjj_mul_pair: one joint windowed loop that shares the doublings of
 * the two multiplications.
 *
 * bjj_mul_pair.  For every item, with A = add_xy[i] (the identity (0, 1) when add_xy is NULL):
 *       out_xy[i] = A + a[i] * P[i] + b[i] * Q[i]          ok[i] = BJJ_DLEQ_OK
 *     as canonical affine bytes: byte for byte bjj_point_add(bjj_point_add(A, bjj_mul_var_base(P, a)), bjj_mul_var_base(Q, b)) for
 *     every P, Q, A ON the curve -- points of order 1, 2, 4, 8 and points outside the prime-order subgroup included: the curve's
 *     addition law is complete and the canonical affine coordinates of a point are unique (the argument of bjj_hip_common_scalar.h).
 *     a and b are n*32 little-endian bytes of ANY 256-bit value, reduced mod 8l (the group order).  Coordinates >= r are reduced mod r.
 *     A P, Q or A that fails the curve equation -- this includes (0, 0), the error output of the other calls -- gives
 *       ok[i] = BJJ_DLEQ_OFF_CURVE       out_xy[i] = (0, 0)
 *     and disturbs no other item.  (bjj_mul_var_base replays the reference's formulas for such a point; this call refuses it.)
 *     One launch: two per-lane tables, 64 joint windows, A as one mixed addition, one inversion pass.
 *
 * bjj_dleq_verify.  g: the table of G, NULL = the context's B8 table; pk: the table of PK (bjj_base_create), required.  tag: 32
 *     little-endian bytes on the HOST, any value, reduced mod r.  Per item C1, D, A, B (64 bytes each) and z (32 bytes); ok[i] is
 *       BJJ_DLEQ_OFF_CURVE (2)   C1 or D fails the curve equation (coordinates >= r are reduced first, as everywhere else)
 *       BJJ_DLEQ_REJECT (0)      otherwise, when a coordinate of A or B is >= r or z >= l: the fields of a PROOF must be canonical --
 *                                this rule is stricter than the rest of the library, and it makes a proof's encoding unique
 *       BJJ_DLEQ_OK (1)          otherwise, exactly when z * G == A + c * PK and z * C1 == B + c * D hold as curve points (which
 *                                requires A and B to be on the curve); BJJ_DLEQ_REJECT when they do not
 *     One launch per call: two permutations, one walk over the tables of G and PK, one joint loop over the per-lane tables of C1 and
 *     -D, two projective comparisons.  No inversion, no point output.
 *   What the transcript binds.  G and PK enter the hash ONLY through tag: derive it from them (the Python binding's Context.dleq_tag
 *     is Poseidon5(G.x, G.y, PK.x, PK.y, label)) or from a session value that fixes them.  A verifier who accepts a tag that does not
 *     bind PK accepts proofs made for another key's table.
 *   Subgroup.  Soundness needs C1 and D in the prime-order subgroup: check them with bjj_in_subgroup.  This call does NOT: a D that is
 *     off by the point of order 2 passes whenever c is even (c * T2 is the identity), and the tests pin exactly that behaviour.
 *
 * bjj_dleq_prove.  g as above; sk and tag: 32 bytes each on the HOST, any value; w: n*32 bytes, the caller's nonces, any value -- fresh,
 *     uniform and secret per item, or sk leaks.  With sk' = sk mod l and w' = w mod l, for every item with C1 on the curve
 *       d_xy[i] = sk' * C1    a_xy[i] = w' * G    b_xy[i] = w' * C1    z[i] = (w' + (c mod l) * sk') mod l    ok[i] = BJJ_DLEQ_OK
 *     each point as canonical affine bytes, d_xy byte for byte bjj_mul_common(sk', C1).  A C1 that fails the curve equation gives
 *     ok[i] = BJJ_DLEQ_OFF_CURVE with d_xy[i] = a_xy[i] = b_xy[i] = (0, 0) and z[i] = 0.
 *     A chain of five launches on one stream without a synchronisation in between: w' (into z), D, A, B with the launchers of
 *     bjj_mul_common, bjj_mul_bases and bjj_mul_var_base, then the hash and z.
 *
 * Arguments.  n == 0 is BJJ_OK and touches nothing.  A NULL ctx is BJJ_E_INVALID and is answered before any device is touched; a NULL
 *     pk (a missing key is not B8), a handle of another context or a freed one, a NULL sk or tag, and a NULL array with n > 0 (add_xy
 *     alone may be NULL) are BJJ_E_INVALID.  ok is required by all three.  A rejected call writes nothing.
 * Host forms.  Synchronous and single-launch (bjj_dleq_prove: one chain): one copy in per array given, the launches, one copy out per
 *     output array.  Pinned and pageable memory give identical results.  There is no chunked pipeline.
 * _dev forms.  The *_dev contract of bjj_hip.h: every array except d_ok 16-byte aligned (d_ok: any address), enqueued on `stream`
 *     (NULL = the context's stream), no synchronisation; one scratch set per stream.  Arrays of a call must not overlap.
 * NOT CONSTANT TIME, like bjj_mul_common: the per-lane table reads of bjj_mul_pair and bjj_dleq_prove depend on the digits of a, b,
 *     w and sk, and the fixed-base table reads on those of w.  These calls do not look at bjj_set_signer_constant_time.  Do not use them
 *     where the memory access pattern of a call is visible to a party that must not learn a scalar.  (bjj_dleq_verify handles public
 *     values only.) */
#ifndef BJJ_HIP_DLEQ_H
#define BJJ_HIP_DLEQ_H

#include "bjj_hip.h"
#include "bjj_hip_bases.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BJJ_DLEQ_REJECT    0
#define BJJ_DLEQ_OK        1
#define BJJ_DLEQ_OFF_CURVE 2

int bjj_mul_pair(bjj_ctx* ctx, const uint8_t* p_xy /* n*64 */, const uint8_t* a /* n*32 */, const uint8_t* q_xy /* n*64 */,
                 const uint8_t* b /* n*32 */, const uint8_t* add_xy /* n*64, or NULL = the identity */, size_t n, uint8_t* out_xy /* n*64 */,
                 uint8_t* ok /* n */);
int bjj_mul_pair_dev(bjj_ctx* ctx, const void* d_p_xy, const void* d_a, const void* d_q_xy, const void* d_b, const void* d_add_xy, size_t n,
                     void* d_out_xy, void* d_ok, void* stream);

int bjj_dleq_verify(bjj_ctx* ctx, const bjj_base* g /* NULL = B8 */, const bjj_base* pk, const uint8_t* tag /* 32, host */,
                    const uint8_t* c1_xy, const uint8_t* d_xy, const uint8_t* a_xy, const uint8_t* b_xy /* n*64 each */,
                    const uint8_t* z /* n*32 */, size_t n, uint8_t* ok /* n */);
int bjj_dleq_verify_dev(bjj_ctx* ctx, const bjj_base* g /* NULL = B8 */, const bjj_base* pk, const uint8_t* tag /* 32, host */,
                        const void* d_c1_xy, const void* d_d_xy, const void* d_a_xy, const void* d_b_xy, const void* d_z, size_t n,
                        void* d_ok, void* stream);

int bjj_dleq_prove(bjj_ctx* ctx, const bjj_base* g /* NULL = B8 */, const uint8_t* sk /* 32, host */, const uint8_t* tag /* 32, host */,
                   const uint8_t* c1_xy /* n*64 */, const uint8_t* w /* n*32 */, size_t n, uint8_t* d_xy, uint8_t* a_xy,
                   uint8_t* b_xy /* n*64 each */, uint8_t* z /* n*32 */, uint8_t* ok /* n */);
int bjj_dleq_prove_dev(bjj_ctx* ctx, const bjj_base* g /* NULL = B8 */, const uint8_t* sk /* 32, host */, const uint8_t* tag /* 32, host */,
                       const void* d_c1_xy, const void* d_w, size_t n, void* d_d_xy, void* d_a_xy, void* d_b_xy, void* d_z, void* d_ok,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
