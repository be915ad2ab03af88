/* gbp_mi355x_post.h — the solution readout of libgbp_mi355x_post.so: what a user wants from a finished run, computed where the
 * beliefs already are.
 *
 *   gbp_post_moments     per variable: mean, marginal covariance, a status word
 *   gbp_post_residuals   per observation: reprojection residual at the means, covariance of the reprojection under the beliefs
 *
 * A library of its own, next to the program list of gbp_mi355x.h, and without a ctx: its inputs are exactly the file-order arrays
 * gbp_read fills (eta [6C], Lambda [36C] row-major, eta [3L], Lambda [9L]) — read from a ctx, gathered from shards or loaded from a
 * file alike.  Stateless: no allocation, no synchronisation, nothing is launched anywhere but on the stream the caller passes (a
 * hipStream_t; 0 = the default stream), so the results are valid for work queued behind the call on that stream.
 *
 * EVERY array pointer below is DEVICE memory on the current device, except K.  Every argument is checked before the first HIP call:
 * a bad one returns GBP_ERR_INVALID and names the argument in gbp_post_last_error(), with or without a GPU in the machine.  Return
 * codes are the gbp_status values of gbp_mi355x.h; no C++ exception crosses this ABI.
 *
 * What the numbers are:
 *   mean        Lambda^-1 eta by fp64 elimination with partial pivoting on the fp32 block, rounded to fp32: the operations of the
 *               metric (gbp_eval) and of gbp_belief_means, so bit-identical to both.
 *   covariance  the GENERAL inverse of the fp32 block, column j = the same solve with e_j as right-hand side, bit for bit.  It is NOT
 *               symmetrised: the Lambda of a belief is not bit-symmetric on every path (accumulated camera beliefs differ from
 *               their transpose by up to 3e-3 relative on real sequences), and neither is its inverse.  Row-major [36] / [9].
 *   status      bit 0: some output of the variable (mean or covariance) is not finite; bit 1: the un-pivoted LDL^T of Lambda has a
 *               non-positive pivot.  The same definitions as n_nonfinite / n_nonpd of gbp_eval_out: over a ctx's beliefs the counts
 *               agree with gbp_eval.  A singular block (all zeros, say) gives inf / NaN and bit 0 — never a fault.
 *   residual    z - pi(mean) with the metric's operations: 0.5 (r0^2 + r1^2) and sqrt(r0^2 + r1^2) are the per-factor terms of
 *               gbp_eval_out.sum_half_sq / sum_norm.
 *   reproj_cov  J_c cov_c J_c^T + J_l cov_l J_l^T in fp32, J the linearisation's Jacobian at the means, stored as S00, S01, S11
 *               (S01 is the entry of row 0: the inputs are general matrices).  Belief propagation does not provide the camera-
 *               landmark cross-covariance; that term is NEGLECTED, so this is the gate of a front end, not the exact marginal.
 */
#ifndef GBP_MI355X_POST_H
#define GBP_MI355X_POST_H

#include "gbp_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GBP_POST_ABI_VERSION 1

GBP_API int gbp_post_abi_version(void);
GBP_API const char* gbp_post_last_error(void);      /* text of the calling thread's last failed gbp_post_* call */

/* NULL outputs are skipped.  n_cams == 0 or n_lmks == 0 is legal, and the matching pointers may then be NULL. */
GBP_API int gbp_post_moments(void* hip_stream, uint32_t n_cams, uint32_t n_lmks, const float* cam_eta, const float* cam_lambda,
                             const float* lmk_eta, const float* lmk_lambda, float* cam_mean /*[6C]*/, float* cam_cov /*[36C]*/,
                             float* lmk_mean /*[3L]*/, float* lmk_cov /*[9L]*/, uint32_t* cam_status /*[C]*/, uint32_t* lmk_status /*[L]*/);

/* One result per edge, in file order.  K: the pin-hole matrix, HOST memory, copied into the launch.  active_flag NULL = every edge
 * active; an inactive edge writes zeros to both outputs.  reproj_cov may be NULL; asking for it needs both cam_cov and lmk_cov. */
GBP_API int gbp_post_residuals(void* hip_stream, uint32_t n_cams, uint32_t n_lmks, uint32_t n_edges, const uint32_t* cam_id,
                               const uint32_t* lmk_id, const float K[9], const float* cam_mean, const float* lmk_mean,
                               const float* measurements /*[2E]*/, const uint32_t* active_flag /*[E]*/, const float* cam_cov,
                               const float* lmk_cov, float* residual /*[2E]*/, float* reproj_cov /*[3E]*/);

#ifdef __cplusplus
}
#endif
#endif
