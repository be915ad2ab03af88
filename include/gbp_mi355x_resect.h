/* gbp_mi355x_resect.h — camera resection of libgbp_mi355x_resect.so: the pose of a camera from its observations of landmarks that are
 * already mapped (tracking, motion-only bundle adjustment), computed where the map already is.
 *
 *   gbp_resect_index     HOST: the camera-major index of a graph (each camera's edges, in file order)
 *   gbp_resect_cameras   per camera: Levenberg-Marquardt over the six pose parameters against fixed landmarks, the prior eta at the
 *                        result, an information matrix, a report, a status word
 *
 * The fourth library, next to gbp_mi355x.h, gbp_mi355x_post.h and gbp_mi355x_seed.h, and like the last two without a ctx: its inputs
 * are the file-order arrays a caller already holds.  Stateless: no allocation, no synchronisation, nothing is launched anywhere but on
 * the stream the caller passes (a hipStream_t; 0 = the default stream), so the results are valid for work queued behind the call on
 * that stream.  Every array pointer of gbp_resect_cameras is DEVICE memory on the current device, except K and the options; every
 * array of gbp_resect_index and gbp_resect_check_index is HOST memory.  Every argument is checked before the first HIP call: a bad one
 * returns GBP_ERR_INVALID and names the argument in gbp_resect_last_error(), with or without a GPU in the machine.  Return codes are
 * the gbp_status values of gbp_mi355x.h; no C++ exception crosses this ABI.
 *
 * THE DEFINITION.  Per camera c with select[c] != 0 (select NULL: every camera).  Its USED observations are the index entries k in
 * [cam_start[c], cam_start[c + 1]) whose edge e = cam_edges[k] (cam_edges NULL: e = k) passes all of: e < n_edges;
 * active_flag[e] == 1 (NULL: all); l = lmk_id[e] < n_lmks; lmk_use[l] != 0 (NULL: all).  An entry with e or l out of range, or a range
 * of cam_start that is reversed or ends past n_edges (it is clamped), is skipped and sets GBP_RESECT_BAD_INDEX: a bad block never faults.
 *
 *   pass(x)   cl = cam_lin(x[3..5]) once (the solver's camera-only linearisation terms).  Per used observation:
 *             jac_hfunc_lin(x, lmk_mean[l], K, cl) — the solver's own linearisation — gives J = Jkf (2 x 6) and the prediction hx;
 *             r = (z0 - hx0, z1 - hx1); err = sqrtf(r0 r0 + r1 r1);
 *             plain = huber_px <= 0 or err <= huber_px;   w = plain ? 1 : huber_px / err;
 *             rho = plain ? 0.5f (err err) : huber_px (err - 0.5f huber_px);
 *             cost += rho;  H_ij += w (J0i J0j + J1i J1j) for i <= j (21 entries);  g_i += w (J0i r0 + J1i r1);  n += 1.
 *             All fp32, no FMA contraction, no atomics.
 *   order     Partial j (j = 0 .. 63) accumulates serially from zero the entries k0 + j, k0 + j + 64, ...  The 64 partials are combined
 *             by the halving tree: for s = 32, 16, 8, 4, 2, 1: partial i += partial i + s, for i < s.  The result is a function of the
 *             inputs alone, not of the launch.
 *   LM        Levenberg-Marquardt with a fixed pass budget and no tolerance:
 *               (cost, H, g) = pass(x); passes = 1; lam = lambda0
 *               while passes < max_passes and lam <= 1e8:
 *                 A = H (full, symmetric) with A_ii = H_ii (1 + lam)                       (fp32)
 *                 dx = solve_pivot<6>(A, g)                                                (the metric's fp64 partial-pivot solve)
 *                 if dx is not finite: lam *= 10; continue
 *                 (cost', H', g') = pass(x + dx); passes += 1
 *                 if x + dx and every sum are finite and cost' < cost: accept (x, cost, H, g; last_step = max |dx_i|);
 *                                                                       lam = max(lam / 10, 1e-9)
 *                 else: lam *= 10
 *             Whether the result is good enough is the caller's decision, from `report`.
 *
 * WHAT IS WRITTEN.  select[c] == 0: nothing, the status word included.  n == 0 (GBP_RESECT_NO_VIEW), n < min_views
 * (GBP_RESECT_FEW_VIEWS) or a first pass with a non-finite sum (GBP_RESECT_NONFINITE): only status and n_views.  A rotation vector of
 * EXACTLY ZERO lands in the last case: the solver's Jacobian divides by |w|^2 (start such a camera a hair off zero).  A NaN in a used
 * landmark or in the start pose does too.  Otherwise:
 *   cam_mean [6c ..]        the accepted pose; if no step was accepted, the start pose's own bits, and GBP_RESECT_STALLED is set
 *   cam_info [36c ..]       the accepted H as a full symmetric 6 x 6, every entry divided by reproj_meas_var.  THE LANDMARKS ARE HELD
 *                           FIXED: this is the information of the pose given a perfectly known map, and overstates what is known.
 *   report [4c ..]          {start cost, final cost, last accepted step (0 if none), final lam}
 *   cam_priors_eta [6c + i] sum_k cam_priors_lambda[36c + 6i + k] mean[k], fp32, k ascending from zero: the row dots of
 *                           gbp_seed_keyframe with the resected pose.  cam_priors_lambda is only read.
 * Status word: the values of GBP_SEED_* where the meaning is shared.  GBP_RESECT_BEHIND: the camera-frame depth of a used landmark is
 * <= 0 at the accepted pose (the operations of jac_hfunc_lin's yc[2]); the result is written all the same.
 */
#ifndef GBP_MI355X_RESECT_H
#define GBP_MI355X_RESECT_H

#include <stddef.h>

#include "gbp_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GBP_RESECT_ABI_VERSION 1

#define GBP_RESECT_NO_VIEW 1u
#define GBP_RESECT_BEHIND 8u
#define GBP_RESECT_NONFINITE 16u
#define GBP_RESECT_BAD_INDEX 32u
#define GBP_RESECT_FEW_VIEWS 64u
#define GBP_RESECT_STALLED 128u

typedef struct gbp_resect_options {
  uint32_t max_passes;    /* default 10: twice the 5 passes a float64 prototype needed from starts up to 0.5 and 20 degrees away
                             (profiles/resect_cameras.md has what the kernel needs on the shipped sequences).  0 is refused. */
  uint32_t min_views;     /* default 6: three points fix a pose only up to four solutions, so twice three.  Below 3 is refused. */
  float huber_px;         /* default 5: the solver's own robust threshold, nstds sqrt(reproj_meas_var) = 2.5 * 2.  <= 0: plain least
                             squares.  NaN is refused. */
  float lambda0;          /* default 1e-3: a conventional Marquardt starting value, not a tuned one.  Positive. */
  float reproj_meas_var;  /* default 4: the solver's default; only cam_info depends on it.  Positive. */
} gbp_resect_options;

GBP_API int gbp_resect_abi_version(void);
GBP_API const char* gbp_resect_last_error(void);      /* text of the calling thread's last failed gbp_resect_* call */
GBP_API int gbp_resect_default_options(gbp_resect_options* opts);

/* HOST.  cam_start [C + 1], cam_edges [E] out: the edges of camera c are cam_edges[cam_start[c] .. cam_start[c + 1]), ascending (an
 * O(E) counting sort of cam_id, stable).  A cam_id >= n_cams returns GBP_ERR_INVALID.  n_edges == 0 is legal. */
GBP_API int gbp_resect_index(uint32_t n_cams, uint32_t n_edges, const uint32_t* cam_id /*[E]*/, uint32_t* cam_start /*[C+1]*/,
                             uint32_t* cam_edges /*[E]*/);
/* HOST.  cam_start[0] == 0, ascending, cam_start[C] == n_edges, every cam_edges entry < n_edges.  cam_edges may be NULL (the identity). */
GBP_API int gbp_resect_check_index(uint32_t n_cams, uint32_t n_edges, const uint32_t* cam_start, const uint32_t* cam_edges);

/* cam_edges NULL: entry k of the index is edge k — a file in the reference's format is sorted by camera, so cam_start alone is its
 * index.  K: the pin-hole matrix, HOST memory, copied into the launch.  opts: HOST, NULL = the defaults.  n_cams == 0 is legal
 * (nothing is launched).  cam_priors_eta needs cam_priors_lambda. */
GBP_API int gbp_resect_cameras(void* hip_stream, uint32_t n_cams, uint32_t n_lmks, uint32_t n_edges, const uint32_t* lmk_id /*[E]*/,
                               const uint32_t* cam_start /*[C+1]*/, const uint32_t* cam_edges /*[E]; NULL = identity*/,
                               const float K[9] /*host*/, const float* lmk_mean /*[3L]*/, const float* measurements /*[2E]*/,
                               const uint32_t* active_flag /*[E]; NULL = all*/, const uint32_t* lmk_use /*[L]; NULL = all*/,
                               const uint32_t* select /*[C]; NULL = every camera*/, const gbp_resect_options* opts /*host; NULL = defaults*/,
                               float* cam_mean /*[6C] in/out: start pose -> result*/, const float* cam_priors_lambda /*[36C] or NULL*/,
                               float* cam_priors_eta /*[6C] or NULL, needs the lambda*/, float* cam_info /*[36C] or NULL*/,
                               float* report /*[4C] or NULL*/, uint32_t* status /*[C]*/, uint32_t* n_views /*[C] or NULL*/);

#ifdef __cplusplus
}
#endif
#endif
