/* gbp_mi355x_seed.h — landmark and keyframe seeding of libgbp_mi355x_seed.so: a start for the solver from what a front end has,
 * observations and rough camera poses, computed where the state already is.
 *
 *   gbp_seed_index       HOST: the landmark-major index of a graph (each landmark's edges, in file order)
 *   gbp_seed_landmarks   per landmark: multi-view triangulation, prior mean and prior strength, a status word
 *   gbp_seed_keyframe    the new keyframe's prior eta from the previous camera's belief: the device twin of gbp_slam_initialise_new_kf
 *
 * A library of its own, next to the program list of gbp_mi355x.h and the readout of gbp_mi355x_post.h, and without a ctx: its inputs
 * are the file-order arrays a caller already holds (gbp_problem's cam_id / lmk_id, the arrays gbp_read and gbp_read_priors fill).
 * Stateless: no allocation, no synchronisation, nothing is launched anywhere but on the stream the caller passes (a hipStream_t;
 * 0 = the default stream), so the results are valid for work queued behind the call on that stream.  The one piece of scratch, a
 * record per camera, is a device workspace the caller provides (gbp_seed_workspace_bytes).
 *
 * Every array pointer of gbp_seed_landmarks and gbp_seed_keyframe is DEVICE memory on the current device, except K and the options;
 * every array of gbp_seed_index and gbp_seed_check_index is HOST memory.  Every argument is checked before the first HIP call: a bad
 * one returns GBP_ERR_INVALID and names the argument in gbp_seed_last_error(), with or without a GPU in the machine.  Return codes are
 * the gbp_status values of gbp_mi355x.h; no C++ exception crosses this ABI.
 *
 * What gbp_seed_landmarks computes, per landmark l with select[l] != 0 (select NULL: every landmark), over its USED observations: the
 * edges lmk_edges[lmk_start[l] .. lmk_start[l + 1]) with active_flag == 1 (active_flag NULL: all of them), in that order — file order
 * when the index is gbp_seed_index's.  Every sum below is accumulated serially from zero in that order, in fp32 unless stated, without
 * FMA contraction and without atomics: the result is a function of the inputs alone, not of the launch.
 *   rays        R = the metric's rotation of the camera mean (gbp_eval's: eigenso3exp), t = its translation, centre o = -R^T t,
 *               direction d = R^T ((u - K[2]) / K[0], (v - K[5]) / K[4], 1), normalised.  (The pin-hole entries jac_hfunc reads.)
 *   parallax    1 - |mean of the unit rays|^2: sin^2 of half the angle for two views.  Below min_parallax the views do not fix a depth.
 *   start       the midpoint method: A = sum (I - d d^T), b = sum (I - d d^T) o, x0 = A^-1 b by the fp64 partial-pivot solve of the
 *               metric on the fp32 sums.
 *   refinement  refine_iters Gauss-Newton steps on sum |z - pi(R x + t)|^2 over x alone: r = the metric's residual, J = the landmark
 *               block of the linearisation's Jacobian (jac_hfunc) at x, (sum J^T J) dx = sum J^T r by the same solve, x += dx.  A step
 *               with a non-finite entry is not taken, and ends the refinement.
 *   placement   where the views do not give a point (one view, low parallax, a non-finite result): x = o + fallback_depth R^T (the
 *               normalised pixel, 1) of the FIRST used view: camera-frame depth fallback_depth ALONG THE OBSERVATION'S RAY.
 *   prior       the rule of gbp_set_prior_lambda at the seeded point: peak = the largest |entry| of its 2 x 9 reprojection Jacobian
 *               (the reference's reprojectionJacFn, the same operations) over the used observations,
 *               lam = (float)((double)peak^2 / reproj_meas_var), Lambda = lam I, eta = mean lam.
 * Status word (GBP_SEED_*): bit 0 no used view — mean and prior of the landmark are NOT touched (status and n_views are written);
 * bit 1 one used view, placed; bit 2 parallax below min_parallax (two edges of one camera land here), placed from the first used view;
 * bit 3 the point has a non-positive camera-frame depth in a used view (evaluated at the point that is written; the point is kept);
 * bit 4 an output was not finite: the point was replaced by the placement, and what is written may still be non-finite when the
 * first used view's camera is; bit 5 an index entry was out of range (an edge >= n_edges, a camera >= n_cams, a range of lmk_start
 * that is reversed or ends past n_edges): those entries are skipped.  A bad block never faults; it gives a flagged result.
 * A landmark with select[l] == 0 has NONE of its outputs touched, the status word included, so the call can write in place into the
 * arrays gbp_read_priors filled.
 */
#ifndef GBP_MI355X_SEED_H
#define GBP_MI355X_SEED_H

#include <stddef.h>

#include "gbp_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GBP_SEED_ABI_VERSION 1

#define GBP_SEED_NO_VIEW 1u
#define GBP_SEED_ONE_VIEW 2u
#define GBP_SEED_LOW_PARALLAX 4u
#define GBP_SEED_BEHIND 8u
#define GBP_SEED_NONFINITE 16u
#define GBP_SEED_BAD_INDEX 32u

typedef struct gbp_seed_options {
  float min_parallax;     /* default 5e-3: two rays less than 8.1 degrees apart (sin^2 of half the angle).  The angle between the rays has
                             to dominate the error of the camera rotations they are built from: rough poses are off by a degree or so.
                             Measured on the shipped sequences at their file cameras (profiles/seed_landmarks.md): at 1e-4 a third of
                             fr2robot2's triangulated points (74 of 219) lie behind a camera and its keyframe-by-keyframe run
                             diverges; at 1e-3 fr1xyz's bundle adjustment has a non-positive-definite belief after 50 passes; at 5e-3
                             and 2e-2 every measured run stays healthy.  The price: fr2robot2's views are so close together that at
                             5e-3 all its landmarks are placed, none triangulated, and its run without the file's points ends at
                             1.30 px where the file-initialised one ends at 0.87 px.  The fp32 noise of the measure is about 1e-7:
                             duplicate edges of one camera are far below any sensible value. */
  float fallback_depth;   /* default 1: the reference's loc_cam_frame depth (av_depth_init), here along the observation's ray */
  uint32_t refine_iters;  /* default 2: Gauss-Newton steps from the midpoint start; each costs one pass over the landmark's observations
                             with a linearisation (jac_hfunc) per observation */
  float reproj_meas_var;  /* default 4: the CLIs' --reproj_meas_var, the variance of gbp_set_prior_lambda */
} gbp_seed_options;

GBP_API int gbp_seed_abi_version(void);
GBP_API const char* gbp_seed_last_error(void);      /* text of the calling thread's last failed gbp_seed_* call */
GBP_API int gbp_seed_default_options(gbp_seed_options* opts);

/* HOST.  lmk_start [L + 1], lmk_edges [E] out: the edges of landmark l are lmk_edges[lmk_start[l] .. lmk_start[l + 1]), ascending
 * (an O(E) counting sort of lmk_id, stable).  A lmk_id >= n_lmks returns GBP_ERR_INVALID.  n_edges == 0 is legal. */
GBP_API int gbp_seed_index(uint32_t n_lmks, uint32_t n_edges, const uint32_t* lmk_id /*[E]*/, uint32_t* lmk_start /*[L+1]*/,
                           uint32_t* lmk_edges /*[E]*/);
/* HOST.  What gbp_seed_landmarks cannot ask of device memory without waiting for it: lmk_start[0] == 0, ascending,
 * lmk_start[L] == n_edges, every lmk_edges entry < n_edges.  For an index that did not come from gbp_seed_index (the kernel skips
 * and flags bad entries, GBP_SEED_BAD_INDEX, but does not say which). */
GBP_API int gbp_seed_check_index(uint32_t n_lmks, uint32_t n_edges, const uint32_t* lmk_start, const uint32_t* lmk_edges);

/* bytes of the device workspace gbp_seed_landmarks needs for n_cams cameras (64 per camera: R, t, o); its base is 16-byte aligned */
GBP_API size_t gbp_seed_workspace_bytes(uint32_t n_cams);

/* K: the pin-hole matrix, HOST memory, copied into the launch.  opts: HOST, NULL = the defaults.  active_flag, select, lmk_priors_eta,
 * lmk_priors_lambda and n_views may be NULL.  n_lmks == 0 is legal (nothing is launched). */
GBP_API int gbp_seed_landmarks(void* hip_stream, uint32_t n_cams, uint32_t n_lmks, uint32_t n_edges, const uint32_t* cam_id /*[E]*/,
                               const uint32_t* lmk_start /*[L+1]*/, const uint32_t* lmk_edges /*[E]*/, const float K[9],
                               const float* cam_mean /*[6C]*/, const float* measurements /*[2E]*/, const uint32_t* active_flag /*[E]*/,
                               const uint32_t* select /*[L]*/, const gbp_seed_options* opts, void* workspace, float* lmk_mean /*[3L]*/,
                               float* lmk_priors_eta /*[3L]*/, float* lmk_priors_lambda /*[9L]*/, uint32_t* status /*[L]*/,
                               uint32_t* n_views /*[L]*/);

/* mu = solve_pivot<6>(belief of camera src); cam_priors_eta[6 dst + i] = sum_k cam_priors_lambda[36 dst + 6 i + k] mu[k] (fp32, k
 * ascending from zero): bit for bit gbp_slam_initialise_new_kf(src, ...) with dst = src + 1.  cam_mean_out [6] (may be NULL) receives
 * mu: the new camera's pose guess, the reference's copy of the previous keyframe. */
GBP_API int gbp_seed_keyframe(void* hip_stream, uint32_t n_cams, uint32_t src, uint32_t dst, const float* cam_beliefs_eta /*[6C]*/,
                              const float* cam_beliefs_lambda /*[36C]*/, const float* cam_priors_lambda /*[36C]*/,
                              float* cam_priors_eta /*[6C] in/out*/, float* cam_mean_out /*[6]*/);

#ifdef __cplusplus
}
#endif
#endif
