/* gbp_mi355x_locate.h — camera location of libgbp_mi355x_locate.so: the pose of a camera from its observations of landmarks that are
 * already mapped, with NO pose guess and with wrong matches among the observations (relocalisation; the gate in front of
 * gbp_resect_cameras, which needs a start inside its basin and only softens a wrong match).
 *
 *   gbp_locate_cameras   per camera: 64 x rounds three-point hypotheses, each scored by the number of observations that agree with it;
 *                        the pose of the winner, the mask of the observations that agree with that pose, a report, a status word
 *
 * The fifth library, next to gbp_mi355x.h, gbp_mi355x_post.h, gbp_mi355x_seed.h and gbp_mi355x_resect.h, and like the last three without
 * a ctx.  The contract is gbp_mi355x_resect.h's: stateless, no allocation, no synchronisation, nothing is launched anywhere but on the
 * stream the caller passes (a hipStream_t; 0 = the default stream).  Every array pointer is DEVICE memory on the current device, except K
 * and the options.  Every argument is checked before the first HIP call: a bad one returns GBP_ERR_INVALID and names the argument in
 * gbp_locate_last_error(), with or without a GPU in the machine.  Return codes are the gbp_status values of gbp_mi355x.h; no C++
 * exception crosses this ABI.  The index (cam_start, cam_edges) is gbp_resect_index's.
 *
 * THE DEFINITION.  Per camera c with select[c] != 0 (select NULL: every camera), index range [k0, k1) = [cam_start[c], cam_start[c + 1])
 * and deg = k1 - k0.  USED observations, the clamping of a bad range and the skipping of a bad entry (GBP_LOCATE_BAD_INDEX) are exactly
 * gbp_resect_cameras's.  cam_mean is never read.
 *
 * 1 count     n_views = the number of used observations.  0: GBP_LOCATE_NO_VIEW; below min_inliers: GBP_LOCATE_FEW_VIEWS.
 * 2 sampling  mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16  (uint32, wrapping).
 *             Hypothesis (round r < rounds, lane j < 64) has h = mix(mix(seed + c) + 64 r + j).  Slot s = 0, 1, 2 tries t = 0 .. 7:
 *             u = mix(h + 8 s + t), entry k0 + ((uint64(u) * deg) >> 32); the slot takes the first try whose entry is used and whose
 *             landmark index differs from the earlier slots'.  A slot without such a try voids the hypothesis.
 * 3 solver    fp64, + - x / and sqrt only, no FMA contraction.  Bearing of a pixel (u, v): (a, b, 1) / sqrt(a a + b b + 1) with
 *             a = (u - K[2]) / K[0], b = (v - K[5]) / K[4].  Points X1..3 (the landmark means), bearings y1..3, unknown depths L1..3 with
 *             Li yi = R Xi + t.  (Persson and Nordberg, "Lambda Twist: an accurate fast robust perspective three point solver", ECCV
 *             2018, for the formulation; the degenerate member is split without its eigenvectors.)
 *             a. F1 = X2 - X1, F2 = X3 - X1, F3 = F1 x F2.  No solution unless |F3|^2 > 1e-10 |F1|^2 |F2|^2 (repeated or collinear
 *                points; a NaN fails the comparison).  a_ij = |Xi - Xj|^2 / (sum of the three), b_ij = yi . yj.
 *             b. Li^2 + Lj^2 - 2 b_ij Li Lj = a_ij (times the sum) are three quadrics M_ij.  D1 = a23 M12 - a12 M23 and
 *                D2 = a23 M13 - a13 M23 vanish at the depths.  det(D1 + g D2) = c0 + c1 g + c2 g^2 + c3 g^3 with c0 = det D1, c3 = det D2,
 *                c1 = trace(adj(D1) D2), c2 = trace(adj(D2) D1).  If |c3| >= |c0|: (A, B) = (D1, D2), else (D2, D1) and the coefficients
 *                reversed: the cubic is made monic by the larger determinant (zero: no solution).
 *             c. Its root: x = y - b / 3 gives y^3 + p y + q; the root y >= 0 of y^3 + p y - |q| from the start
 *                2 max(sqrt|p|, s), s = |q|^(1/4) if |q| <= 1 else |q|^(1/2) (an upper bound of every root, on the convex side, so
 *                Newton descends monotonically), 40 Newton steps y -= g(y) / g'(y) (a step with g' <= 0 is left out); the sign of q
 *                gives the sign of y back.  40: from that start the distance to the root shrinks by 2/3 a step until the quadratic
 *                phase, so a start 1e4 times the root needs 23 steps to get there and the rest squares the error; with 40 the CPU
 *                tests' solutions reproject their own three points to 2e-12 px at worst over all their families (near identity, near
 *                pi, 1 000 scene units, nearly collinear), and differ from a float64 numpy solver by 3e-9 at most.
 *             d. D0 = A + g B is two planes l, m through the origin: D0 = l m^T + m l^T, adj(D0) = -(l x m)(l x m)^T.  i = the index of
 *                the most negative diagonal entry of adj(D0) (first on ties; none negative: no solution), p = column i of adj(D0) /
 *                sqrt(-adj(D0)_ii), C = D0 + [p]x; (r, c) = the entry of C largest in magnitude (first in row-major order): the planes
 *                are row r and column c of C.
 *             e. Per plane n (row first): k = the index of the largest |n_k| (first), the depth k expressed by the other two, which
 *                leaves a quadratic qa tau^2 + 2 qb tau + qc of the quadric B if |g| <= 1, else A, in the ratio tau of the other two;
 *                negative discriminant: none; q = -(qb + sign(qb) sqrt(disc)), tau = q / qa, then qc / q.  The depths are scaled so
 *                that the three quadrics sum to the sum of the squared distances.  A solution needs three depths > 0.
 *             f. R = (E1 E2 E3)(F1 F2 F3)^-1 with E1 = L2 y2 - L1 y1, E2 = L3 y3 - L1 y1, E3 = E1 x E2 (the inverse by rows F2 x F3,
 *                F3 x F1, F3, over |F3|^2), t = L1 y1 - R X1.  A non-finite entry: no solution.  Solutions are numbered in the order
 *                plane, tau.  R and t are rounded to fp32: the CANDIDATE.
 * 4 scoring   fp32, no FMA contraction.  yc_i = ((R_i0 X0 + R_i1 X1) + R_i2 X2) + t_i; an observation (u, v) AGREES when it is used,
 *             yc_2 > 0 and du du + dv dv <= inlier_px inlier_px with du = u - (K[0] (yc_0 / yc_2) + K[2]), dv = v - (K[4] (yc_1 / yc_2)
 *             + K[5]).  The score of a candidate is the count over all used observations of the camera.  The winner is the largest
 *             count; ties go to the lowest r, then j, then solution number.  Counts are integers: the launch shape cannot matter.
 *             No candidate at all: GBP_LOCATE_NO_HYPOTHESIS.
 * 5 pose      fp64 from the winner's fp32 R: the quaternion by the largest of trace, R00, R11, R22 (Shepperd), made w >= 0 and unit;
 *             theta = 2 atan2(|v|, w) in [0, pi], with atan2 of two non-negative numbers as atan(min / max) (pi/2 - . if |v| > w),
 *             atan t = pi/4 + atan((t - 1) / (t + 1)) above sqrt(2) - 1, and the Taylor polynomial through x^25 below (truncation
 *             under 2e-12 rad: far below fp32, and gbp_resect_cameras polishes).  The rotation vector is v theta / |v|; a rotation below
 *             1e-4 rad is returned with length 1e-4 (along v, or along x if v is zero): the solver's Jacobian divides by |w|^2.  The
 *             pose (t, w) is rounded to fp32.
 * 6 final     at that fp32 pose, the solver's own prediction: cl = cam_lin(w), hx = jac_hfunc_lin(pose, X, K, cl), depth as
 *             gbp_resect_cameras computes it; an observation is an INLIER when it is used, depth > 0 and r0 r0 + r1 r1 <=
 *             inlier_px inlier_px (r = z - hx, fp32).  n_inliers counts them; below min_inliers: GBP_LOCATE_FEW_INLIERS.  The sum of
 *             the inliers' r0 r0 + r1 r1 is taken in gbp_resect_cameras's order (64 serial partials, the halving tree).
 *
 * WHAT IS WRITTEN.  select[c] == 0: nothing.  NO_VIEW, FEW_VIEWS, NO_HYPOTHESIS: status and n_views.  FEW_INLIERS: and n_inliers.
 * Otherwise the camera is LOCATED: also cam_mean [6c ..], inlier[e] = 1 or 0 for every used observation of the camera (nothing else
 * of `inlier`), report [4c ..] = {64 r + j of the winner, its solution number, candidates scored, sum / n_inliers}.  A landmark with a
 * NaN mean yields no solution where it is sampled and agrees with nothing: it sets no bit, its observation gets inlier 0.
 */
#ifndef GBP_MI355X_LOCATE_H
#define GBP_MI355X_LOCATE_H

#include <stddef.h>

#include "gbp_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GBP_LOCATE_ABI_VERSION 1

/* the shared bits have gbp_mi355x_resect.h's values */
#define GBP_LOCATE_NO_VIEW 1u
#define GBP_LOCATE_BAD_INDEX 32u
#define GBP_LOCATE_FEW_VIEWS 64u
#define GBP_LOCATE_FEW_INLIERS 256u
#define GBP_LOCATE_NO_HYPOTHESIS 512u

typedef struct gbp_locate_options {
  uint32_t rounds;       /* default 4.  One round is 64 hypotheses.  A hypothesis is all-inlier with probability w^3 at an inlier share
                            w, so none of 64 rounds is with (1 - w^3)^(64 rounds): at w = 0.3 that is 0.174, 0.030, 0.00091 for 1, 2, 4
                            rounds: 4 is the smallest power of two that stays below 1e-3.  0 is refused, and so is more than 4 096: a camera's
                            rounds run one after the other in one wavefront (2 ms a round at 1 000 views), 4 096 rounds already leave
                            (1 - w^3)^(64 rounds) below 1e-3 down to w = 0.03, and 64 r + j stays exact in report's float. */
  float inlier_px;       /* default 5: the solver's own robust threshold, gbp_resect_options.huber_px.  Positive and finite. */
  uint32_t min_inliers;  /* default 6: the three sampled points plus as many again, gbp_resect_options.min_views.  Below 4 is refused. */
  uint32_t seed;         /* default 0 */
} gbp_locate_options;

GBP_API int gbp_locate_abi_version(void);
GBP_API const char* gbp_locate_last_error(void);      /* text of the calling thread's last failed gbp_locate_* call */
GBP_API int gbp_locate_default_options(gbp_locate_options* opts);

/* cam_edges NULL: entry k of the index is edge k.  K: the pin-hole matrix, HOST memory, copied into the launch.  opts: HOST, NULL = the
 * defaults.  n_cams == 0 is legal (nothing is launched). */
GBP_API int gbp_locate_cameras(void* hip_stream, uint32_t n_cams, uint32_t n_lmks, uint32_t n_edges, const uint32_t* lmk_id /*[E]*/,
                               const uint32_t* cam_start /*[C+1]*/, const uint32_t* cam_edges /*[E]; NULL = identity*/,
                               const float K[9] /*host*/, const float* lmk_mean /*[3L]*/, const float* measurements /*[2E]*/,
                               const uint32_t* active_flag /*[E]; NULL = all*/, const uint32_t* lmk_use /*[L]; NULL = all*/,
                               const uint32_t* select /*[C]; NULL = every camera*/, const gbp_locate_options* opts /*host; NULL = defaults*/,
                               float* cam_mean /*[6C] out only*/, uint32_t* inlier /*[E] or NULL*/, float* report /*[4C] or NULL*/,
                               uint32_t* status /*[C]*/, uint32_t* n_views /*[C] or NULL*/, uint32_t* n_inliers /*[C] or NULL*/);

#ifdef __cplusplus
}
#endif
#endif
