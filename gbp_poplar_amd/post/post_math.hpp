// post/post_math.hpp — the solution readout's arithmetic, per variable and per observation: means and marginal covariances of the
// beliefs, reprojection residuals, reprojection covariances.  One header for both sides: the kernels of gbp_post.hip call these
// routines with one lane per variable / per edge, a plain C++ translation unit (tests/sanitize/post_math_main.cpp) calls them in a
// loop — GBP_DEV is then an ordinary inline function.  Nothing is restated here: the pivot solve, the health check, the rotation and
// the residual are the metric's (csrc/kernels/gbp_metric_math.hpp), the Jacobian is the sweep's (csrc/gbp_device_math.hpp).
#pragma once
#include "../csrc/kernels/gbp_metric_math.hpp"

namespace gbp {
namespace post {
using namespace gbpdev;

constexpr uint32_t kStatusNonFinite = 1u;      // some output of the variable (mean or covariance) is not finite
constexpr uint32_t kStatusNonPD = 2u;          // !ldl_pivots_positive<N>(Lambda): the definition of gbp_eval_out.n_nonpd

// Mean and covariance of one belief (eta [N], Lambda [N x N] row-major, fp32):
//   mean       = solve_pivot<N>(Lambda, eta)
//   cov[:, j]  = solve_pivot<N>(Lambda, e_j)            (the general inverse: NOT symmetrised)
// bit for bit, from ONE elimination: the pivot choice and the multipliers depend on Lambda alone and the N + 1 right-hand sides
// never meet, so every column sees exactly the fp64 operations solve_pivot applies to it, the back-substitution through the
// fp32-rounded x[j] included.  Compile-time bounds and selects for the row swaps, as there: the N x (2N + 1) tableau stays in registers.
// A singular Lambda divides by a zero pivot: inf / NaN outputs, kStatusNonFinite, no fault.
template <int N>
GBP_DEV uint32_t moments(const float* lam, const float* eta, float (&mean)[N], float (&cov)[N * N]) {
  constexpr int W = 2 * N + 1;
  double M[N][W];
  GBP_UNROLL
  for (int i = 0; i < N; ++i) {
    GBP_UNROLL
    for (int j = 0; j < N; ++j) M[i][j] = lam[i * N + j];
    M[i][N] = eta[i];
    GBP_UNROLL
    for (int j = 0; j < N; ++j) M[i][N + 1 + j] = (float)(i == j ? 1.f : 0.f);
  }
  GBP_UNROLL
  for (int k = 0; k < N; ++k) {
    int piv = k;
    double best = fabs(M[k][k]);
    GBP_UNROLL
    for (int i = k + 1; i < N; ++i)
      if (fabs(M[i][k]) > best) { best = fabs(M[i][k]); piv = i; }
    GBP_UNROLL
    for (int i = k + 1; i < N; ++i) {      // swap rows k and piv (at most one i matches)
      const bool sw = piv == i;
      GBP_UNROLL
      for (int j = 0; j < W; ++j) {
        const double t = M[k][j];
        M[k][j] = sw ? M[i][j] : t;
        M[i][j] = sw ? t : M[i][j];
      }
    }
    GBP_UNROLL
    for (int i = k + 1; i < N; ++i) {
      const double f = M[i][k] / M[k][k];
      GBP_UNROLL
      for (int j = k; j < W; ++j) M[i][j] -= f * M[k][j];
    }
  }
  bool finite = true;
  GBP_UNROLL
  for (int c = 0; c <= N; ++c) {           // right-hand side c: eta, then e_0 .. e_{N-1}
    float x[N];
    GBP_UNROLL
    for (int i = N - 1; i >= 0; --i) {
      double s = M[i][N + c];
      GBP_UNROLL
      for (int j = i + 1; j < N; ++j) s -= M[i][j] * (double)x[j];
      x[i] = (float)(s / M[i][i]);
      finite &= (x[i] - x[i] == 0.f);
    }
    GBP_UNROLL
    for (int i = 0; i < N; ++i) {
      if (c == 0) mean[i] = x[i];
      else cov[i * N + (c - 1)] = x[i];
    }
  }
  return (finite ? 0u : kStatusNonFinite) | (ldl_pivots_positive<N>(lam, N) ? 0u : kStatusNonPD);
}

// One observation under the beliefs: residual = z - pi(mean) with the metric's operations (eval_cam_rot + eval_reproj_residual, so
// 0.5 (r0^2 + r1^2) and sqrt(r0^2 + r1^2) are the metric's per-factor terms), and where the covariances are given
//   S = J_c cov_c J_c^T + J_l cov_l J_l^T        (2 x 2, fp32; s = {S00, S01, S11})
// with J = jac_hfunc at the means and every sum taken k-sequentially from 0, the way the reference's matMul orders them.  The camera-
// landmark cross-covariance is not part of the beliefs and is neglected.  The covariances are general matrices (see moments), so S01
// is the entry of row 0 and no symmetry is assumed.
GBP_DEV void edge_residual(const float (&cm)[6], const float (&lm)[3], const float (&K)[9], float z0, float z1, float (&r)[2]) {
  float R[9];
  eval_cam_rot(cm, R);
  const float t[3] = {cm[0], cm[1], cm[2]};
  eval_reproj_residual(R, t, lm, z0, z1, K, r[0], r[1]);
}
template <int N>      // J [2 x N] cov [N x N] J^T: T = J cov, then T J^T
GBP_DEV void project_cov(const float* J, const float (&cov)[N * N], float (&S)[4]) {
  float T[2][N];
  GBP_UNROLL
  for (int a = 0; a < 2; ++a) {
    GBP_UNROLL
    for (int j = 0; j < N; ++j) {
      float acc = 0.f;
      GBP_UNROLL
      for (int k = 0; k < N; ++k) acc += J[a * N + k] * cov[k * N + j];
      T[a][j] = acc;
    }
  }
  GBP_UNROLL
  for (int a = 0; a < 2; ++a) {
    GBP_UNROLL
    for (int b = 0; b < 2; ++b) {
      float acc = 0.f;
      GBP_UNROLL
      for (int k = 0; k < N; ++k) acc += T[a][k] * J[b * N + k];
      S[a * 2 + b] = acc;
    }
  }
}
GBP_DEV void edge_reproj_cov(const float (&cm)[6], const float (&lm)[3], const float (&K)[9], const float (&cov_c)[36], const float (&cov_l)[9],
                             float (&s)[3]) {
  Lin lin;
  jac_hfunc(cm, lm, K, lin);
  float Sc[4], Sl[4];
  project_cov<6>(lin.Jkf, cov_c, Sc);
  project_cov<3>(lin.Jl, cov_l, Sl);
  s[0] = Sc[0] + Sl[0];
  s[1] = Sc[1] + Sl[1];
  s[2] = Sc[3] + Sl[3];
}

}  // namespace post
}  // namespace gbp
