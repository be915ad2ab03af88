// locate/locate_math.hpp — the arithmetic of camera location (include/gbp_mi355x_locate.h states what it computes): the hash and the
// sampling of a hypothesis, the three-point solver, a candidate's agreement with an observation, the pose of the winner, the final
// pass, and the loop over rounds, hypotheses and solutions of one camera.  One header for both sides, as resect/resect_math.hpp (whose
// Graph, used_entry and camera_range it takes by inclusion): the kernel of gbp_locate.hip runs locate_camera with one wavefront per
// camera (its Wave: lane = hypothesis while generating, lane = observation while scoring), a plain C++ translation unit
// (tests/sanitize/locate_math_main.cpp) runs it with a Wave that loops.  The fp64 part uses + - x / and sqrt only, so both sides
// produce the same bits; the final pass is the solver's own prediction (csrc/gbp_device_math.hpp: cam_lin, jac_hfunc_lin).
#pragma once
#include "../../include/gbp_mi355x_locate.h"
#include "../resect/resect_math.hpp"

namespace gbp {
namespace locate {
using namespace gbpdev;
using resect::camera_range;
using resect::Graph;
using resect::used_entry;

constexpr int kLanes = 64;         // hypotheses of a round; the stride of the scoring passes
constexpr int kMaxSol = 4;         // solutions of a hypothesis
constexpr int kTries = 8;          // tries of a slot
constexpr int kNewton = 40;        // Newton steps on the cubic
constexpr int kAtanTerms = 13;     // x .. x^25
constexpr double kHair = 1e-4;     // the shortest rotation vector returned
constexpr double kCollinear = 1e-10;   // sin^2 of the triangle's angle at point 1 below which there is no solution

struct Params {      // by value in the kernel arguments
  float K[9];
  float inlier_px;
  uint32_t rounds, min_inliers, seed;
};

struct Outputs {
  float* cam_mean;
  uint32_t* inlier;
  float* report;
  uint32_t* status;
  uint32_t* n_views;
  uint32_t* n_inliers;
};

struct Obs {      // one index entry: its edge, landmark, pixel and landmark mean if it is used
  float z0, z1, X0, X1, X2;
  uint32_t e, l;
  bool used;
};

struct Cand {     // a candidate pose, fp32: yc = R X + t
  float R[9], t[3];
};

struct Hyp {      // the solutions of one hypothesis, twelve floats each (R row-major, then t)
  float v[12 * kMaxSol];
  uint32_t n;
};

GBP_DEV uint32_t mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

GBP_DEV void load_obs(const Graph& g, uint32_t k, Obs& o, bool& bad) {
  o.e = 0u; o.l = 0xffffffffu;
  o.z0 = o.z1 = o.X0 = o.X1 = o.X2 = 0.f;
  o.used = used_entry(g, k, o.e, o.l, bad);
  if (!o.used) { o.l = 0xffffffffu; return; }
  o.X0 = g.lmk_mean[3 * (size_t)o.l]; o.X1 = g.lmk_mean[3 * (size_t)o.l + 1]; o.X2 = g.lmk_mean[3 * (size_t)o.l + 2];
  o.z0 = g.meas[2 * (size_t)o.e]; o.z1 = g.meas[2 * (size_t)o.e + 1];
}

// the three index entries of hypothesis (r, j) of camera c; false: a slot found no entry (the hypothesis is void)
GBP_DEV bool sample_triple(const Graph& g, uint32_t seed, uint32_t c, uint32_t r, uint32_t j, uint32_t k0, uint32_t deg, Obs (&o)[3], uint32_t (&off)[3]) {
  const uint32_t h = mix(mix(seed + c) + 64u * r + j);
  bool ok = true;
  GBP_UNROLL
  for (int s = 0; s < 3; ++s) {
    bool found = false;
    o[s].used = false; o[s].l = 0xffffffffu; o[s].e = 0u;
    o[s].z0 = o[s].z1 = o[s].X0 = o[s].X1 = o[s].X2 = 0.f;
    off[s] = 0u;
    for (int t = 0; t < kTries && !found; ++t) {
      const uint32_t u = mix(h + 8u * (uint32_t)s + (uint32_t)t);
      const uint32_t d = (uint32_t)(((uint64_t)u * deg) >> 32);
      Obs q;
      bool ignored = false;
      load_obs(g, k0 + d, q, ignored);
      bool fresh = q.used;
      GBP_UNROLL
      for (int i = 0; i < 3; ++i)
        if (i < s) fresh = fresh && q.l != o[i].l;
      if (fresh) { o[s] = q; off[s] = d; found = true; }
    }
    ok = ok && found;
  }
  return ok;
}

// ---- fp64, IEEE operations only ----
GBP_DEV bool fin(double v) { return v - v == 0.0; }
GBP_DEV double dabs(double v) { return v < 0.0 ? -v : v; }
GBP_DEV double sel3(int i, double a, double b, double c) { return i == 0 ? a : (i == 1 ? b : c); }

GBP_DEV double det3(const double (&M)[9]) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}
GBP_DEV void adj3(const double (&M)[9], double (&A)[9]) {      // M adj(M) = det(M) I
  A[0] = M[4] * M[8] - M[5] * M[7]; A[1] = M[2] * M[7] - M[1] * M[8]; A[2] = M[1] * M[5] - M[2] * M[4];
  A[3] = M[5] * M[6] - M[3] * M[8]; A[4] = M[0] * M[8] - M[2] * M[6]; A[5] = M[2] * M[3] - M[0] * M[5];
  A[6] = M[3] * M[7] - M[4] * M[6]; A[7] = M[1] * M[6] - M[0] * M[7]; A[8] = M[0] * M[4] - M[1] * M[3];
}
GBP_DEV double tr_prod(const double (&A)[9], const double (&B)[9]) {      // trace(A B)
  double s = 0.0;
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) {
    GBP_UNROLL
    for (int j = 0; j < 3; ++j) s += A[3 * i + j] * B[3 * j + i];
  }
  return s;
}
GBP_DEV double bilinear(const double (&u)[3], const double (&Q)[9], const double (&v)[3]) {
  double s = 0.0;
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) {
    GBP_UNROLL
    for (int j = 0; j < 3; ++j) s += u[i] * Q[3 * i + j] * v[j];
  }
  return s;
}
GBP_DEV void cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
GBP_DEV double dot(const double (&a)[3], const double (&b)[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// The real root of x^3 + b x^2 + c x + d Newton converges to from the convex side (the header's step 3.c).
GBP_DEV double cubic_root(double b, double c, double d) {
  const double b3 = b / 3.0;
  const double p = c - b * b3;
  const double q = 2.0 * b3 * b3 * b3 - b3 * c + d;
  const double aq = dabs(q);                       // y^3 + p y - |q| = 0 has a root y >= 0; the root of the cubic is -+ y - b / 3
  const double sp = sqrt(dabs(p)), sq = sqrt(aq);
  const double s = aq <= 1.0 ? sqrt(sq) : sq;      // >= |q|^(1/3)
  double y = 2.0 * (sp > s ? sp : s);
  for (int i = 0; i < kNewton; ++i) {
    const double gv = (y * y + p) * y - aq, gp = 3.0 * (y * y) + p;
    y = gp > 0.0 ? y - gv / gp : y;
  }
  return (q > 0.0 ? -y : y) - b3;
}

// The three-point solver (Persson and Nordberg's formulation: the depths' quadrics, a degenerate member of their pencil, its two
// planes).  y: the unit bearings, X: the points; up to four (R, t) with R X_i + t = depth_i y_i, depth_i > 0, into R [n][9], t [n][3].
GBP_DEV int p3p(const double (&y)[3][3], const double (&X)[3][3], double (&Rs)[kMaxSol][9], double (&ts)[kMaxSol][3]) {
  double F1[3], F2[3], F3[3], X23[3];
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) { F1[i] = X[1][i] - X[0][i]; F2[i] = X[2][i] - X[0][i]; X23[i] = X[2][i] - X[1][i]; }
  cross(F1, F2, F3);
  const double A12 = dot(F1, F1), A13 = dot(F2, F2), A23 = dot(X23, X23), n3 = dot(F3, F3);
  if (!(n3 > kCollinear * (A12 * A13))) return 0;      // repeated or collinear points, or a NaN
  const double asum = A12 + A13 + A23;
  const double a12 = A12 / asum, a13 = A13 / asum, a23 = A23 / asum;
  const double b12 = dot(y[0], y[1]), b13 = dot(y[0], y[2]), b23 = dot(y[1], y[2]);
  const double D1[9] = {a23, -(a23 * b12), 0.0, -(a23 * b12), a23 - a12, a12 * b23, 0.0, a12 * b23, -a12};
  const double D2[9] = {a23, 0.0, -(a23 * b13), 0.0, -a13, a13 * b23, -(a23 * b13), a13 * b23, a23 - a13};
  double J1[9], J2[9];
  adj3(D1, J1);
  adj3(D2, J2);
  const double c0 = det3(D1), c3 = det3(D2), c1 = tr_prod(J1, D2), c2 = tr_prod(J2, D1);
  const bool swap = !(dabs(c3) >= dabs(c0));      // det(A + g B) with the larger of the two determinants leading
  const double lead = swap ? c0 : c3;
  if (!(dabs(lead) > 0.0)) return 0;
  const double g = swap ? cubic_root(c1 / lead, c2 / lead, c3 / lead) : cubic_root(c2 / lead, c1 / lead, c0 / lead);
  if (!fin(g)) return 0;
  double D0[9], Q[9];
  const bool useB = dabs(g) <= 1.0;                 // the member the planes are cut with: B where A = -g B is the smaller one
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) {
    const double A = swap ? D2[i] : D1[i], B = swap ? D1[i] : D2[i];
    D0[i] = A + g * B;
    Q[i] = useB ? B : A;
  }
  // D0 = l m^T + m l^T: adj(D0) = -(l x m)(l x m)^T; with p = (l x m) up to sign, D0 + [p]x has rank one: its rows are m, its columns l
  double Bm[9];
  adj3(D0, Bm);
  int pi = 0;
  double pd = -Bm[0];
  if (-Bm[4] > pd) { pi = 1; pd = -Bm[4]; }
  if (-Bm[8] > pd) { pi = 2; pd = -Bm[8]; }
  if (!(pd > 0.0)) return 0;
  const double beta = sqrt(pd);
  const double px = sel3(pi, Bm[0], Bm[1], Bm[2]) / beta, py = sel3(pi, Bm[3], Bm[4], Bm[5]) / beta, pz = sel3(pi, Bm[6], Bm[7], Bm[8]) / beta;
  const double Cm[9] = {D0[0], D0[1] - pz, D0[2] + py, D0[3] + pz, D0[4], D0[5] - px, D0[6] - py, D0[7] + px, D0[8]};
  int br = 0, bc = 0;
  double bv = -1.0;
  GBP_UNROLL
  for (int r = 0; r < 3; ++r) {
    GBP_UNROLL
    for (int c = 0; c < 3; ++c) {
      const double a = dabs(Cm[3 * r + c]);
      if (a > bv) { bv = a; br = r; bc = c; }
    }
  }
  if (!(bv > 0.0)) return 0;
  const double lines[2][3] = {{sel3(br, Cm[0], Cm[3], Cm[6]), sel3(br, Cm[1], Cm[4], Cm[7]), sel3(br, Cm[2], Cm[5], Cm[8])},
                              {sel3(bc, Cm[0], Cm[1], Cm[2]), sel3(bc, Cm[3], Cm[4], Cm[5]), sel3(bc, Cm[6], Cm[7], Cm[8])}};
  // the inverse of (F1 F2 F3) by rows: (F2 x F3, F3 x F1, F3) / |F3|^2
  double G1[3], G2[3], G3[3];
  cross(F2, F3, G1);
  cross(F3, F1, G2);
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) { G1[i] = G1[i] / n3; G2[i] = G2[i] / n3; G3[i] = F3[i] / n3; }
  int n = 0;
  GBP_UNROLL
  for (int li = 0; li < 2; ++li) {
    const double n0 = lines[li][0], n1 = lines[li][1], n2 = lines[li][2];
    int k = 0;
    double nk = dabs(n0);
    if (dabs(n1) > nk) { k = 1; nk = dabs(n1); }
    if (dabs(n2) > nk) { k = 2; nk = dabs(n2); }
    if (!(nk > 0.0)) continue;
    // the plane n . L = 0 spanned by u and v: the depth with the largest coefficient is expressed by the other two
    const double m0 = -(n0 / sel3(k, n0, n1, n2)), m1 = -(n1 / sel3(k, n0, n1, n2)), m2 = -(n2 / sel3(k, n0, n1, n2));
    // k == 0: L = a (m1, 1, 0) + b (m2, 0, 1); k == 1: a (1, m0, 0) + b (0, m2, 1); k == 2: a (1, 0, m0) + b (0, 1, m1); tau = a / b
    const double uu[3] = {k == 0 ? m1 : 1.0, k == 0 ? 1.0 : (k == 1 ? m0 : 0.0), k == 2 ? m0 : 0.0};
    const double v[3] = {k == 0 ? m2 : 0.0, k == 2 ? 1.0 : (k == 1 ? m2 : 0.0), k == 2 ? m1 : 1.0};
    const double qa = bilinear(uu, Q, uu), qb = bilinear(uu, Q, v), qc = bilinear(v, Q, v);
    const double disc = qb * qb - qa * qc;
    if (!(disc >= 0.0)) continue;
    const double sd = sqrt(disc);
    const double qq = -(qb + (qb >= 0.0 ? sd : -sd));
    const double taus[2] = {qq / qa, qc / qq};
    GBP_UNROLL
    for (int ti = 0; ti < 2; ++ti) {
      const double tau = taus[ti];
      double w[3];
      GBP_UNROLL
      for (int i = 0; i < 3; ++i) w[i] = tau * uu[i] + v[i];
      const double S = (w[0] * w[0] + w[1] * w[1] - 2.0 * b12 * (w[0] * w[1])) + (w[0] * w[0] + w[2] * w[2] - 2.0 * b13 * (w[0] * w[2])) +
                       (w[1] * w[1] + w[2] * w[2] - 2.0 * b23 * (w[1] * w[2]));
      if (!(S > 0.0)) continue;
      const double sc = sqrt(asum / S);
      const double L0 = sc * w[0], L1 = sc * w[1], L2 = sc * w[2];
      if (!(L0 > 0.0 && L1 > 0.0 && L2 > 0.0)) continue;
      double Y1[3], E1[3], E2[3], E3[3];
      GBP_UNROLL
      for (int i = 0; i < 3; ++i) { Y1[i] = L0 * y[0][i]; E1[i] = L1 * y[1][i] - Y1[i]; E2[i] = L2 * y[2][i] - Y1[i]; }
      cross(E1, E2, E3);
      double R[9], t[3];
      bool ok = true;
      GBP_UNROLL
      for (int i = 0; i < 3; ++i) {
        GBP_UNROLL
        for (int jj = 0; jj < 3; ++jj) {
          R[3 * i + jj] = E1[i] * G1[jj] + E2[i] * G2[jj] + E3[i] * G3[jj];
          ok = ok && fin(R[3 * i + jj]);
        }
      }
      GBP_UNROLL
      for (int i = 0; i < 3; ++i) {
        t[i] = Y1[i] - (R[3 * i] * X[0][0] + R[3 * i + 1] * X[0][1] + R[3 * i + 2] * X[0][2]);
        ok = ok && fin(t[i]);
      }
      if (!ok) continue;
      GBP_UNROLL
      for (int s = 0; s < kMaxSol; ++s) {
        if (s == n) {
          GBP_UNROLL
          for (int i = 0; i < 9; ++i) Rs[s][i] = R[i];
          GBP_UNROLL
          for (int i = 0; i < 3; ++i) ts[s][i] = t[i];
        }
      }
      ++n;
    }
  }
  return n;
}

// the unit bearing of a pixel through K (fx = K[0], fy = K[4], cx = K[2], cy = K[5])
GBP_DEV void bearing(const float (&K)[9], float z0, float z1, double (&y)[3]) {
  const double a = ((double)z0 - (double)K[2]) / (double)K[0], b = ((double)z1 - (double)K[5]) / (double)K[4];
  const double nrm = sqrt(a * a + b * b + 1.0);
  y[0] = a / nrm; y[1] = b / nrm; y[2] = 1.0 / nrm;
}

// hypothesis (r, j) of camera c: sample, solve, round to fp32
GBP_DEV void hypothesis(const Graph& g, const Params& p, uint32_t c, uint32_t r, uint32_t j, uint32_t k0, uint32_t deg, Hyp& h) {
  h.n = 0u;
  GBP_UNROLL
  for (int i = 0; i < 12 * kMaxSol; ++i) h.v[i] = 0.f;
  Obs o[3];
  uint32_t off[3];
  if (!sample_triple(g, p.seed, c, r, j, k0, deg, o, off)) return;
  double y[3][3], X[3][3];
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) {
    bearing(p.K, o[i].z0, o[i].z1, y[i]);
    X[i][0] = (double)o[i].X0; X[i][1] = (double)o[i].X1; X[i][2] = (double)o[i].X2;
  }
  double Rs[kMaxSol][9], ts[kMaxSol][3];
  const int n = p3p(y, X, Rs, ts);
  h.n = (uint32_t)n;
  GBP_UNROLL
  for (int s = 0; s < kMaxSol; ++s) {
    if (s < n) {
      GBP_UNROLL
      for (int i = 0; i < 9; ++i) h.v[12 * s + i] = (float)Rs[s][i];
      GBP_UNROLL
      for (int i = 0; i < 3; ++i) h.v[12 * s + 9 + i] = (float)ts[s][i];
    }
  }
}

// ---- scoring, fp32 ----
GBP_DEV bool agrees(const Cand& c, const Obs& o, const float (&K)[9], float thr2) {
  const float y0 = ((c.R[0] * o.X0 + c.R[1] * o.X1) + c.R[2] * o.X2) + c.t[0];
  const float y1 = ((c.R[3] * o.X0 + c.R[4] * o.X1) + c.R[5] * o.X2) + c.t[1];
  const float y2 = ((c.R[6] * o.X0 + c.R[7] * o.X1) + c.R[8] * o.X2) + c.t[2];
  const float du = o.z0 - (K[0] * (y0 / y2) + K[2]), dv = o.z1 - (K[4] * (y1 / y2) + K[5]);
  return o.used && y2 > 0.f && du * du + dv * dv <= thr2;
}

// ---- the pose of the winner ----
// atan2(s, c) for s, c >= 0 not both zero: t = min / max; above sqrt(2) - 1, atan t = pi/4 + atan((t - 1) / (t + 1)); the Taylor
// polynomial through x^25 on |x| <= sqrt(2) - 1 (truncation below 2e-12); pi/2 - . if s > c
GBP_DEV double atan2_pos(double s, double c) {
  const double hi = s > c ? s : c, lo = s > c ? c : s;
  const double t = lo / hi;
  const bool shift = t > 0.41421356237309503;
  const double x = shift ? (t - 1.0) / (t + 1.0) : t;
  const double z = x * x;
  double acc = (((kAtanTerms - 1) & 1) ? -1.0 : 1.0) / (double)(2 * kAtanTerms - 1);
  GBP_UNROLL
  for (int k = kAtanTerms - 2; k >= 0; --k) {
    const double ck = 1.0 / (double)(2 * k + 1);
    acc = ((k & 1) ? -ck : ck) + z * acc;
  }
  double a = x * acc;
  if (shift) a = 0.78539816339744828 + a;
  return s > c ? 1.5707963267948966 - a : a;
}

GBP_DEV void pose_of(const Cand& cd, float (&x)[6]) {
  double R[9];
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) R[i] = (double)cd.R[i];
  const double tr = R[0] + R[4] + R[8];
  double qw, qx, qy, qz;
  if (tr > 0.0) {
    const double S = 2.0 * sqrt(tr + 1.0);
    qw = S / 4.0; qx = (R[7] - R[5]) / S; qy = (R[2] - R[6]) / S; qz = (R[3] - R[1]) / S;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double S = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]);
    qw = (R[7] - R[5]) / S; qx = S / 4.0; qy = (R[1] + R[3]) / S; qz = (R[2] + R[6]) / S;
  } else if (R[4] > R[8]) {
    const double S = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]);
    qw = (R[2] - R[6]) / S; qx = (R[1] + R[3]) / S; qy = S / 4.0; qz = (R[5] + R[7]) / S;
  } else {
    const double S = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]);
    qw = (R[3] - R[1]) / S; qx = (R[2] + R[6]) / S; qy = (R[5] + R[7]) / S; qz = S / 4.0;
  }
  if (qw < 0.0) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
  const double nq = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  qw = qw / nq; qx = qx / nq; qy = qy / nq; qz = qz / nq;
  const double vn = sqrt(qx * qx + qy * qy + qz * qz);
  const double theta = 2.0 * atan2_pos(vn, qw);
  double w0, w1, w2;
  if (theta >= kHair) {
    const double k = theta / vn;
    w0 = k * qx; w1 = k * qy; w2 = k * qz;
  } else if (vn > 0.0) {
    const double k = kHair / vn;
    w0 = k * qx; w1 = k * qy; w2 = k * qz;
  } else {                       // (no axis, or a NaN: the final pass decides)
    w0 = kHair; w1 = 0.0; w2 = 0.0;
  }
  x[0] = cd.t[0]; x[1] = cd.t[1]; x[2] = cd.t[2];
  x[3] = (float)w0; x[4] = (float)w1; x[5] = (float)w2;
}

// ---- the final pass: the solver's own prediction at the written pose ----
GBP_DEV bool final_agrees(const float (&x)[6], const CamLin& cl, const Obs& o, const float (&K)[9], float thr2, float& err2) {
  const float lm[3] = {o.X0, o.X1, o.X2};
  Lin lin;
  jac_hfunc_lin(x, lm, K, cl, lin);
  float depth = 0.f;
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) depth += cl.R[6 + i] * lm[i];
  depth += x[2];
  const float r0 = o.z0 - lin.hx[0], r1 = o.z1 - lin.hx[1];
  err2 = r0 * r0 + r1 * r1;
  return o.used && depth > 0.f && err2 <= thr2;
}

struct CameraResult {
  float x[6];
  float mse;
  uint32_t status, n_views, n_inliers, n_cand, win_h, win_s;
  int level;      // what is stored: 0 status and n_views; 1 and n_inliers; 2 everything
};

// One camera.  Wave (every result the same in every lane, so every branch below is the whole wave's):
//   void count(uint32_t& n_views, bool& bad)
//   void generate(uint32_t r)                          hypothesis (r, j) for j = 0 .. 63
//   bool candidate(uint32_t j, int s, Cand& c)         solution s of hypothesis j of the round generated last, if it exists
//   uint32_t score(const Cand& c, float thr2)          the used observations that agree
//   void final_pass(const float (&x)[6], float thr2, uint32_t& n, float& sumsq)
//   void mark(const float (&x)[6], float thr2)         inlier[e] of every used observation
template <class Wave>
GBP_DEV void locate_camera(Wave& wave, const Params& p, uint32_t status, CameraResult& out) {
  bool bad = false;
  uint32_t n = 0u;
  wave.count(n, bad);
  if (bad) status |= GBP_LOCATE_BAD_INDEX;
  out.n_views = n; out.n_inliers = 0u; out.n_cand = 0u; out.win_h = 0u; out.win_s = 0u; out.mse = 0.f; out.level = 0;
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) out.x[i] = 0.f;
  if (n == 0u) { out.status = status | GBP_LOCATE_NO_VIEW; return; }
  if (n < p.min_inliers) { out.status = status | GBP_LOCATE_FEW_VIEWS; return; }
  const float thr2 = p.inlier_px * p.inlier_px;
  bool have = false;
  uint32_t best = 0u;
  Cand bc;
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) bc.R[i] = 0.f;
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) bc.t[i] = 0.f;
  for (uint32_t r = 0; r < p.rounds; ++r) {
    wave.generate(r);
    for (uint32_t j = 0; j < (uint32_t)kLanes; ++j) {
      GBP_UNROLL
      for (int s = 0; s < kMaxSol; ++s) {
        Cand cd;
        if (!wave.candidate(j, s, cd)) continue;
        const uint32_t cnt = wave.score(cd, thr2);
        out.n_cand += 1u;
        if (!have || cnt > best) {
          have = true; best = cnt; bc = cd;
          out.win_h = 64u * r + j; out.win_s = (uint32_t)s;
        }
      }
    }
  }
  if (!have) { out.status = status | GBP_LOCATE_NO_HYPOTHESIS; return; }
  pose_of(bc, out.x);
  float sumsq = 0.f;
  wave.final_pass(out.x, thr2, out.n_inliers, sumsq);
  out.level = 1;
  if (out.n_inliers < p.min_inliers) { out.status = status | GBP_LOCATE_FEW_INLIERS; return; }
  out.level = 2;
  wave.mark(out.x, thr2);
  out.mse = sumsq / (float)out.n_inliers;
  out.status = status;
}

// what one lane stores of camera c
GBP_DEV void store_camera(const Outputs& o, uint32_t c, const CameraResult& r) {
  o.status[c] = r.status;
  if (o.n_views) o.n_views[c] = r.n_views;
  if (r.level >= 1 && o.n_inliers) o.n_inliers[c] = r.n_inliers;
  if (r.level < 2) return;
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) o.cam_mean[6 * (size_t)c + i] = r.x[i];
  if (o.report) {
    o.report[4 * (size_t)c] = (float)r.win_h;
    o.report[4 * (size_t)c + 1] = (float)r.win_s;
    o.report[4 * (size_t)c + 2] = (float)r.n_cand;
    o.report[4 * (size_t)c + 3] = r.mse;
  }
}

}  // namespace locate
}  // namespace gbp
