// seed/seed_math.hpp — the seeding arithmetic (include/gbp_mi355x_seed.h states what it computes): the record of a camera, the
// triangulation, refinement and prior of one landmark, the prior eta of a new keyframe.  One header for both sides, as post/post_math.hpp:
// the kernels of gbp_seed.hip call these routines with one lane per camera / per landmark, a plain C++ translation unit
// (tests/sanitize/seed_math_main.cpp) calls them in a loop — GBP_DEV is then an ordinary inline function, and the pointers are host
// memory.  The rotation, the residual and the pivot solve are the metric's (csrc/kernels/gbp_metric_math.hpp), the refinement's Jacobian
// is the sweep's (csrc/gbp_device_math.hpp); the one restatement is jacobian_peak, whose original is a host function of the core library.
#pragma once
#include "../../include/gbp_mi355x_seed.h"
#include "../csrc/kernels/gbp_metric_math.hpp"

namespace gbp {
namespace seed {
using namespace gbpdev;

// what a landmark's lane needs of a camera, 64 bytes: four 16-byte loads from a 16-byte aligned table
struct alignas(16) CamRec {
  float R[9];      // eval_cam_rot of the mean
  float t[3];
  float o[3];      // the centre, -R^T t
  float pad;
};
static_assert(sizeof(CamRec) == 64, "one camera record is 64 bytes");

struct Params {      // by value in the kernel arguments
  float K[9];
  float min_parallax, fallback_depth, reproj_meas_var;
  uint32_t refine_iters;
};

GBP_DEV bool finite3(const float (&v)[3]) { return (v[0] - v[0] == 0.f) && (v[1] - v[1] == 0.f) && (v[2] - v[2] == 0.f); }

GBP_DEV void cam_record(const float (&cm)[6], CamRec& rec) {
  eval_cam_rot(cm, rec.R);
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) rec.t[i] = cm[i];
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) rec.o[i] = -((rec.R[i] * cm[0] + rec.R[3 + i] * cm[1]) + rec.R[6 + i] * cm[2]);
  rec.pad = 0.f;
}

// the arrays of one call (device pointers in the kernel, host pointers in the host program)
struct Graph {
  uint32_t n_cams, n_edges;
  const uint32_t* cam_id;
  const uint32_t* lmk_edges;
  const float* cam_mean;
  const float* meas;
  const uint32_t* active_flag;
  const CamRec* recs;
};

// The used observation behind index entry k: false if the entry is inactive or out of range (the latter sets GBP_SEED_BAD_INDEX).
GBP_DEV bool used_edge(const Graph& g, uint32_t k, uint32_t& e, uint32_t& c, uint32_t& status) {
  e = g.lmk_edges[k];
  if (e >= g.n_edges) { status |= GBP_SEED_BAD_INDEX; return false; }
  if (g.active_flag && g.active_flag[e] != 1u) return false;
  c = g.cam_id[e];
  if (c >= g.n_cams) { status |= GBP_SEED_BAD_INDEX; return false; }
  return true;
}

// R^T (the normalised pixel, 1): the observation's ray in the world frame, with camera-frame depth 1
GBP_DEV void pixel_ray(const CamRec& rec, const float (&K)[9], float u, float v, float (&w)[3]) {
  const float a = (u - K[2]) / K[0], b = (v - K[5]) / K[4];
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) w[i] = (rec.R[i] * a + rec.R[3 + i] * b) + rec.R[6 + i];
}

// Largest |entry| of the 2 x 9 reprojection Jacobian at (camera, x), and the camera-frame depth of x: jacobian_peak of csrc/gbp_host.cpp
// (util.cpp:48-72), the function gbp_set_prior_lambda takes its maxima of, operation for operation, on the record's rotation — which is
// rodrigues_host's.  Blocks: d/dt = jK, d/dw = jK (-hat(R x)), d/dx = jK R, with jK = d(p0 / p2, p1 / p2)/dp K.
GBP_DEV float jacobian_peak(const CamRec& rec, const float (&x)[3], const float (&K)[9], float& depth) {
  float Ry[3], pc[3], q[3];
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) Ry[i] = (rec.R[3 * i] * x[0] + rec.R[3 * i + 1] * x[1]) + rec.R[3 * i + 2] * x[2];
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) pc[i] = Ry[i] + rec.t[i];
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) q[i] = (K[3 * i] * pc[0] + K[3 * i + 1] * pc[1]) + K[3 * i + 2] * pc[2];
  depth = pc[2];
  const double z2 = (double)q[2] * (double)q[2];
  const float jp[6] = {1 / q[2], 0, (float)(-q[0] / z2), 0, 1 / q[2], (float)(-q[1] / z2)};
  const float D[9] = {-0.f, Ry[2], -Ry[1], -Ry[2], -0.f, Ry[0], Ry[1], -Ry[0], -0.f};      // -hat(R x)
  float jK[6], peak = 0.f;
  GBP_UNROLL
  for (int r = 0; r < 2; ++r) {
    GBP_UNROLL
    for (int c = 0; c < 3; ++c) {
      float s = 0.f;
      GBP_UNROLL
      for (int k = 0; k < 3; ++k) s += jp[r * 3 + k] * K[k * 3 + c];
      jK[r * 3 + c] = s;
    }
  }
  GBP_UNROLL
  for (int r = 0; r < 2; ++r) {
    GBP_UNROLL
    for (int c = 0; c < 3; ++c) {
      float s = 0.f, t = 0.f;
      GBP_UNROLL
      for (int k = 0; k < 3; ++k) {
        s += jK[r * 3 + k] * D[k * 3 + c];
        t += jK[r * 3 + k] * rec.R[k * 3 + c];
      }
      const float a0 = fabsf(jK[r * 3 + c]), a1 = fabsf(s), a2 = fabsf(t);
      const float m = a0 > (a1 > a2 ? a1 : a2) ? a0 : (a1 > a2 ? a1 : a2);
      peak = m > peak ? m : peak;
    }
  }
  return peak;
}

struct LandmarkSeed {
  float mean[3];
  float lam;
  float eta[3];
  uint32_t status, n_views;
};

// One landmark over index entries [k0, k1).  The caller has clamped the range to the index (k0 <= k1 <= n_edges).
GBP_DEV void seed_landmark(const Graph& g, const Params& p, uint32_t k0, uint32_t k1, uint32_t status, LandmarkSeed& out) {
  // ---- rays: the sums of the midpoint method, the mean ray, the first used view
  float A[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // I - d d^T summed: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
  float b[3] = {0.f, 0.f, 0.f}, m[3] = {0.f, 0.f, 0.f};
  float w0[3] = {0.f, 0.f, 0.f}, o0[3] = {0.f, 0.f, 0.f};
  uint32_t n = 0;
  for (uint32_t k = k0; k < k1; ++k) {
    uint32_t e, c;
    if (!used_edge(g, k, e, c, status)) continue;
    const CamRec rec = g.recs[c];
    float w[3], d[3];
    pixel_ray(rec, p.K, g.meas[2 * (size_t)e], g.meas[2 * (size_t)e + 1], w);
    const float len = sqrtf((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    GBP_UNROLL
    for (int i = 0; i < 3; ++i) d[i] = w[i] / len;
    if (n == 0) {
      GBP_UNROLL
      for (int i = 0; i < 3; ++i) { w0[i] = w[i]; o0[i] = rec.o[i]; }
    }
    const float dot = (d[0] * rec.o[0] + d[1] * rec.o[1]) + d[2] * rec.o[2];
    A[0] += 1.f - d[0] * d[0]; A[1] += -(d[0] * d[1]); A[2] += -(d[0] * d[2]);
    A[3] += 1.f - d[1] * d[1]; A[4] += -(d[1] * d[2]); A[5] += 1.f - d[2] * d[2];
    GBP_UNROLL
    for (int i = 0; i < 3; ++i) { b[i] += rec.o[i] - d[i] * dot; m[i] += d[i]; }
    ++n;
  }
  out.n_views = n;
  out.status = status;
  if (n == 0) {
    out.status |= GBP_SEED_NO_VIEW;
    return;
  }
  float place[3], x[3];
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) place[i] = o0[i] + p.fallback_depth * w0[i];
  bool placed = true;
  if (n == 1) {
    status |= GBP_SEED_ONE_VIEW;
  } else {
    const float inv_n = 1.f / (float)n;
    const float mm[3] = {m[0] * inv_n, m[1] * inv_n, m[2] * inv_n};
    const float parallax = 1.f - ((mm[0] * mm[0] + mm[1] * mm[1]) + mm[2] * mm[2]);
    if (parallax < p.min_parallax) {
      status |= GBP_SEED_LOW_PARALLAX;
    } else {
      placed = false;
      const float A9[9] = {A[0], A[1], A[2], A[1], A[3], A[4], A[2], A[4], A[5]};
      solve_pivot<3>(A9, 3, b, x);
      // ---- Gauss-Newton on the reprojection error, over x alone
      for (uint32_t it = 0; it < p.refine_iters; ++it) {
        float H[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gr[3] = {0.f, 0.f, 0.f};
        for (uint32_t k = k0; k < k1; ++k) {
          uint32_t e, c, ignored = 0;
          if (!used_edge(g, k, e, c, ignored)) continue;
          const CamRec rec = g.recs[c];
          float cm[6], r[2];
          GBP_UNROLL
          for (int i = 0; i < 6; ++i) cm[i] = g.cam_mean[6 * (size_t)c + i];
          eval_reproj_residual(rec.R, rec.t, x, g.meas[2 * (size_t)e], g.meas[2 * (size_t)e + 1], p.K, r[0], r[1]);
          Lin lin;
          jac_hfunc(cm, x, p.K, lin);
          const float (&J)[6] = lin.Jl;
          H[0] += J[0] * J[0] + J[3] * J[3]; H[1] += J[0] * J[1] + J[3] * J[4]; H[2] += J[0] * J[2] + J[3] * J[5];
          H[3] += J[1] * J[1] + J[4] * J[4]; H[4] += J[1] * J[2] + J[4] * J[5]; H[5] += J[2] * J[2] + J[5] * J[5];
          GBP_UNROLL
          for (int i = 0; i < 3; ++i) gr[i] += J[i] * r[0] + J[3 + i] * r[1];
        }
        const float H9[9] = {H[0], H[1], H[2], H[1], H[3], H[4], H[2], H[4], H[5]};
        float dx[3];
        solve_pivot<3>(H9, 3, gr, dx);
        const float xn[3] = {x[0] + dx[0], x[1] + dx[1], x[2] + dx[2]};
        if (!finite3(xn)) break;
        GBP_UNROLL
        for (int i = 0; i < 3; ++i) x[i] = xn[i];
      }
      if (!finite3(x)) placed = true;
      if (placed) status |= GBP_SEED_NONFINITE;
    }
  }
  if (placed) {
    GBP_UNROLL
    for (int i = 0; i < 3; ++i) x[i] = place[i];
  }
  // ---- the prior at the seeded point; a non-finite result moves the point to the placement, once
  for (;;) {
    float peak = 0.f;
    bool behind = false;
    for (uint32_t k = k0; k < k1; ++k) {
      uint32_t e, c, ignored = 0;
      if (!used_edge(g, k, e, c, ignored)) continue;
      const CamRec rec = g.recs[c];
      float depth;
      const float a = jacobian_peak(rec, x, p.K, depth);
      peak = a > peak ? a : peak;      // (a NaN is not a maximum)
      behind |= depth <= 0.f;          // (a NaN depth is the non-finite bit's business)
    }
    out.lam = (float)(((double)peak * (double)peak) / (double)p.reproj_meas_var);
    GBP_UNROLL
    for (int i = 0; i < 3; ++i) { out.mean[i] = x[i]; out.eta[i] = x[i] * out.lam; }
    const bool finite = finite3(out.mean) && finite3(out.eta) && (out.lam - out.lam == 0.f);
    out.status = status | (behind ? GBP_SEED_BEHIND : 0u);
    if (finite) break;
    out.status |= GBP_SEED_NONFINITE;
    if (placed) break;
    placed = true;
    status |= GBP_SEED_NONFINITE;
    GBP_UNROLL
    for (int i = 0; i < 3; ++i) x[i] = place[i];
  }
}

// gbp_slam_initialise_new_kf on the device: the mean of camera src, the fp32 row dots of camera dst's prior Lambda with it
GBP_DEV void keyframe_prior(const float* belief_eta, const float* belief_lambda, const float* prior_lambda, float (&mu)[6], float (&eta)[6]) {
  float lam[36], be[6];
  GBP_UNROLL
  for (int i = 0; i < 36; ++i) lam[i] = belief_lambda[i];
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) be[i] = belief_eta[i];
  solve_pivot<6>(lam, 6, be, mu);
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) {
    float s = 0.f;
    GBP_UNROLL
    for (int k = 0; k < 6; ++k) s += prior_lambda[6 * i + k] * mu[k];
    eta[i] = s;
  }
}

}  // namespace seed
}  // namespace gbp
