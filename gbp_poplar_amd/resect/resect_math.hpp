// resect/resect_math.hpp — the resection arithmetic (include/gbp_mi355x_resect.h states what it computes): one observation's share of a
// pass, a lane's partial of a pass, the combine of two partials, the Levenberg-Marquardt loop of one camera and what it stores.  One
// header for both sides, as seed/seed_math.hpp: the kernel of gbp_resect.hip runs resect_camera with one wavefront per camera (its
// Wave: 64 lanes, the tree across them), a plain C++ translation unit (tests/sanitize/resect_math_main.cpp) runs it with a Wave that
// loops over 64 partials — GBP_DEV is then an ordinary inline function, and the pointers are host memory.  The linearisation is the
// sweep's (csrc/gbp_device_math.hpp: cam_lin, jac_hfunc_lin), the solve is the metric's (csrc/kernels/gbp_metric_math.hpp).
#pragma once
#include "../../include/gbp_mi355x_resect.h"
#include "../csrc/kernels/gbp_metric_math.hpp"

namespace gbp {
namespace resect {
using namespace gbpdev;

constexpr int kLanes = 64;      // the partials of the definition
constexpr int kSums = 28;       // cost, H (21 upper entries, row-major: (0,0) (0,1) .. (0,5) (1,1) ..), g (6)

struct Params {      // by value in the kernel arguments
  float K[9];
  float huber_px, lambda0, reproj_meas_var;
  uint32_t max_passes, min_views;
};

// the arrays of one call (device pointers in the kernel, host pointers in the host program)
struct Graph {
  uint32_t n_lmks, n_edges;
  const uint32_t* lmk_id;
  const uint32_t* cam_edges;      // NULL: entry k is edge k
  const float* lmk_mean;
  const float* meas;
  const uint32_t* active_flag;    // NULL: all
  const uint32_t* lmk_use;        // NULL: all
};

struct Outputs {
  float* cam_mean;
  const float* cam_priors_lambda;
  float* cam_priors_eta;
  float* cam_info;
  float* report;
  uint32_t* status;
  uint32_t* n_views;
};

struct Sums {
  float v[kSums];
  uint32_t n;
};

// index of H(i, j), i <= j, in Sums::v
GBP_DEV constexpr int hidx(int i, int j) { return 1 + i * 6 - i * (i - 1) / 2 + (j - i); }

GBP_DEV void clear(Sums& s) {
  GBP_UNROLL
  for (int i = 0; i < kSums; ++i) s.v[i] = 0.f;
  s.n = 0u;
}
// one step of the halving tree: partial i += partial i + s
GBP_DEV void combine(Sums& a, const Sums& b) {
  GBP_UNROLL
  for (int i = 0; i < kSums; ++i) a.v[i] += b.v[i];
  a.n += b.n;
}
GBP_DEV bool finite(const Sums& s) {
  bool ok = true;
  GBP_UNROLL
  for (int i = 0; i < kSums; ++i) ok = ok && (s.v[i] - s.v[i] == 0.f);
  return ok;
}
GBP_DEV bool finite6(const float (&v)[6]) {
  bool ok = true;
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) ok = ok && (v[i] - v[i] == 0.f);
  return ok;
}

// The used observation behind index entry k: false if the entry is inactive, excluded or out of range (the latter sets bad).
GBP_DEV bool used_entry(const Graph& g, uint32_t k, uint32_t& e, uint32_t& l, bool& bad) {
  e = g.cam_edges ? g.cam_edges[k] : k;
  if (e >= g.n_edges) { bad = true; return false; }
  if (g.active_flag && g.active_flag[e] != 1u) return false;
  l = g.lmk_id[e];
  if (l >= g.n_lmks) { bad = true; return false; }
  if (g.lmk_use && g.lmk_use[l] == 0u) return false;
  return true;
}

// One lane's partial of pass(x): the entries k0 + lane, k0 + lane + 64, ... below k1, serially from zero.  behind: a used landmark with
// camera-frame depth <= 0 (jac_hfunc_lin's yc[2], the same operations).
GBP_DEV void lane_pass(const Graph& g, const Params& p, const float (&x)[6], const CamLin& cl, uint32_t k0, uint32_t k1, uint32_t lane, Sums& s,
                       bool& behind, bool& bad) {
  clear(s);
  for (uint64_t k = (uint64_t)k0 + lane; k < k1; k += kLanes) {
    uint32_t e, l;
    if (!used_entry(g, (uint32_t)k, e, l, bad)) continue;
    float lm[3];
    GBP_UNROLL
    for (int i = 0; i < 3; ++i) lm[i] = g.lmk_mean[3 * (size_t)l + i];
    const float z0 = g.meas[2 * (size_t)e], z1 = g.meas[2 * (size_t)e + 1];
    Lin lin;
    jac_hfunc_lin(x, lm, p.K, cl, lin);
    float depth = 0.f;
    GBP_UNROLL
    for (int i = 0; i < 3; ++i) depth += cl.R[6 + i] * lm[i];
    depth += x[2];
    behind = behind || depth <= 0.f;      // (a NaN depth is the non-finite bit's business)
    const float (&J)[12] = lin.Jkf;
    const float r0 = z0 - lin.hx[0], r1 = z1 - lin.hx[1];
    const float err = sqrtf(r0 * r0 + r1 * r1);
    const bool plain = p.huber_px <= 0.f || err <= p.huber_px;
    const float w = plain ? 1.f : p.huber_px / err;
    const float rho = plain ? 0.5f * (err * err) : p.huber_px * (err - 0.5f * p.huber_px);
    s.v[0] += rho;
    GBP_UNROLL
    for (int i = 0; i < 6; ++i) {
      GBP_UNROLL
      for (int j = i; j < 6; ++j) s.v[hidx(i, j)] += w * (J[i] * J[j] + J[6 + i] * J[6 + j]);
    }
    GBP_UNROLL
    for (int i = 0; i < 6; ++i) s.v[22 + i] += w * (J[i] * r0 + J[6 + i] * r1);
    s.n += 1u;
  }
}

// lane 0's share of a step: A = H with the diagonal scaled, dx = A^-1 g
GBP_DEV void lm_step(const Sums& s, float lam, float (&dx)[6]) {
  float A[36], gr[6];
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) {
    GBP_UNROLL
    for (int j = 0; j < 6; ++j) A[6 * i + j] = i == j ? s.v[hidx(i, i)] * (1.f + lam) : s.v[i < j ? hidx(i, j) : hidx(j, i)];
    gr[i] = s.v[22 + i];
  }
  solve_pivot<6>(A, 6, gr, dx);
}

struct CameraResult {
  float x[6];
  Sums s;              // the accepted pass
  float start_cost, last_step, lam;
  uint32_t status, n_views;
  bool written;        // false: only status and n_views are stored
};

// One camera over index entries [k0, k1) (clamped by the caller, who passes what the clamp flagged as status).  Wave:
//   void pass(const float (&x)[6], Sums& total, bool& behind, bool& bad)   the tree's result, the same in every lane
//   void solve(const Sums& s, float lam, float (&dx)[6])                   lm_step in one lane, dx the same in every lane
// so every branch below is taken by the whole wave.
template <class Wave>
GBP_DEV void resect_camera(Wave& wave, const Params& p, const float (&start)[6], uint32_t status, CameraResult& out) {
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) out.x[i] = start[i];
  bool behind = false, bad = false;
  wave.pass(out.x, out.s, behind, bad);
  if (bad) status |= GBP_RESECT_BAD_INDEX;
  out.n_views = out.s.n;
  out.written = false;
  out.start_cost = out.s.v[0];
  out.last_step = 0.f;
  out.lam = p.lambda0;
  if (out.s.n == 0u) { out.status = status | GBP_RESECT_NO_VIEW; return; }
  if (out.s.n < p.min_views) { out.status = status | GBP_RESECT_FEW_VIEWS; return; }
  if (!finite(out.s)) { out.status = status | GBP_RESECT_NONFINITE; return; }
  out.written = true;
  bool accepted = false;
  uint32_t passes = 1u;
  float lam = p.lambda0;
  while (passes < p.max_passes && lam <= 1e8f) {
    float dx[6], xt[6];
    wave.solve(out.s, lam, dx);
    if (!finite6(dx)) { lam *= 10.f; continue; }
    GBP_UNROLL
    for (int i = 0; i < 6; ++i) xt[i] = out.x[i] + dx[i];
    Sums t;
    bool behind_t = false, ignored = false;
    wave.pass(xt, t, behind_t, ignored);
    ++passes;
    if (finite6(xt) && finite(t) && t.v[0] < out.s.v[0]) {
      float step = 0.f;
      GBP_UNROLL
      for (int i = 0; i < 6; ++i) {
        const float a = fabsf(dx[i]);
        step = a > step ? a : step;
        out.x[i] = xt[i];
      }
      out.s = t;
      out.last_step = step;
      behind = behind_t;
      accepted = true;
      lam = lam / 10.f;
      lam = lam > 1e-9f ? lam : 1e-9f;
    } else {
      lam *= 10.f;
    }
  }
  out.lam = lam;
  out.status = status | (behind ? GBP_RESECT_BEHIND : 0u) | (accepted ? 0u : GBP_RESECT_STALLED);
}

// what one lane stores of camera c
GBP_DEV void store_camera(const Outputs& o, const Params& p, uint32_t c, const CameraResult& r) {
  o.status[c] = r.status;
  if (o.n_views) o.n_views[c] = r.n_views;
  if (!r.written) return;
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) o.cam_mean[6 * (size_t)c + i] = r.x[i];
  if (o.cam_info) {
    GBP_UNROLL
    for (int i = 0; i < 6; ++i) {
      GBP_UNROLL
      for (int j = 0; j < 6; ++j) o.cam_info[36 * (size_t)c + 6 * i + j] = r.s.v[i < j ? hidx(i, j) : hidx(j, i)] / p.reproj_meas_var;
    }
  }
  if (o.report) {
    o.report[4 * (size_t)c] = r.start_cost;
    o.report[4 * (size_t)c + 1] = r.s.v[0];
    o.report[4 * (size_t)c + 2] = r.last_step;
    o.report[4 * (size_t)c + 3] = r.lam;
  }
  if (o.cam_priors_eta) {
    GBP_UNROLL
    for (int i = 0; i < 6; ++i) {
      float s = 0.f;
      GBP_UNROLL
      for (int k = 0; k < 6; ++k) s += o.cam_priors_lambda[36 * (size_t)c + 6 * i + k] * r.x[k];
      o.cam_priors_eta[6 * (size_t)c + i] = s;
    }
  }
}

// the index range of camera c, clamped to the index; what the clamp had to do is flagged
GBP_DEV void camera_range(const uint32_t* cam_start, uint32_t c, uint32_t n_edges, uint32_t& k0, uint32_t& k1, uint32_t& status) {
  k0 = cam_start[c]; k1 = cam_start[c + 1]; status = 0u;
  if (k1 > n_edges) { k1 = n_edges; status = GBP_RESECT_BAD_INDEX; }
  if (k0 > k1) { k0 = k1; status = GBP_RESECT_BAD_INDEX; }
}

}  // namespace resect
}  // namespace gbp
