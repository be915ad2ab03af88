// seed/gbp_seed.hip — libgbp_mi355x_seed.so (include/gbp_mi355x_seed.h): the seeding kernels and the exports that launch them.
// The arithmetic is seed_math.hpp's (shared with the host twin the tests compile); here are the mapping, the memory accesses and the
// argument checks.  Not on the iteration path: one call per start / per keyframe, on the caller's stream, nothing allocated, nothing
// waited for.
#include "../../include/gbp_mi355x_seed.h"
#include "../stateless/stateless_index.hpp"
#include "seed_math.hpp"

namespace gbp {
namespace seed {

// One lane per camera: its 64-byte record (rotation of the metric, translation, centre).  1 000 cameras make a 64 KB table that the
// landmark lanes gather from L2.
__global__ __launch_bounds__(256) void k_seed_cameras(uint32_t n_cams, const float* __restrict__ cam_mean, CamRec* __restrict__ recs) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cams) return;
  float cm[6];
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) cm[i] = cam_mean[(size_t)c * 6 + i];
  CamRec rec;
  cam_record(cm, rec);
  recs[c] = rec;
}

// One lane per landmark: the lane walks its own index range three to 3 + refine_iters times and keeps every sum in registers, in
// index order — the serial sums of the definition, whatever the launch.  A landmark's observations are scattered over the cameras'
// blocks of the file, so a lane group would share no load but the index entry; the camera records (64 B) and means (24 B) are gathered
// from L2.  Lanes of one wave differ in degree: a wave lasts as long as its largest landmark (profiles/seed_landmarks.md).
__global__ __launch_bounds__(256) void k_seed_landmarks(uint32_t n_lmks, Graph g, const uint32_t* __restrict__ lmk_start,
                                                        const uint32_t* __restrict__ select, const Params p, float* __restrict__ lmk_mean,
                                                        float* __restrict__ lmk_eta, float* __restrict__ lmk_lambda,
                                                        uint32_t* __restrict__ status, uint32_t* __restrict__ n_views) {
  const uint32_t l = blockIdx.x * 256 + threadIdx.x;
  if (l >= n_lmks) return;
  if (select && select[l] == 0u) return;
  uint32_t k0 = lmk_start[l], k1 = lmk_start[l + 1], st = 0u;
  if (k1 > g.n_edges) { k1 = g.n_edges; st = GBP_SEED_BAD_INDEX; }
  if (k0 > k1) { k0 = k1; st = GBP_SEED_BAD_INDEX; }
  LandmarkSeed s;
  seed_landmark(g, p, k0, k1, st, s);
  status[l] = s.status;
  if (n_views) n_views[l] = s.n_views;
  if (s.status & GBP_SEED_NO_VIEW) return;
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) lmk_mean[(size_t)l * 3 + i] = s.mean[i];
  if (lmk_eta) {
    GBP_UNROLL
    for (int i = 0; i < 3; ++i) lmk_eta[(size_t)l * 3 + i] = s.eta[i];
  }
  if (lmk_lambda) {
    GBP_UNROLL
    for (int i = 0; i < 9; ++i) lmk_lambda[(size_t)l * 9 + i] = (i % 4 == 0) ? s.lam : 0.f;
  }
}

// One lane: a 6 x 6 solve and six row dots.
__global__ __launch_bounds__(64) void k_seed_keyframe(uint32_t src, uint32_t dst, const float* __restrict__ cam_beliefs_eta,
                                                      const float* __restrict__ cam_beliefs_lambda, const float* __restrict__ cam_priors_lambda,
                                                      float* __restrict__ cam_priors_eta, float* __restrict__ cam_mean_out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float mu[6], eta[6];
  keyframe_prior(cam_beliefs_eta + (size_t)src * 6, cam_beliefs_lambda + (size_t)src * 36, cam_priors_lambda + (size_t)dst * 36, mu, eta);
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) cam_priors_eta[(size_t)dst * 6 + i] = eta[i];
  if (cam_mean_out) {
    GBP_UNROLL
    for (int i = 0; i < 6; ++i) cam_mean_out[i] = mu[i];
  }
}

static void defaults(gbp_seed_options& o) {
  o.min_parallax = 5e-3f;
  o.fallback_depth = 1.f;
  o.refine_iters = 2u;
  o.reproj_meas_var = 4.f;
}

}  // namespace seed
}  // namespace gbp

using namespace gbp::seed;
using namespace gbp::stateless;

GBP_STATELESS_EXPORT_T(int, 0, gbp_seed_abi_version, (void), ()) { return GBP_SEED_ABI_VERSION; }

GBP_STATELESS_EXPORT_T(const char*, "", gbp_seed_last_error, (void), ()) { return last_error().c_str(); }

GBP_STATELESS_EXPORT(gbp_seed_default_options, (gbp_seed_options* opts), (opts)) {
  if (!opts) return null_arg("gbp_seed_default_options", "opts");
  defaults(*opts);
  last_error().clear();
  return GBP_OK;
}

GBP_STATELESS_EXPORT(gbp_seed_index, (uint32_t n_lmks, uint32_t n_edges, const uint32_t* lmk_id, uint32_t* lmk_start, uint32_t* lmk_edges),
                (n_lmks, n_edges, lmk_id, lmk_start, lmk_edges)) {
  return build_index("gbp_seed_index", kLmkIndex, n_lmks, n_edges, lmk_id, lmk_start, lmk_edges);
}

GBP_STATELESS_EXPORT(gbp_seed_check_index, (uint32_t n_lmks, uint32_t n_edges, const uint32_t* lmk_start, const uint32_t* lmk_edges),
                (n_lmks, n_edges, lmk_start, lmk_edges)) {
  return check_index("gbp_seed_check_index", kLmkIndex, n_lmks, n_edges, lmk_start, lmk_edges, false);
}

GBP_STATELESS_EXPORT_T(size_t, 0, gbp_seed_workspace_bytes, (uint32_t n_cams), (n_cams)) { return sizeof(CamRec) * (size_t)n_cams; }

GBP_STATELESS_EXPORT(gbp_seed_landmarks,
                (void* hip_stream, uint32_t n_cams, uint32_t n_lmks, uint32_t n_edges, const uint32_t* cam_id, const uint32_t* lmk_start,
                 const uint32_t* lmk_edges, const float K[9], const float* cam_mean, const float* measurements, const uint32_t* active_flag,
                 const uint32_t* select, const gbp_seed_options* opts, void* workspace, float* lmk_mean, float* lmk_priors_eta,
                 float* lmk_priors_lambda, uint32_t* status, uint32_t* n_views),
                (hip_stream, n_cams, n_lmks, n_edges, cam_id, lmk_start, lmk_edges, K, cam_mean, measurements, active_flag, select, opts,
                 workspace, lmk_mean, lmk_priors_eta, lmk_priors_lambda, status, n_views)) {
  const char* fn = "gbp_seed_landmarks";
  if (!K) return null_arg(fn, "K");
  gbp_seed_options o;
  defaults(o);
  if (opts) o = *opts;
  if (const int rc = need_positive(fn, "opts.reproj_meas_var", o.reproj_meas_var)) return rc;
  if (const int rc = need_positive(fn, "opts.fallback_depth", o.fallback_depth)) return rc;
  if (const int rc = need_number(fn, "opts.min_parallax", o.min_parallax)) return rc;
  if (n_lmks) {
    if (!lmk_start) return null_arg(fn, "lmk_start");
    if (!lmk_mean) return null_arg(fn, "lmk_mean");
    if (!status) return null_arg(fn, "status");
  }
  if (n_edges) {
    if (!cam_id) return null_arg(fn, "cam_id");
    if (!lmk_edges) return null_arg(fn, "lmk_edges");
    if (!cam_mean) return null_arg(fn, "cam_mean");
    if (!measurements) return null_arg(fn, "measurements");
    if (n_cams == 0) return bad_arg(fn, "n_cams is 0 with n_edges > 0");
  }
  if (n_cams) {
    if (!cam_mean) return null_arg(fn, "cam_mean");
    if (!workspace) return null_arg(fn, "workspace");
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return bad_arg(fn, "workspace is not 16-byte aligned");
  }
  if ((uint64_t)n_lmks > kMaxLanes || (uint64_t)n_cams > kMaxLanes) return bad_arg(fn, "n_lmks or n_cams is too large");
  last_error().clear();
  if (n_lmks == 0) return GBP_OK;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  CamRec* recs = static_cast<CamRec*>(workspace);
  if (n_cams) {
    hipLaunchKernelGGL(k_seed_cameras, dim3((n_cams + 255) / 256), dim3(256), 0, s, n_cams, cam_mean, recs);
    if (const int rc = launched(fn)) return rc;
  }
  Params p;
  for (int i = 0; i < 9; ++i) p.K[i] = K[i];
  p.min_parallax = o.min_parallax; p.fallback_depth = o.fallback_depth; p.reproj_meas_var = o.reproj_meas_var; p.refine_iters = o.refine_iters;
  Graph g;
  g.n_cams = n_cams; g.n_edges = n_edges; g.cam_id = cam_id; g.lmk_edges = lmk_edges; g.cam_mean = cam_mean; g.meas = measurements;
  g.active_flag = active_flag; g.recs = recs;
  hipLaunchKernelGGL(k_seed_landmarks, dim3((n_lmks + 255) / 256), dim3(256), 0, s, n_lmks, g, lmk_start, select, p, lmk_mean, lmk_priors_eta,
                     lmk_priors_lambda, status, n_views);
  return launched(fn);
}

GBP_STATELESS_EXPORT(gbp_seed_keyframe,
                (void* hip_stream, uint32_t n_cams, uint32_t src, uint32_t dst, const float* cam_beliefs_eta, const float* cam_beliefs_lambda,
                 const float* cam_priors_lambda, float* cam_priors_eta, float* cam_mean_out),
                (hip_stream, n_cams, src, dst, cam_beliefs_eta, cam_beliefs_lambda, cam_priors_lambda, cam_priors_eta, cam_mean_out)) {
  const char* fn = "gbp_seed_keyframe";
  if (src >= n_cams) return bad_arg(fn, "src = " + std::to_string(src) + " is not below n_cams");
  if (dst >= n_cams) return bad_arg(fn, "dst = " + std::to_string(dst) + " is not below n_cams");
  if (!cam_beliefs_eta) return null_arg(fn, "cam_beliefs_eta");
  if (!cam_beliefs_lambda) return null_arg(fn, "cam_beliefs_lambda");
  if (!cam_priors_lambda) return null_arg(fn, "cam_priors_lambda");
  if (!cam_priors_eta) return null_arg(fn, "cam_priors_eta");
  last_error().clear();
  hipLaunchKernelGGL(k_seed_keyframe, dim3(1), dim3(64), 0, static_cast<hipStream_t>(hip_stream), src, dst, cam_beliefs_eta, cam_beliefs_lambda,
                     cam_priors_lambda, cam_priors_eta, cam_mean_out);
  return launched(fn);
}
