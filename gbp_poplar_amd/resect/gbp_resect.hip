// resect/gbp_resect.hip — libgbp_mi355x_resect.so (include/gbp_mi355x_resect.h): the resection kernel and the exports that launch it.
// The arithmetic is resect_math.hpp's (shared with the host twin the tests compile); here are the mapping, the cross-lane tree, the
// memory accesses and the argument checks.  Not on the iteration path: one call per keyframe, on the caller's stream, nothing
// allocated, nothing waited for.
#include "../../include/gbp_mi355x_resect.h"
#include "../stateless/stateless_index.hpp"
#include "../stateless/stateless_wave.hpp"
#include "resect_call.hpp"

namespace gbp {
namespace resect {
using stateless::kWavesPerBlock;      // cameras per workgroup
using stateless::lane0;

// lane i reads lane i + n of its own DPP row of 16 (n = 8, 4, 2, 1; a lane past the row's end keeps its value, which the tree never uses)
template <int N> GBP_DEV int row_shl(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x100 + N, 0xF, 0xF, false); }
template <int N> GBP_DEV float row_shl(float v) { return __int_as_float(row_shl<N>(__float_as_int(v))); }

// The halving tree of the definition across the 64 lanes: after step s, lanes i < s hold partial i + partial i + s.  Lane 0 ends
// with the total; what the other lanes end with is not used.  32 and 16 cross DPP rows (a shuffle through the LDS crossbar), from 8 on
// the lanes that still matter read inside their own row (a row shift).  Same operands, same additions.
GBP_DEV void tree(Sums& s) {
  GBP_UNROLL
  for (int i = 0; i < kSums; ++i) {
    float v = s.v[i];
    v += __shfl_down(v, 32);
    v += __shfl_down(v, 16);
    v += row_shl<8>(v);
    v += row_shl<4>(v);
    v += row_shl<2>(v);
    v += row_shl<1>(v);
    s.v[i] = lane0(v);
  }
  int n = (int)s.n;
  n += __shfl_down(n, 32);
  n += __shfl_down(n, 16);
  n += row_shl<8>(n);
  n += row_shl<4>(n);
  n += row_shl<2>(n);
  n += row_shl<1>(n);
  s.n = (uint32_t)__builtin_amdgcn_readfirstlane(n);
}

// One wavefront = one camera: the 64 partials of the definition are the lanes, their 28 accumulators and the count stay in registers.
// Every lane computes cam_lin of the pose of a pass itself (the same operations on the same operands); the totals are lane 0's,
// broadcast, so every decision of resect_camera is the whole wave's.
struct DeviceWave {
  const Graph& g;
  const Params& p;
  uint32_t k0, k1, lane;
  GBP_DEV void pass(const float (&x)[6], Sums& total, bool& behind, bool& bad) {
    CamLin cl;
    const float w[3] = {x[3], x[4], x[5]};
    cam_lin(w, cl);
    bool b = false, d = false;
    lane_pass(g, p, x, cl, k0, k1, lane, total, b, d);
    tree(total);
    behind = behind || __builtin_amdgcn_ballot_w64(b) != 0ull;
    bad = bad || __builtin_amdgcn_ballot_w64(d) != 0ull;
  }
  GBP_DEV void solve(const Sums& s, float lam, float (&dx)[6]) {
    GBP_UNROLL
    for (int i = 0; i < 6; ++i) dx[i] = 0.f;
    if (lane == 0u) lm_step(s, lam, dx);
    GBP_UNROLL
    for (int i = 0; i < 6; ++i) dx[i] = lane0(dx[i]);
  }
};

__global__ __launch_bounds__(64 * kWavesPerBlock) void k_resect_cameras(uint32_t n_cams, Graph g, const uint32_t* __restrict__ cam_start,
                                                                        const uint32_t* __restrict__ select, const Params p, Outputs o) {
  const uint32_t c = stateless::wave_item();
  if (c >= n_cams) return;                        // (the whole wave)
  if (select && select[c] == 0u) return;
  uint32_t k0, k1, st;
  camera_range(cam_start, c, g.n_edges, k0, k1, st);
  float start[6];
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) start[i] = o.cam_mean[6 * (size_t)c + i];
  DeviceWave wave{g, p, k0, k1, threadIdx.x & 63u};
  CameraResult r;
  resect_camera(wave, p, start, st, r);
  if (wave.lane == 0u) store_camera(o, p, c, r);
}

static void defaults(gbp_resect_options& o) {
  o.max_passes = 10u;
  o.min_views = 6u;
  o.huber_px = 5.f;
  o.lambda0 = 1e-3f;
  o.reproj_meas_var = 4.f;
}

}  // namespace resect
}  // namespace gbp

using namespace gbp::resect;
using namespace gbp::stateless;

GBP_STATELESS_EXPORT_T(int, 0, gbp_resect_abi_version, (void), ()) { return GBP_RESECT_ABI_VERSION; }

GBP_STATELESS_EXPORT_T(const char*, "", gbp_resect_last_error, (void), ()) { return last_error().c_str(); }

GBP_STATELESS_EXPORT(gbp_resect_default_options, (gbp_resect_options* opts), (opts)) {
  if (!opts) return null_arg("gbp_resect_default_options", "opts");
  defaults(*opts);
  last_error().clear();
  return GBP_OK;
}

GBP_STATELESS_EXPORT(gbp_resect_index, (uint32_t n_cams, uint32_t n_edges, const uint32_t* cam_id, uint32_t* cam_start, uint32_t* cam_edges),
                (n_cams, n_edges, cam_id, cam_start, cam_edges)) {
  return build_index("gbp_resect_index", kCamIndex, n_cams, n_edges, cam_id, cam_start, cam_edges);
}

GBP_STATELESS_EXPORT(gbp_resect_check_index, (uint32_t n_cams, uint32_t n_edges, const uint32_t* cam_start, const uint32_t* cam_edges),
                (n_cams, n_edges, cam_start, cam_edges)) {
  return check_index("gbp_resect_check_index", kCamIndex, n_cams, n_edges, cam_start, cam_edges, true);
}

GBP_STATELESS_EXPORT(gbp_resect_cameras,
                (void* hip_stream, uint32_t n_cams, uint32_t n_lmks, uint32_t n_edges, const uint32_t* lmk_id, const uint32_t* cam_start,
                 const uint32_t* cam_edges, const float K[9], const float* lmk_mean, const float* measurements, const uint32_t* active_flag,
                 const uint32_t* lmk_use, const uint32_t* select, const gbp_resect_options* opts, float* cam_mean, const float* cam_priors_lambda,
                 float* cam_priors_eta, float* cam_info, float* report, uint32_t* status, uint32_t* n_views),
                (hip_stream, n_cams, n_lmks, n_edges, lmk_id, cam_start, cam_edges, K, lmk_mean, measurements, active_flag, lmk_use, select, opts,
                 cam_mean, cam_priors_lambda, cam_priors_eta, cam_info, report, status, n_views)) {
  const char* fn = "gbp_resect_cameras";
  gbp_resect_options o;
  defaults(o);
  if (opts) o = *opts;
  if (o.max_passes == 0u) return bad_arg(fn, "opts.max_passes is 0");
  if (o.min_views < 3u) return bad_arg(fn, "opts.min_views is below 3");
  if (const int rc = need_number(fn, "opts.huber_px", o.huber_px)) return rc;
  if (const int rc = need_positive(fn, "opts.lambda0", o.lambda0)) return rc;
  if (const int rc = need_positive(fn, "opts.reproj_meas_var", o.reproj_meas_var)) return rc;
  if (n_cams) {
    if (const int rc = check_cameras(fn, K, cam_start, cam_mean, status)) return rc;
    if (cam_priors_eta && !cam_priors_lambda) return bad_arg(fn, "cam_priors_eta without cam_priors_lambda");
    if (n_edges)
      if (const int rc = check_edges(fn, n_lmks, lmk_id, lmk_mean, measurements)) return rc;
  }
  last_error().clear();
  if (n_cams == 0) return GBP_OK;
  Params p;
  for (int i = 0; i < 9; ++i) p.K[i] = K[i];
  p.huber_px = o.huber_px; p.lambda0 = o.lambda0; p.reproj_meas_var = o.reproj_meas_var; p.max_passes = o.max_passes; p.min_views = o.min_views;
  const Graph g = graph_of(n_lmks, n_edges, lmk_id, cam_edges, lmk_mean, measurements, active_flag, lmk_use);
  Outputs out;
  out.cam_mean = cam_mean; out.cam_priors_lambda = cam_priors_lambda; out.cam_priors_eta = cam_priors_eta; out.cam_info = cam_info;
  out.report = report; out.status = status; out.n_views = n_views;
  hipLaunchKernelGGL(k_resect_cameras, wave_grid(n_cams), dim3(64 * kWavesPerBlock), 0, static_cast<hipStream_t>(hip_stream), n_cams, g,
                     cam_start, select, p, out);
  return launched(fn);
}
