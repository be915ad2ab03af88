// locate/gbp_locate.hip — libgbp_mi355x_locate.so (include/gbp_mi355x_locate.h): the location kernel and the exports that launch it.
// The arithmetic is locate_math.hpp's (shared with the host twin the tests compile); here are the mapping, the broadcasts, the
// memory accesses and the argument checks.  Not on the iteration path: one call per keyframe, on the caller's stream, nothing
// allocated, nothing waited for.
#include "../../include/gbp_mi355x_locate.h"
#include "../resect/resect_call.hpp"
#include "../stateless/stateless_wave.hpp"
#include "locate_math.hpp"

namespace gbp {
namespace locate {
using stateless::kWavesPerBlock;      // cameras per workgroup
using stateless::lane0;

GBP_DEV float from_lane(float v, uint32_t j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)j)); }
GBP_DEV uint32_t votes(bool b) { return (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(b)); }

// One wavefront = one camera.  Generating: lane j solves hypothesis (r, j) in fp64 and keeps its up to four candidates (48 floats) in
// registers.  Scoring: candidate (j, s) is read out of lane j into scalars (s is unrolled, j is the loop counter: whether it exists
// is the whole wave's branch), lane i tests the observations k0 + i, k0 + i + 64, ...; the count is the population of the ballot.
// While the index range has at most 64 entries every lane keeps its one observation in registers across all candidates; beyond that
// the observations are read again per candidate (the L2 holds a camera's few kilobytes).
struct DeviceWave {
  const Graph& g;
  const Params& p;
  uint32_t c, k0, k1, lane;
  Hyp h;
  Obs mine;
  bool resident;
  uint32_t* inlier;
  GBP_DEV void count(uint32_t& n, bool& bad) {
    uint32_t total = 0u;
    bool b = false;
    resident = k1 - k0 <= (uint32_t)kLanes;
    mine.used = false; mine.e = 0u; mine.l = 0xffffffffu;
    mine.z0 = mine.z1 = mine.X0 = mine.X1 = mine.X2 = 0.f;
    for (uint64_t base = k0; base < k1; base += kLanes) {      // (base is the whole wave's: so is every ballot)
      const uint64_t k = base + lane;
      Obs o;
      o.used = false;
      if (k < k1) load_obs(g, (uint32_t)k, o, b);
      total += votes(o.used);
      if (base == k0 && k < k1) mine = o;
    }
    n = total;
    bad = bad || __builtin_amdgcn_ballot_w64(b) != 0ull;
  }
  GBP_DEV void generate(uint32_t r) { hypothesis(g, p, c, r, lane, k0, k1 - k0, h); }
  GBP_DEV bool candidate(uint32_t j, int s, Cand& cd) {
    const uint32_t n = (uint32_t)__builtin_amdgcn_readlane((int)h.n, (int)j);
    if (n <= (uint32_t)s) return false;
    GBP_UNROLL
    for (int i = 0; i < 9; ++i) cd.R[i] = from_lane(h.v[12 * s + i], j);
    GBP_UNROLL
    for (int i = 0; i < 3; ++i) cd.t[i] = from_lane(h.v[12 * s + 9 + i], j);
    return true;
  }
  GBP_DEV uint32_t score(const Cand& cd, float thr2) {
    if (resident) return votes(agrees(cd, mine, p.K, thr2));
    uint32_t total = 0u;
    for (uint64_t base = k0; base < k1; base += kLanes) {
      const uint64_t k = base + lane;
      Obs o;
      o.used = false;
      bool ignored = false;
      if (k < k1) load_obs(g, (uint32_t)k, o, ignored);
      total += votes(o.used && agrees(cd, o, p.K, thr2));
    }
    return total;
  }
  // the final pass over this lane's entries: fn(observation, inlier, err2)
  template <class F> GBP_DEV void final_each(const float (&x)[6], float thr2, F&& fn) {
    CamLin cl;
    const float w[3] = {x[3], x[4], x[5]};
    cam_lin(w, cl);
    for (uint64_t k = (uint64_t)k0 + lane; k < k1; k += kLanes) {
      Obs o;
      bool ignored = false;
      load_obs(g, (uint32_t)k, o, ignored);
      if (!o.used) continue;
      float err2 = 0.f;
      const bool in = final_agrees(x, cl, o, p.K, thr2, err2);
      fn(o, in, err2);
    }
  }
  GBP_DEV void final_pass(const float (&x)[6], float thr2, uint32_t& n, float& sumsq) {
    float s = 0.f;
    int m = 0;
    final_each(x, thr2, [&](const Obs&, bool in, float err2) {
      if (in) { s += err2; m += 1; }
    });
    GBP_UNROLL
    for (int d = 32; d >= 1; d /= 2) {      // the halving tree: after step d, lanes i < d hold partial i + partial i + d
      s += __shfl_down(s, d);
      m += __shfl_down(m, d);
    }
    sumsq = lane0(s);
    n = (uint32_t)__builtin_amdgcn_readfirstlane(m);
  }
  GBP_DEV void mark(const float (&x)[6], float thr2) {
    if (!inlier) return;
    final_each(x, thr2, [&](const Obs& o, bool in, float) { inlier[o.e] = in ? 1u : 0u; });
  }
};

__global__ __launch_bounds__(64 * kWavesPerBlock) void k_locate_cameras(uint32_t n_cams, Graph g, const uint32_t* __restrict__ cam_start,
                                                                        const uint32_t* __restrict__ select, const Params p, Outputs o) {
  const uint32_t c = stateless::wave_item();
  if (c >= n_cams) return;                        // (the whole wave)
  if (select && select[c] == 0u) return;
  uint32_t k0, k1, st;
  camera_range(cam_start, c, g.n_edges, k0, k1, st);
  DeviceWave wave{g, p, c, k0, k1, threadIdx.x & 63u, {}, {}, false, o.inlier};
  CameraResult r;
  locate_camera(wave, p, st, r);
  if (wave.lane == 0u) store_camera(o, c, r);
}

static void defaults(gbp_locate_options& o) {
  o.rounds = 4u;
  o.min_inliers = 6u;
  o.inlier_px = 5.f;
  o.seed = 0u;
}

}  // namespace locate
}  // namespace gbp

using namespace gbp::locate;
using namespace gbp::stateless;

GBP_STATELESS_EXPORT_T(int, 0, gbp_locate_abi_version, (void), ()) { return GBP_LOCATE_ABI_VERSION; }

GBP_STATELESS_EXPORT_T(const char*, "", gbp_locate_last_error, (void), ()) { return last_error().c_str(); }

GBP_STATELESS_EXPORT(gbp_locate_default_options, (gbp_locate_options* opts), (opts)) {
  if (!opts) return null_arg("gbp_locate_default_options", "opts");
  defaults(*opts);
  last_error().clear();
  return GBP_OK;
}

GBP_STATELESS_EXPORT(gbp_locate_cameras,
                (void* hip_stream, uint32_t n_cams, uint32_t n_lmks, uint32_t n_edges, const uint32_t* lmk_id, const uint32_t* cam_start,
                 const uint32_t* cam_edges, const float K[9], const float* lmk_mean, const float* measurements, const uint32_t* active_flag,
                 const uint32_t* lmk_use, const uint32_t* select, const gbp_locate_options* opts, float* cam_mean, uint32_t* inlier, float* report,
                 uint32_t* status, uint32_t* n_views, uint32_t* n_inliers),
                (hip_stream, n_cams, n_lmks, n_edges, lmk_id, cam_start, cam_edges, K, lmk_mean, measurements, active_flag, lmk_use, select, opts,
                 cam_mean, inlier, report, status, n_views, n_inliers)) {
  const char* fn = "gbp_locate_cameras";
  gbp_locate_options o;
  defaults(o);
  if (opts) o = *opts;
  if (o.rounds == 0u) return bad_arg(fn, "opts.rounds is 0");
  if (o.rounds > 4096u) return bad_arg(fn, "opts.rounds is above 4096");
  if (o.min_inliers < 4u) return bad_arg(fn, "opts.min_inliers is below 4");
  if (const int rc = need_positive(fn, "opts.inlier_px", o.inlier_px)) return rc;
  if (n_cams) {
    if (const int rc = gbp::resect::check_cameras(fn, K, cam_start, cam_mean, status)) return rc;
    if (n_edges)
      if (const int rc = gbp::resect::check_edges(fn, n_lmks, lmk_id, lmk_mean, measurements)) return rc;
  }
  last_error().clear();
  if (n_cams == 0) return GBP_OK;
  Params p;
  for (int i = 0; i < 9; ++i) p.K[i] = K[i];
  p.inlier_px = o.inlier_px; p.rounds = o.rounds; p.min_inliers = o.min_inliers; p.seed = o.seed;
  const Graph g = gbp::resect::graph_of(n_lmks, n_edges, lmk_id, cam_edges, lmk_mean, measurements, active_flag, lmk_use);
  Outputs out;
  out.cam_mean = cam_mean; out.inlier = inlier; out.report = report; out.status = status; out.n_views = n_views; out.n_inliers = n_inliers;
  hipLaunchKernelGGL(k_locate_cameras, wave_grid(n_cams), dim3(64 * kWavesPerBlock), 0, static_cast<hipStream_t>(hip_stream), n_cams, g,
                     cam_start, select, p, out);
  return launched(fn);
}
