// The resection arithmetic (gbp_poplar_amd/resect/resect_math.hpp) compiled for the HOST, on its own: the header the kernel of
// resect/gbp_resect.hip is built from, one loop over 64 partials per camera in place of one wavefront.  Built by
// tests/test_resect_cpu.py under ASan + UBSan (and plain by tests/test_gpu_resect.py, as the twin the device results are compared
// with); never loaded into python.
//
//   resect_math_main IN OUT [libm|device]
// IN  (binary, little endian): uint32 C, L, E, has (bit 0 select, 1 cam_edges, 2 active_flag, 3 lmk_use, 4 cam_priors_lambda);
//     uint32 max_passes, min_views; float huber_px, lambda0, reproj_meas_var; uint32 lmk_id [E], cam_start [C + 1], cam_edges [E];
//     float K [9], lmk_mean [3L], measurements [2E]; uint32 active_flag [E], lmk_use [L], select [C]; float cam_priors_lambda [36C];
//     then what the outputs hold BEFORE the call: float cam_mean [6C] (the start poses), cam_priors_eta [6C], cam_info [36C],
//     report [4C]; uint32 status [C], n_views [C]
// OUT: the six output arrays after the call, in that order (what gbp_resect_cameras leaves in them).
// libm | device: whose sinf / cosf the arithmetic takes (the include pattern of the other twins; the resection itself calls neither:
// its rotation is the linearisation's, whose sine and cosine are fp64 values rounded once).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

#include "device_trig_twin.hpp"
#include "host_twin_io.hpp"
#define sinf twin_sinf
#define cosf twin_cosf
#include "../../gbp_poplar_amd/resect/resect_math.hpp"
#undef sinf
#undef cosf

using namespace gbp::resect;

// the wavefront of the kernel as a loop: partial j is lane j, the tree runs over the array
struct HostWave {
  const Graph& g;
  const Params& p;
  uint32_t k0, k1;
  void pass(const float (&x)[6], Sums& total, bool& behind, bool& bad) {
    CamLin cl;
    const float w[3] = {x[3], x[4], x[5]};
    cam_lin(w, cl);
    Sums part[kLanes];
    for (uint32_t j = 0; j < (uint32_t)kLanes; ++j) lane_pass(g, p, x, cl, k0, k1, j, part[j], behind, bad);
    for (int s = kLanes / 2; s >= 1; s /= 2)
      for (int i = 0; i < s; ++i) combine(part[i], part[i + s]);
    total = part[0];
  }
  void solve(const Sums& s, float lam, float (&dx)[6]) { lm_step(s, lam, dx); }
};

int main(int argc, char** argv) {
  FILE* in = twin_open(argc, argv);
  if (!in) return 2;
  std::vector<uint32_t> dims, uopts, lmk_id, cam_start, cam_edges, active, lmk_use, select, status, n_views;
  std::vector<float> fopts, K, lmk_mean, z, prior_lambda, cam_mean, eta, info, report;
  bool ok = get(in, dims, 4);
  const size_t C = ok ? dims[0] : 0, L = ok ? dims[1] : 0, E = ok ? dims[2] : 0;
  ok = ok && get(in, uopts, 2) && get(in, fopts, 3) && get(in, lmk_id, E) && get(in, cam_start, C + 1) && get(in, cam_edges, E) && get(in, K, 9) &&
       get(in, lmk_mean, 3 * L) && get(in, z, 2 * E) && get(in, active, E) && get(in, lmk_use, L) && get(in, select, C) &&
       get(in, prior_lambda, 36 * C) && get(in, cam_mean, 6 * C) && get(in, eta, 6 * C) && get(in, info, 36 * C) && get(in, report, 4 * C) &&
       get(in, status, C) && get(in, n_views, C);
  if (!twin_read(in, ok, argv)) return 2;
  const uint32_t has = dims[3];

  Params p;
  for (int i = 0; i < 9; ++i) p.K[i] = K[i];
  p.max_passes = uopts[0]; p.min_views = uopts[1]; p.huber_px = fopts[0]; p.lambda0 = fopts[1]; p.reproj_meas_var = fopts[2];
  Graph g;
  g.n_lmks = (uint32_t)L; g.n_edges = (uint32_t)E; g.lmk_id = lmk_id.data(); g.cam_edges = (has & 2u) ? cam_edges.data() : nullptr;
  g.lmk_mean = lmk_mean.data(); g.meas = z.data(); g.active_flag = (has & 4u) ? active.data() : nullptr;
  g.lmk_use = (has & 8u) ? lmk_use.data() : nullptr;
  Outputs o;
  o.cam_mean = cam_mean.data(); o.cam_priors_lambda = prior_lambda.data(); o.cam_priors_eta = (has & 16u) ? eta.data() : nullptr;
  o.cam_info = info.data(); o.report = report.data(); o.status = status.data(); o.n_views = n_views.data();
  for (size_t c = 0; c < C; ++c) {      // the body of k_resect_cameras
    if ((has & 1u) && select[c] == 0u) continue;
    uint32_t k0, k1, st;
    camera_range(cam_start.data(), (uint32_t)c, g.n_edges, k0, k1, st);
    float start[6];
    for (int i = 0; i < 6; ++i) start[i] = cam_mean[6 * c + i];
    HostWave wave{g, p, k0, k1};
    CameraResult r;
    resect_camera(wave, p, start, st, r);
    store_camera(o, p, (uint32_t)c, r);
  }
  FILE* out = twin_create(argv);
  if (!out) return 2;
  ok = put(out, cam_mean) && put(out, eta) && put(out, info) && put(out, report) && put(out, status) && put(out, n_views);
  return twin_done(out, ok, argv, "resect_math");
}
