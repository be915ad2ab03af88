// The seeding arithmetic (gbp_poplar_amd/seed/seed_math.hpp) compiled for the HOST, on its own: the header the kernels of
// seed/gbp_seed.hip are built from, one call per camera / per landmark in place of one lane.  Built by tests/test_seed_cpu.py under
// ASan + UBSan (and plain by tests/test_gpu_seed.py, as the twin the device results are compared with); never loaded into python.
//
//   seed_math_main IN OUT [libm|device]
// IN  (binary, little endian): uint32 C, L, E, has_select; float min_parallax, fallback_depth, reproj_meas_var; uint32 refine_iters;
//     float cam_mean [6C]; uint32 cam_id [E], lmk_start [L + 1], lmk_edges [E]; float K [9], measurements [2E]; uint32 active_flag [E],
//     select [L]; then what the outputs hold BEFORE the call: float lmk_mean [3L], eta [3L], lambda [9L]; uint32 status [L], n_views [L]
// OUT: the five output arrays after the call, in that order (what gbp_seed_landmarks leaves in them).
// libm | device (default libm): whose sinf / cosf the camera rotation (eval_cam_rot) takes: the one operation of the chain
// IEEE 754 does not pin.  device = the twin of the GPU math library's algorithm in tests/sanitize/device_trig_twin.hpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

#include "device_trig_twin.hpp"
#include "host_twin_io.hpp"
#define sinf twin_sinf      // (behind <cmath> and the HIP headers, in front of the arithmetic: only eval_cam_rot calls them)
#define cosf twin_cosf
#include "../../gbp_poplar_amd/seed/seed_math.hpp"
#undef sinf
#undef cosf

int main(int argc, char** argv) {
  FILE* in = twin_open(argc, argv);
  if (!in) return 2;
  std::vector<uint32_t> dims, iters, cam_id, lmk_start, lmk_edges, active, select, status, n_views;
  std::vector<float> fopts, cam_mean, K, z, mean, eta, lambda;
  bool ok = get(in, dims, 4);
  const size_t C = ok ? dims[0] : 0, L = ok ? dims[1] : 0, E = ok ? dims[2] : 0;
  ok = ok && get(in, fopts, 3) && get(in, iters, 1) && get(in, cam_mean, 6 * C) && get(in, cam_id, E) && get(in, lmk_start, L + 1) &&
       get(in, lmk_edges, E) && get(in, K, 9) && get(in, z, 2 * E) && get(in, active, E) && get(in, select, L) && get(in, mean, 3 * L) &&
       get(in, eta, 3 * L) && get(in, lambda, 9 * L) && get(in, status, L) && get(in, n_views, L);
  if (!twin_read(in, ok, argv)) return 2;
  const bool has_select = dims[3] != 0;

  using namespace gbp::seed;
  std::vector<CamRec> recs(C);
  for (size_t c = 0; c < C; ++c) {
    float cm[6];
    for (int i = 0; i < 6; ++i) cm[i] = cam_mean[6 * c + i];
    cam_record(cm, recs[c]);
  }
  Params p;
  for (int i = 0; i < 9; ++i) p.K[i] = K[i];
  p.min_parallax = fopts[0]; p.fallback_depth = fopts[1]; p.reproj_meas_var = fopts[2]; p.refine_iters = iters[0];
  Graph g;
  g.n_cams = (uint32_t)C; g.n_edges = (uint32_t)E; g.cam_id = cam_id.data(); g.lmk_edges = lmk_edges.data(); g.cam_mean = cam_mean.data();
  g.meas = z.data(); g.active_flag = active.data(); g.recs = recs.data();
  for (size_t l = 0; l < L; ++l) {      // the body of k_seed_landmarks
    if (has_select && select[l] == 0u) continue;
    uint32_t k0 = lmk_start[l], k1 = lmk_start[l + 1], st = 0u;
    if (k1 > g.n_edges) { k1 = g.n_edges; st = GBP_SEED_BAD_INDEX; }
    if (k0 > k1) { k0 = k1; st = GBP_SEED_BAD_INDEX; }
    LandmarkSeed s;
    seed_landmark(g, p, k0, k1, st, s);
    status[l] = s.status;
    n_views[l] = s.n_views;
    if (s.status & GBP_SEED_NO_VIEW) continue;
    for (int i = 0; i < 3; ++i) { mean[3 * l + i] = s.mean[i]; eta[3 * l + i] = s.eta[i]; }
    for (int i = 0; i < 9; ++i) lambda[9 * l + i] = (i % 4 == 0) ? s.lam : 0.f;
  }
  FILE* out = twin_create(argv);
  if (!out) return 2;
  ok = put(out, mean) && put(out, eta) && put(out, lambda) && put(out, status) && put(out, n_views);
  return twin_done(out, ok, argv, "seed_math");
}
