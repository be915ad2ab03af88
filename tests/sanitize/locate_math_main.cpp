// The location arithmetic (gbp_poplar_amd/locate/locate_math.hpp) compiled for the HOST, on its own: the header the kernel of
// locate/gbp_locate.hip is built from, loops over 64 hypotheses and over the observations in place of one wavefront.  Built by
// tests/test_locate_cpu.py under ASan + UBSan (and plain by tests/test_gpu_locate.py, as the twin the device results are compared
// with); never loaded into python.
//
//   locate_math_main IN OUT [libm|device]
// IN  (binary, little endian): uint32 C, L, E, has (bit 0 select, 1 cam_edges, 2 active_flag, 3 lmk_use, 4 inlier; 8: SOLVER mode,
//     9: SAMPLING mode); uint32 rounds, min_inliers, seed; float inlier_px; uint32 lmk_id [E], cam_start [C + 1], cam_edges [E];
//     float K [9], lmk_mean [3L], measurements [2E]; uint32 active_flag [E], lmk_use [L], select [C]; then what the outputs hold BEFORE
//     the call: float cam_mean [6C]; uint32 inlier [E]; float report [4C]; uint32 status [C], n_views [C], n_inliers [C]
// OUT: the six output arrays after the call, in that order (what gbp_locate_cameras leaves in them).
// SOLVER mode (the three-point solver alone): IN is uint32 N, 0, 0, 256; float K [9]; float pixels [6N]; float points [9N].
//     OUT: uint32 n_solutions [N]; double R [36N]; double t [12N] (zero where there is no solution).
// SAMPLING mode: the ordinary input, then uint32 Q and Q x (seed, c, r, j).  OUT: uint32 Q x (1 if the hypothesis is not void, the
//     three offsets into the camera's index range).
// libm | device: whose sinf / cosf the arithmetic takes (the include pattern of the other twins; location itself calls neither: the
// rotation of its final pass is the linearisation's, whose sine and cosine are fp64 values rounded once).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

#include "device_trig_twin.hpp"
#include "host_twin_io.hpp"
#define sinf twin_sinf
#define cosf twin_cosf
#include "../../gbp_poplar_amd/locate/locate_math.hpp"
#undef sinf
#undef cosf

using namespace gbp::locate;

// the wavefront of the kernel as loops: hypothesis j is lane j; the scoring passes run over the index range
struct HostWave {
  const Graph& g;
  const Params& p;
  uint32_t c, k0, k1;
  uint32_t* inlier;
  Hyp h[kLanes];
  void count(uint32_t& n, bool& bad) {
    n = 0u;
    for (uint64_t k = k0; k < k1; ++k) {
      Obs o;
      load_obs(g, (uint32_t)k, o, bad);
      n += o.used ? 1u : 0u;
    }
  }
  void generate(uint32_t r) {
    for (uint32_t j = 0; j < (uint32_t)kLanes; ++j) hypothesis(g, p, c, r, j, k0, k1 - k0, h[j]);
  }
  bool candidate(uint32_t j, int s, Cand& cd) {
    if (h[j].n <= (uint32_t)s) return false;
    for (int i = 0; i < 9; ++i) cd.R[i] = h[j].v[12 * s + i];
    for (int i = 0; i < 3; ++i) cd.t[i] = h[j].v[12 * s + 9 + i];
    return true;
  }
  uint32_t score(const Cand& cd, float thr2) {
    uint32_t n = 0u;
    for (uint64_t k = k0; k < k1; ++k) {
      Obs o;
      bool ignored = false;
      load_obs(g, (uint32_t)k, o, ignored);
      n += o.used && agrees(cd, o, p.K, thr2) ? 1u : 0u;
    }
    return n;
  }
  void final_pass(const float (&x)[6], float thr2, uint32_t& n, float& sumsq) {
    CamLin cl;
    const float w[3] = {x[3], x[4], x[5]};
    cam_lin(w, cl);
    float part[kLanes];
    uint32_t cnt[kLanes];
    for (uint32_t j = 0; j < (uint32_t)kLanes; ++j) {
      part[j] = 0.f; cnt[j] = 0u;
      for (uint64_t k = (uint64_t)k0 + j; k < k1; k += kLanes) {
        Obs o;
        bool ignored = false;
        load_obs(g, (uint32_t)k, o, ignored);
        float err2 = 0.f;
        if (o.used && final_agrees(x, cl, o, p.K, thr2, err2)) { part[j] += err2; cnt[j] += 1u; }
      }
    }
    for (int s = kLanes / 2; s >= 1; s /= 2)
      for (int i = 0; i < s; ++i) { part[i] += part[i + s]; cnt[i] += cnt[i + s]; }
    sumsq = part[0];
    n = cnt[0];
  }
  void mark(const float (&x)[6], float thr2) {
    if (!inlier) return;
    CamLin cl;
    const float w[3] = {x[3], x[4], x[5]};
    cam_lin(w, cl);
    for (uint64_t k = k0; k < k1; ++k) {
      Obs o;
      bool ignored = false;
      load_obs(g, (uint32_t)k, o, ignored);
      float err2 = 0.f;
      if (o.used) inlier[o.e] = final_agrees(x, cl, o, p.K, thr2, err2) ? 1u : 0u;
    }
  }
};

static int solver_mode(FILE* in, size_t N, char** argv) {
  std::vector<float> K, px, pts;
  const bool ok = get(in, K, 9) && get(in, px, 6 * N) && get(in, pts, 9 * N);
  if (!twin_read(in, ok, argv)) return 2;
  float K9[9];
  for (int i = 0; i < 9; ++i) K9[i] = K[i];
  std::vector<uint32_t> nsol(N);
  std::vector<double> R(36 * N, 0.0), t(12 * N, 0.0);
  for (size_t q = 0; q < N; ++q) {
    double y[3][3], X[3][3], Rs[kMaxSol][9], ts[kMaxSol][3];
    for (int i = 0; i < 3; ++i) {
      bearing(K9, px[6 * q + 2 * i], px[6 * q + 2 * i + 1], y[i]);
      for (int k = 0; k < 3; ++k) X[i][k] = (double)pts[9 * q + 3 * i + k];
    }
    const int n = p3p(y, X, Rs, ts);
    nsol[q] = (uint32_t)n;
    for (int s = 0; s < n; ++s) {
      for (int i = 0; i < 9; ++i) R[36 * q + 9 * s + i] = Rs[s][i];
      for (int i = 0; i < 3; ++i) t[12 * q + 3 * s + i] = ts[s][i];
    }
  }
  FILE* out = twin_create(argv);
  if (!out) return 2;
  return twin_done(out, put(out, nsol) && put(out, R) && put(out, t), argv, "locate_math");
}

int main(int argc, char** argv) {
  FILE* in = twin_open(argc, argv);
  if (!in) return 2;
  std::vector<uint32_t> dims, uopts, lmk_id, cam_start, cam_edges, active, lmk_use, select, inlier, status, n_views, n_inliers, nq, queries;
  std::vector<float> fopts, K, lmk_mean, z, cam_mean, report;
  bool ok = get(in, dims, 4);
  if (ok && (dims[3] & 256u)) return solver_mode(in, dims[0], argv);
  const size_t C = ok ? dims[0] : 0, L = ok ? dims[1] : 0, E = ok ? dims[2] : 0;
  ok = ok && get(in, uopts, 3) && get(in, fopts, 1) && get(in, lmk_id, E) && get(in, cam_start, C + 1) && get(in, cam_edges, E) && get(in, K, 9) &&
       get(in, lmk_mean, 3 * L) && get(in, z, 2 * E) && get(in, active, E) && get(in, lmk_use, L) && get(in, select, C) &&
       get(in, cam_mean, 6 * C) && get(in, inlier, E) && get(in, report, 4 * C) && get(in, status, C) && get(in, n_views, C) && get(in, n_inliers, C);
  const uint32_t has = ok ? dims[3] : 0u;
  if (ok && (has & 512u)) ok = get(in, nq, 1) && get(in, queries, 4 * (size_t)nq[0]);
  if (!twin_read(in, ok, argv)) return 2;

  Params p;
  for (int i = 0; i < 9; ++i) p.K[i] = K[i];
  p.rounds = uopts[0]; p.min_inliers = uopts[1]; p.seed = uopts[2]; p.inlier_px = fopts[0];
  Graph g;
  g.n_lmks = (uint32_t)L; g.n_edges = (uint32_t)E; g.lmk_id = lmk_id.data(); g.cam_edges = (has & 2u) ? cam_edges.data() : nullptr;
  g.lmk_mean = lmk_mean.data(); g.meas = z.data(); g.active_flag = (has & 4u) ? active.data() : nullptr;
  g.lmk_use = (has & 8u) ? lmk_use.data() : nullptr;
  if (has & 512u) {
    std::vector<uint32_t> res(queries.size());
    for (size_t q = 0; q < nq[0]; ++q) {
      const uint32_t c = queries[4 * q + 1];
      uint32_t k0, k1, st, off[3];
      camera_range(cam_start.data(), c, g.n_edges, k0, k1, st);
      Obs o[3];
      res[4 * q] = sample_triple(g, queries[4 * q], c, queries[4 * q + 2], queries[4 * q + 3], k0, k1 - k0, o, off) ? 1u : 0u;
      for (int i = 0; i < 3; ++i) res[4 * q + 1 + i] = off[i];
    }
    FILE* out = twin_create(argv);
    if (!out) return 2;
    return twin_done(out, put(out, res), argv, "locate_math");
  }
  Outputs o;
  o.cam_mean = cam_mean.data(); o.inlier = (has & 16u) ? inlier.data() : nullptr; o.report = report.data(); o.status = status.data();
  o.n_views = n_views.data(); o.n_inliers = n_inliers.data();
  for (size_t c = 0; c < C; ++c) {      // the body of k_locate_cameras
    if ((has & 1u) && select[c] == 0u) continue;
    uint32_t k0, k1, st;
    camera_range(cam_start.data(), (uint32_t)c, g.n_edges, k0, k1, st);
    HostWave wave{g, p, (uint32_t)c, k0, k1, o.inlier, {}};
    CameraResult r;
    locate_camera(wave, p, st, r);
    store_camera(o, (uint32_t)c, r);
  }
  FILE* out = twin_create(argv);
  if (!out) return 2;
  ok = put(out, cam_mean) && put(out, inlier) && put(out, report) && put(out, status) && put(out, n_views) && put(out, n_inliers);
  return twin_done(out, ok, argv, "locate_math");
}
