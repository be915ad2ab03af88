// The solution readout's arithmetic (gbp_poplar_amd/post/post_math.hpp) compiled for the HOST, on its own: the header the kernels
// of post/gbp_post.hip are built from, one call per variable / per edge in place of one lane.  Built by tests/test_post_cpu.py under
// ASan + UBSan (and plain by tests/test_gpu_post.py, as the twin the device results are compared with); never loaded into python.
//
//   post_math_main IN OUT [libm|device]
// IN  (binary, little endian): uint32 C, L, E, want_cov; float cam_eta [6C], cam_lambda [36C], lmk_eta [3L], lmk_lambda [9L];
//     uint32 cam_id [E], lmk_id [E]; float K [9], measurements [2E]; uint32 active_flag [E]
// OUT: float cam_mean [6C], cam_cov [36C], lmk_mean [3L], lmk_cov [9L]; uint32 cam_status [C], lmk_status [L];
//     float residual [2E], reproj_cov [3E] (zeros without want_cov) — the residuals at the means and covariances just computed,
//     as gbp_post_residuals computes them from the output of gbp_post_moments.
// libm | device (default libm): whose sinf / cosf the rotation of the residual (eval_cam_rot) takes: the one operation of the chain
// IEEE 754 does not pin.  device = the twin of the GPU math library's algorithm in tests/sanitize/device_trig_twin.hpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

#include "device_trig_twin.hpp"
#include "host_twin_io.hpp"
#define sinf twin_sinf      // (behind <cmath> and the HIP headers, in front of the arithmetic: only eval_cam_rot calls them)
#define cosf twin_cosf
#include "../../gbp_poplar_amd/post/post_math.hpp"
#undef sinf
#undef cosf

int main(int argc, char** argv) {
  FILE* in = twin_open(argc, argv);
  if (!in) return 2;
  std::vector<uint32_t> dims, cam_id, lmk_id, active;
  std::vector<float> ce, cl, le, ll, K, z;
  bool ok = get(in, dims, 4);
  const size_t C = ok ? dims[0] : 0, L = ok ? dims[1] : 0, E = ok ? dims[2] : 0;
  ok = ok && get(in, ce, 6 * C) && get(in, cl, 36 * C) && get(in, le, 3 * L) && get(in, ll, 9 * L) && get(in, cam_id, E) && get(in, lmk_id, E) &&
       get(in, K, 9) && get(in, z, 2 * E) && get(in, active, E);
  if (!twin_read(in, ok, argv)) return 2;
  const bool want_cov = dims[3] != 0;

  std::vector<float> cm(6 * C), cc(36 * C), lm(3 * L), lc(9 * L), res(2 * E, 0.f), rc(3 * E, 0.f);
  std::vector<uint32_t> cs(C), ls(L);
  for (size_t c = 0; c < C; ++c) {
    float mean[6], cov[36];
    cs[c] = gbp::post::moments<6>(&cl[36 * c], &ce[6 * c], mean, cov);
    for (int i = 0; i < 6; ++i) cm[6 * c + i] = mean[i];
    for (int i = 0; i < 36; ++i) cc[36 * c + i] = cov[i];
  }
  for (size_t l = 0; l < L; ++l) {
    float mean[3], cov[9];
    ls[l] = gbp::post::moments<3>(&ll[9 * l], &le[3 * l], mean, cov);
    for (int i = 0; i < 3; ++i) lm[3 * l + i] = mean[i];
    for (int i = 0; i < 9; ++i) lc[9 * l + i] = cov[i];
  }
  float K9[9];
  for (int i = 0; i < 9; ++i) K9[i] = K[i];
  for (size_t e = 0; e < E; ++e) {
    if (active[e] == 0u) continue;
    const size_t c = cam_id[e], l = lmk_id[e];
    if (c >= C || l >= L) { std::fprintf(stderr, "edge %zu: index out of range\n", e); return 2; }
    float m6[6], m3[3], r[2], s[3], c36[36], c9[9];
    for (int i = 0; i < 6; ++i) m6[i] = cm[6 * c + i];
    for (int i = 0; i < 3; ++i) m3[i] = lm[3 * l + i];
    gbp::post::edge_residual(m6, m3, K9, z[2 * e], z[2 * e + 1], r);
    res[2 * e] = r[0]; res[2 * e + 1] = r[1];
    if (want_cov) {
      for (int i = 0; i < 36; ++i) c36[i] = cc[36 * c + i];
      for (int i = 0; i < 9; ++i) c9[i] = lc[9 * l + i];
      gbp::post::edge_reproj_cov(m6, m3, K9, c36, c9, s);
      for (int i = 0; i < 3; ++i) rc[3 * e + i] = s[i];
    }
  }
  FILE* out = twin_create(argv);
  if (!out) return 2;
  ok = put(out, cm) && put(out, cc) && put(out, lm) && put(out, lc) && put(out, cs) && put(out, ls) && put(out, res) && put(out, rc);
  return twin_done(out, ok, argv, "post_math");
}
