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
// libm | device (default libm): whose sinf / cosf the rotation of the residual (eval_cam_rot) takes.  They are the one operation of
// the chain that IEEE 754 does not pin: the host's libm and the GPU's math library both return a float within an ulp or so of the true
// value, not always the same one (measured: cosf one ulp apart for two of six test cameras).  "libm" is what gbp_eval_host calls, so
// the CPU tests compare like with like; "device" evaluates the GPU library's own algorithm for |x| < 2^17 — a three-term Cody-Waite
// reduction by pi/2 and two short polynomials, every multiply-add fused, as the gfx950 code object of the kernels does it (read from
// the compiler's output for sinf / cosf) — in IEEE operations that give the same bits on any host: the twin the GPU tests compare with.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

static bool g_device_trig = false;
static uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float float_of(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static float f64(uint64_t u) { double d; std::memcpy(&d, &u, 8); return (float)d; }      // (the constants: doubles that are exact floats)
// r = |x| - n pi/2 with n = rint(|x| 2/pi); sin and cos of r by their polynomials
static void device_sincos_reduced(float ax, int& n, float& s, float& c) {
  const float fn = std::rint(ax * f64(0x3FE45F3060000000ull));
  float r = std::fmaf(fn, f64(0xBFF921FB40000000ull), ax);
  r = std::fmaf(fn, f64(0xBE74442D00000000ull), r);
  r = std::fmaf(fn, f64(0xBCF8469880000000ull), r);
  n = (int)fn;
  const float t = r * r;
  float a = std::fmaf(t, f64(0xBF29833040000000ull), f64(0x3F81103880000000ull));
  a = std::fmaf(t, a, f64(0xBFC55553A0000000ull));
  s = std::fmaf(r, t * a, r);
  float b = std::fmaf(t, f64(0x3EFAEA6680000000ull), f64(0xBF56C9E760000000ull));
  b = std::fmaf(t, b, f64(0x3FA5557EE0000000ull));
  b = std::fmaf(t, b, f64(0xBFE0000080000000ull));
  c = std::fmaf(t, b, 1.0f);
}
static float twin_sinf(float x) {
  const float ax = std::fabs(x);
  if (!g_device_trig || !(ax < 131072.0f)) return sinf(x);      // (beyond 2^17 the library reduces with a table of 2/pi: no rotation vector gets there)
  int n;
  float s, c;
  device_sincos_reduced(ax, n, s, c);
  return float_of(bits_of((n & 1) ? c : s) ^ (((uint32_t)n << 30) & 0x80000000u) ^ (bits_of(ax) ^ bits_of(x)));
}
static float twin_cosf(float x) {
  const float ax = std::fabs(x);
  if (!g_device_trig || !(ax < 131072.0f)) return cosf(x);
  int n;
  float s, c;
  device_sincos_reduced(ax, n, s, c);
  return float_of(bits_of((n & 1) ? -s : c) ^ (((uint32_t)n << 30) & 0x80000000u));
}
#define sinf twin_sinf      // (behind <cmath> and the HIP headers, in front of the arithmetic: only eval_cam_rot calls them)
#define cosf twin_cosf
#include "../../gbp_poplar_amd/post/post_math.hpp"
#undef sinf
#undef cosf

template <class T> static bool get(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <class T> static bool put(FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) { std::fprintf(stderr, "usage: %s IN OUT [libm|device]\n", argv[0]); return 2; }
  if (argc == 4) {
    if (std::strcmp(argv[3], "device") != 0 && std::strcmp(argv[3], "libm") != 0) { std::fprintf(stderr, "unknown trig mode %s\n", argv[3]); return 2; }
    g_device_trig = std::strcmp(argv[3], "device") == 0;
  }
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::vector<uint32_t> dims, cam_id, lmk_id, active;
  std::vector<float> ce, cl, le, ll, K, z;
  bool ok = get(in, dims, 4);
  const size_t C = ok ? dims[0] : 0, L = ok ? dims[1] : 0, E = ok ? dims[2] : 0;
  ok = ok && get(in, ce, 6 * C) && get(in, cl, 36 * C) && get(in, le, 3 * L) && get(in, ll, 9 * L) && get(in, cam_id, E) && get(in, lmk_id, E) &&
       get(in, K, 9) && get(in, z, 2 * E) && get(in, active, E);
  std::fclose(in);
  if (!ok) { std::fprintf(stderr, "%s is truncated\n", argv[1]); return 2; }
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
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  ok = put(out, cm) && put(out, cc) && put(out, lm) && put(out, lc) && put(out, cs) && put(out, ls) && put(out, res) && put(out, rc);
  if (std::fclose(out) != 0 || !ok) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  std::printf("post_math: ok\n");
  return 0;
}
