// The GPU math library's sinf / cosf for |x| < 2^17, restated in IEEE operations: the only copy, for both host twins
// (post_math_main.cpp, seed_math_main.cpp).  sinf / cosf are the one operation of eval_cam_rot that IEEE 754 does not pin: the host's
// libm and the GPU's math library both return a float within an ulp or so of the true value, not always the same one (measured: cosf one
// ulp apart for two of six test cameras).  Without g_device_trig, twin_sinf / twin_cosf are the host libm's — what gbp_eval_host calls,
// so the CPU tests compare like with like.  With it they evaluate the GPU library's own algorithm — a three-term Cody-Waite reduction
// by pi/2 and two short polynomials, every multiply-add fused, as the gfx950 code object of the kernels does it (read from the
// compiler's output for sinf / cosf) — in IEEE operations that give the same bits on any host: the twin the GPU tests compare with.
// Include it behind <cmath> and the HIP headers, then `#define sinf twin_sinf` / `#define cosf twin_cosf` around the arithmetic header.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

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
