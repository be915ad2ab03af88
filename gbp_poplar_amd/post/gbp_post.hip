// post/gbp_post.hip — libgbp_mi355x_post.so (include/gbp_mi355x_post.h): the two readout kernels and the exports that launch them.
// The arithmetic is post_math.hpp's (shared with the host twin the tests compile); here are the mapping, the memory accesses and
// the argument checks.  Not on the iteration path: one launch per call, on the caller's stream, nothing allocated, nothing waited for.
#include "../../include/gbp_mi355x_post.h"
#include "../stateless/stateless_export.hpp"
#include "post_math.hpp"

namespace gbp {
namespace post {

struct K9 { float k[9]; };      // the pin-hole matrix, by value in the kernel arguments

// One lane per variable, cameras first (the mapping of k_means).  The 6 x 13 fp64 tableau of moments<6> lives in registers
// (profiles/post_readout.md: no scratch); a lane's loads and stores are its variable's contiguous record.
__global__ __launch_bounds__(256) void k_post_moments(uint32_t n_cams, uint32_t n_lmks, const float* __restrict__ cam_eta,
                                                      const float* __restrict__ cam_lambda, const float* __restrict__ lmk_eta,
                                                      const float* __restrict__ lmk_lambda, float* __restrict__ cam_mean,
                                                      float* __restrict__ cam_cov, float* __restrict__ lmk_mean, float* __restrict__ lmk_cov,
                                                      uint32_t* __restrict__ cam_status, uint32_t* __restrict__ lmk_status) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t < n_cams) {
    float lam[36], eta[6], mean[6], cov[36];
    GBP_UNROLL
    for (int i = 0; i < 36; ++i) lam[i] = cam_lambda[(size_t)t * 36 + i];
    GBP_UNROLL
    for (int i = 0; i < 6; ++i) eta[i] = cam_eta[(size_t)t * 6 + i];
    const uint32_t st = moments<6>(lam, eta, mean, cov);
    if (cam_mean) {
      GBP_UNROLL
      for (int i = 0; i < 6; ++i) cam_mean[(size_t)t * 6 + i] = mean[i];
    }
    if (cam_cov) {
      GBP_UNROLL
      for (int i = 0; i < 36; ++i) cam_cov[(size_t)t * 36 + i] = cov[i];
    }
    if (cam_status) cam_status[t] = st;
  } else if (t - n_cams < n_lmks) {
    const uint32_t l = t - n_cams;
    float lam[9], eta[3], mean[3], cov[9];
    GBP_UNROLL
    for (int i = 0; i < 9; ++i) lam[i] = lmk_lambda[(size_t)l * 9 + i];
    GBP_UNROLL
    for (int i = 0; i < 3; ++i) eta[i] = lmk_eta[(size_t)l * 3 + i];
    const uint32_t st = moments<3>(lam, eta, mean, cov);
    if (lmk_mean) {
      GBP_UNROLL
      for (int i = 0; i < 3; ++i) lmk_mean[(size_t)l * 3 + i] = mean[i];
    }
    if (lmk_cov) {
      GBP_UNROLL
      for (int i = 0; i < 9; ++i) lmk_cov[(size_t)l * 9 + i] = cov[i];
    }
    if (lmk_status) lmk_status[l] = st;
  }
}

// One lane per edge, in file order: the edges are sorted by camera, so the 64 lanes of a wave read one or two camera records
// (mean 24 bytes, covariance 144 bytes) that stay in cache while the landmark records are gathered.  The camera covariance is nine
// 16-byte loads where its base allows (a record is 144 bytes, so every record is then aligned), 4-byte loads otherwise.
// An edge whose camera or landmark index is out of range touches nothing and writes NaN.
template <bool COV>
__global__ __launch_bounds__(256) void k_post_residuals(uint32_t n_cams, uint32_t n_lmks, uint32_t n_edges, const uint32_t* __restrict__ cam_id,
                                                        const uint32_t* __restrict__ lmk_id, const K9 K, const float* __restrict__ cam_mean,
                                                        const float* __restrict__ lmk_mean, const float* __restrict__ meas,
                                                        const uint32_t* __restrict__ active_flag, const float* __restrict__ cam_cov,
                                                        const float* __restrict__ lmk_cov, int cov16, float* __restrict__ residual,
                                                        float* __restrict__ reproj_cov) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_edges) return;
  float r[2] = {0.f, 0.f}, s[3] = {0.f, 0.f, 0.f};
  if (!active_flag || active_flag[e] != 0u) {
    const uint32_t c = cam_id[e], l = lmk_id[e];
    if (c < n_cams && l < n_lmks) {
      float cm[6], lm[3];
      GBP_UNROLL
      for (int i = 0; i < 6; ++i) cm[i] = cam_mean[(size_t)c * 6 + i];
      GBP_UNROLL
      for (int i = 0; i < 3; ++i) lm[i] = lmk_mean[(size_t)l * 3 + i];
      edge_residual(cm, lm, K.k, meas[(size_t)e * 2], meas[(size_t)e * 2 + 1], r);
      if (COV) {
        float cc[36], cl[9];
        if (cov16) {
          const float4* q = reinterpret_cast<const float4*>(cam_cov) + (size_t)c * 9;
          GBP_UNROLL
          for (int i = 0; i < 9; ++i) {
            const float4 v = q[i];
            cc[4 * i] = v.x; cc[4 * i + 1] = v.y; cc[4 * i + 2] = v.z; cc[4 * i + 3] = v.w;
          }
        } else {
          GBP_UNROLL
          for (int i = 0; i < 36; ++i) cc[i] = cam_cov[(size_t)c * 36 + i];
        }
        GBP_UNROLL
        for (int i = 0; i < 9; ++i) cl[i] = lmk_cov[(size_t)l * 9 + i];
        edge_reproj_cov(cm, lm, K.k, cc, cl, s);
      }
    } else {
      const float nan = __builtin_nanf("");
      r[0] = r[1] = s[0] = s[1] = s[2] = nan;
    }
  }
  residual[(size_t)e * 2] = r[0];
  residual[(size_t)e * 2 + 1] = r[1];
  if (COV) {
    GBP_UNROLL
    for (int i = 0; i < 3; ++i) reproj_cov[(size_t)e * 3 + i] = s[i];
  }
}

}  // namespace post
}  // namespace gbp

using namespace gbp::post;
using namespace gbp::stateless;

GBP_STATELESS_EXPORT_T(int, 0, gbp_post_abi_version, (void), ()) { return GBP_POST_ABI_VERSION; }

GBP_STATELESS_EXPORT_T(const char*, "", gbp_post_last_error, (void), ()) { return last_error().c_str(); }

GBP_STATELESS_EXPORT(gbp_post_moments,
                (void* hip_stream, uint32_t n_cams, uint32_t n_lmks, const float* cam_eta, const float* cam_lambda, const float* lmk_eta,
                 const float* lmk_lambda, float* cam_mean, float* cam_cov, float* lmk_mean, float* lmk_cov, uint32_t* cam_status,
                 uint32_t* lmk_status),
                (hip_stream, n_cams, n_lmks, cam_eta, cam_lambda, lmk_eta, lmk_lambda, cam_mean, cam_cov, lmk_mean, lmk_cov, cam_status,
                 lmk_status)) {
  const char* fn = "gbp_post_moments";
  if (n_cams && !cam_eta) return null_arg(fn, "cam_eta");
  if (n_cams && !cam_lambda) return null_arg(fn, "cam_lambda");
  if (n_lmks && !lmk_eta) return null_arg(fn, "lmk_eta");
  if (n_lmks && !lmk_lambda) return null_arg(fn, "lmk_lambda");
  const uint64_t n = (uint64_t)n_cams + n_lmks;
  if (n > kMaxLanes) return bad_arg(fn, "n_cams + n_lmks is too large");
  last_error().clear();
  if (n == 0) return GBP_OK;
  hipLaunchKernelGGL(k_post_moments, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(hip_stream), n_cams, n_lmks,
                     cam_eta, cam_lambda, lmk_eta, lmk_lambda, cam_mean, cam_cov, lmk_mean, lmk_cov, cam_status, lmk_status);
  return launched(fn);
}

GBP_STATELESS_EXPORT(gbp_post_residuals,
                (void* hip_stream, uint32_t n_cams, uint32_t n_lmks, uint32_t n_edges, const uint32_t* cam_id, const uint32_t* lmk_id,
                 const float K[9], const float* cam_mean, const float* lmk_mean, const float* measurements, const uint32_t* active_flag,
                 const float* cam_cov, const float* lmk_cov, float* residual, float* reproj_cov),
                (hip_stream, n_cams, n_lmks, n_edges, cam_id, lmk_id, K, cam_mean, lmk_mean, measurements, active_flag, cam_cov, lmk_cov,
                 residual, reproj_cov)) {
  const char* fn = "gbp_post_residuals";
  if (!K) return null_arg(fn, "K");
  if (reproj_cov && !cam_cov) return bad_arg(fn, "reproj_cov needs cam_cov, which is NULL");
  if (reproj_cov && !lmk_cov) return bad_arg(fn, "reproj_cov needs lmk_cov, which is NULL");
  if (n_edges) {
    if (!cam_id) return null_arg(fn, "cam_id");
    if (!lmk_id) return null_arg(fn, "lmk_id");
    if (!cam_mean) return null_arg(fn, "cam_mean");
    if (!lmk_mean) return null_arg(fn, "lmk_mean");
    if (!measurements) return null_arg(fn, "measurements");
    if (!residual) return null_arg(fn, "residual");
    if (n_cams == 0) return bad_arg(fn, "n_cams is 0 with n_edges > 0");
    if (n_lmks == 0) return bad_arg(fn, "n_lmks is 0 with n_edges > 0");
  }
  if ((uint64_t)n_edges > kMaxLanes) return bad_arg(fn, "n_edges is too large");
  last_error().clear();
  if (n_edges == 0) return GBP_OK;
  K9 k;
  for (int i = 0; i < 9; ++i) k.k[i] = K[i];
  const dim3 grid((n_edges + 255) / 256), block(256);
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const int cov16 = (reinterpret_cast<uintptr_t>(cam_cov) & 15u) == 0 ? 1 : 0;
  if (reproj_cov)
    hipLaunchKernelGGL(k_post_residuals<true>, grid, block, 0, s, n_cams, n_lmks, n_edges, cam_id, lmk_id, k, cam_mean, lmk_mean, measurements,
                       active_flag, cam_cov, lmk_cov, cov16, residual, reproj_cov);
  else
    hipLaunchKernelGGL(k_post_residuals<false>, grid, block, 0, s, n_cams, n_lmks, n_edges, cam_id, lmk_id, k, cam_mean, lmk_mean, measurements,
                       active_flag, cam_cov, lmk_cov, cov16, residual, reproj_cov);
  return launched(fn);
}
