// resect/resect_call.hpp — the HOST side that a camera-major call (gbp_resect_cameras, gbp_locate_cameras) shares: the checks of the
// arguments both take, in two steps so that a library's own checks keep their place between them, and the Graph of the C arguments.
#pragma once
#include "../stateless/stateless_export.hpp"
#include "resect_math.hpp"

namespace gbp {
namespace resect {

// with n_cams > 0
inline int check_cameras(const char* fn, const float* K, const uint32_t* cam_start, const float* cam_mean, const uint32_t* status) {
  if (!K) return stateless::null_arg(fn, "K");
  if (!cam_start) return stateless::null_arg(fn, "cam_start");
  if (!cam_mean) return stateless::null_arg(fn, "cam_mean");
  if (!status) return stateless::null_arg(fn, "status");
  return GBP_OK;
}
// with n_cams > 0 and n_edges > 0
inline int check_edges(const char* fn, uint32_t n_lmks, const uint32_t* lmk_id, const float* lmk_mean, const float* measurements) {
  if (!lmk_id) return stateless::null_arg(fn, "lmk_id");
  if (!lmk_mean) return stateless::null_arg(fn, "lmk_mean");
  if (!measurements) return stateless::null_arg(fn, "measurements");
  if (n_lmks == 0) return stateless::bad_arg(fn, "n_lmks is 0 with n_edges > 0");
  return GBP_OK;
}
inline Graph graph_of(uint32_t n_lmks, uint32_t n_edges, const uint32_t* lmk_id, const uint32_t* cam_edges, const float* lmk_mean,
                      const float* measurements, const uint32_t* active_flag, const uint32_t* lmk_use) {
  return Graph{n_lmks, n_edges, lmk_id, cam_edges, lmk_mean, measurements, active_flag, lmk_use};
}

}  // namespace resect
}  // namespace gbp
