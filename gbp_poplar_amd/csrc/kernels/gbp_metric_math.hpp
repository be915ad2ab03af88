// kernels/gbp_metric_math.hpp — the metric math: fp64 pivot solves of the beliefs, the reprojection residual of a factor, the
// order of the metric's sums and the records they leave.  Device helpers only; used by the metric kernels and by every kernel the
// metric rides in (k_sweep<EV>, k_beliefs*_ev, k_persist_flow<EV>).  The per-lane arithmetic in front of "THE ORDER OF THE METRIC'S
// SUMS" is also what the solution readout is made of (post/post_math.hpp), which compiles it for the host as well.
#pragma once
#include "../gbp_kernels.h"
#include "../gbp_device_math.hpp"

namespace gbp {
using namespace gbpdev;

// =================================================================================================
// Metric: util.cpp:74-144.  Variable means by an fp64 partial-pivot solve of the fp32 belief
// (stands in for Eigen's general inverse), residuals in fp32, sums in fp64.
// =================================================================================================
// Every loop has compile-time bounds and every row swap is a select, so the 6 x 7 fp64 tableau lives in registers
// (no scratch: this kernel sits on the critical path of the per-iteration metric of small graphs).
template <int N>
GBP_DEV void solve_pivot(const float* A, int lda, const float* b, float* x) {
  double M[N][N + 1];
  GBP_UNROLL
  for (int i = 0; i < N; ++i) {
    GBP_UNROLL
    for (int j = 0; j < N; ++j) M[i][j] = A[i * lda + j];
    M[i][N] = b[i];
  }
  GBP_UNROLL
  for (int k = 0; k < N; ++k) {
    int piv = k;
    double best = fabs(M[k][k]);
    GBP_UNROLL
    for (int i = k + 1; i < N; ++i)
      if (fabs(M[i][k]) > best) { best = fabs(M[i][k]); piv = i; }
    GBP_UNROLL
    for (int i = k + 1; i < N; ++i) {      // swap rows k and piv (at most one i matches)
      const bool sw = piv == i;
      GBP_UNROLL
      for (int j = 0; j <= N; ++j) {
        const double t = M[k][j];
        M[k][j] = sw ? M[i][j] : t;
        M[i][j] = sw ? t : M[i][j];
      }
    }
    GBP_UNROLL
    for (int i = k + 1; i < N; ++i) {
      const double f = M[i][k] / M[k][k];
      GBP_UNROLL
      for (int j = k; j <= N; ++j) M[i][j] -= f * M[k][j];
    }
  }
  GBP_UNROLL
  for (int i = N - 1; i >= 0; --i) {
    double s = M[i][N];
    GBP_UNROLL
    for (int j = i + 1; j < N; ++j) s -= M[i][j] * (double)x[j];
    x[i] = (float)(s / M[i][i]);
  }
}

// health check: a belief Lambda is usable by inv6x6 / inv3x3 only while the un-pivoted
// LDL^T pivots of its lower triangle (matlib.cpp:193-206) stay positive; a non-PD landmark belief is the
// early-warning sign of the blow-ups seen on fr1xyz.
template <int N>
GBP_DEV bool ldl_pivots_positive(const float* A, int lda) {
  double L[N][N], D[N];
  bool ok = true;
  GBP_UNROLL
  for (int j = 0; j < N; ++j) {
    double d = A[j * lda + j];
    GBP_UNROLL
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k] * D[k];
    D[j] = d;
    if (!(d > 0.0)) ok = false;
    GBP_UNROLL
    for (int i = j + 1; i < N; ++i) {
      double v = A[i * lda + j];
      GBP_UNROLL
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k] * D[k];
      L[i][j] = v / d;
    }
  }
  return ok;
}

// One factor's share of the metric (util.cpp:95-129): reprojection residual of the belief means, in two steps — the rotation
// of the camera's mean (eigenso3exp, util.cpp:20-32: a function of the camera alone), then the residual of one factor.  k_eval and
// the metric phase of k_persist evaluate both per factor (eval_factor), the metric that rides in the two-kernel path evaluates
// the first once per camera (k_beliefs<EV>) and the second per factor (k_sweep<EV>): the same operations on the same operands.
GBP_DEV void eval_cam_rot(const float (&cm)[6], float (&R)[9]) {
  // eigenso3exp, util.cpp:20-32 (single expression)
  const float th = sqrtf(cm[3] * cm[3] + cm[4] * cm[4] + cm[5] * cm[5]);
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.f : 0.f;
  if (!(th < 1e-6)) {
    const float W[9] = {0.f, -cm[5], cm[4], cm[5], 0.f, -cm[3], -cm[4], cm[3], 0.f};
    const float sa = sinf(th) / th, sb = (1 - cosf(th)) / (th * th);
    GBP_UNROLL
    for (int r = 0; r < 3; ++r) {
      GBP_UNROLL
      for (int c = 0; c < 3; ++c) {
        float ww = 0.f;
        GBP_UNROLL
        for (int k = 0; k < 3; ++k) ww += W[r * 3 + k] * W[k * 3 + c];
        R[r * 3 + c] = R[r * 3 + c] + (sa * W[r * 3 + c] + sb * ww);
      }
    }
  }
}
// the residual itself, z - pi(mean): what the metric sums (eval_residual) and what the solution readout hands out per observation
// (post/post_math.hpp)
template <class KF>     // Kd[i]: the pin-hole matrix from a device pointer (k_eval) or from the kernel arguments
GBP_DEV void eval_reproj_residual(const float (&R)[9], const float (&t)[3], const float (&lmu)[3], float z0, float z1, KF&& Kd, float& r0, float& r1) {
  float pcf[3], pr[2];
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) pcf[i] = (R[i * 3] * lmu[0] + R[i * 3 + 1] * lmu[1]) + R[i * 3 + 2] * lmu[2];
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) pcf[i] += t[i];
  GBP_UNROLL
  for (int i = 0; i < 2; ++i) pr[i] = ((Kd[i * 3] * pcf[0] + Kd[i * 3 + 1] * pcf[1]) + Kd[i * 3 + 2] * pcf[2]) / pcf[2];
  r0 = z0 - pr[0];
  r1 = z1 - pr[1];
}
template <class KF>
GBP_DEV void eval_residual(const float (&R)[9], const float (&t)[3], const float (&lmu)[3], float z0, float z1, KF&& Kd, double& s_norm, double& s_half) {
  float r0, r1;
  eval_reproj_residual(R, t, lmu, z0, z1, Kd, r0, r1);
  s_norm += (double)sqrtf(r0 * r0 + r1 * r1);
  s_half += (double)(float)(0.5 * (double)(r0 * r0 + r1 * r1));
}
GBP_DEV void eval_factor(const float (&cm)[6], const float (&lmu)[3], float z0, float z1, const float* Kd, double& s_norm, double& s_half) {
  float R[9];
  eval_cam_rot(cm, R);
  const float t[3] = {cm[0], cm[1], cm[2]};
  eval_residual(R, t, lmu, z0, z1, Kd, s_norm, s_half);
}
#if defined(__HIP__)      // below: wave-level code (what is above is per-lane arithmetic that post/post_math.hpp also compiles for the host)
// THE ORDER OF THE METRIC'S SUMS (every path produces exactly these fp64 additions):
//   w_t  = the 64 lane values of tile t (0 + the factor's term) reduced by the shuffle tree below;
//   B_b  = ((w_4b + w_4b+1) + w_4b+2) + w_4b+3      the 256 factor positions of sweep workgroup b;
//   S_j  = B_j + B_j+N + B_j+2N + ...  (serially, from 0)   N = eval_blocks(n_tiles) <= 1 024 block sums travel to the host;
//   sum  = S_0 + S_1 + ... (serially, on the host: sum_eval in gbp_api_eval.cpp).
// (lane 0 ends with the sum; what the other lanes end with is not used.  The tree is s += shfl_down(s, off) for off = 32, 16, 8,
// 4, 2, 1; from 8 on the lanes that still matter read inside their own DPP row: a row shift — two v_mov_b32_dpp per double — instead
// of two ds_bpermute round trips through the LDS crossbar per double and step.  Same operands, same additions.)
GBP_DEV double row_shl_f64(double v, const int ctrl_row_shl) {
  const long long b = __double_as_longlong(v);
  int lo = (int)(unsigned)b, hi = (int)(unsigned)((unsigned long long)b >> 32);
  switch (ctrl_row_shl) {      // (the DPP control is an immediate)
    case 8: lo = __builtin_amdgcn_update_dpp(lo, lo, 0x108, 0xF, 0xF, false); hi = __builtin_amdgcn_update_dpp(hi, hi, 0x108, 0xF, 0xF, false); break;
    case 4: lo = __builtin_amdgcn_update_dpp(lo, lo, 0x104, 0xF, 0xF, false); hi = __builtin_amdgcn_update_dpp(hi, hi, 0x104, 0xF, 0xF, false); break;
    case 2: lo = __builtin_amdgcn_update_dpp(lo, lo, 0x102, 0xF, 0xF, false); hi = __builtin_amdgcn_update_dpp(hi, hi, 0x102, 0xF, 0xF, false); break;
    default: lo = __builtin_amdgcn_update_dpp(lo, lo, 0x101, 0xF, 0xF, false); hi = __builtin_amdgcn_update_dpp(hi, hi, 0x101, 0xF, 0xF, false); break;
  }
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
GBP_DEV void eval_wave_tree(double& s_norm, double& s_half) {
  s_norm += __shfl_down(s_norm, 32); s_half += __shfl_down(s_half, 32);
  s_norm += __shfl_down(s_norm, 16); s_half += __shfl_down(s_half, 16);
  s_norm += row_shl_f64(s_norm, 8); s_half += row_shl_f64(s_half, 8);
  s_norm += row_shl_f64(s_norm, 4); s_half += row_shl_f64(s_half, 4);
  s_norm += row_shl_f64(s_norm, 2); s_half += row_shl_f64(s_half, 2);
  s_norm += row_shl_f64(s_norm, 1); s_half += row_shl_f64(s_half, 1);
}

// One tile's share of the riding metric (EvalRide in gbp_kernels.h): the residual of every factor from its state word, its
// measurement and the metric records of its camera (q0..q2) and landmark (lq); the wave's partial sums go to slot counter - 1 of
// the ring, at index TILE.  Every lane computes (no branch for the callers' loads to sink into); the launch is the same for every
// iteration of a burst, the first included: the slot comes from a counter in device memory, and while that is 0 there is nothing
// to store.  Wave slot 0 also collects what the belief update counted and zeroes the counters for the next one.
// `done` = *ev.counter, read by the caller BEFORE its first store: behind stores the load would be a vector load, and waiting for
// it would wait for every store the wave has in flight (vmcnt counts both, in order: +1.5 us at the end of every sweep wave).
template <class KF>
GBP_DEV void ride_metric(const EvalRide& ev, uint32_t done, uint32_t ws, uint32_t tile, uint32_t lane, int packed, float z0, float z1,
                         const float4 q0, const float4 q1, const float4 q2, const float4 lq, KF&& K) {
  const uint32_t flags = (uint32_t)packed & 7u;
  const bool pad = (flags & kFlagPad) != 0, counts = !pad && (flags & kFlagActive) != 0;
  const float R[9] = {q0.x, q0.y, q0.z, q1.x, q1.y, q1.z, q2.x, q2.y, q2.z}, t[3] = {q0.w, q1.w, q2.w}, lmu[3] = {lq.x, lq.y, lq.z};
  double r_norm = 0, r_half = 0;
  eval_residual(R, t, lmu, z0, z1, K, r_norm, r_half);
  double s_norm = counts ? r_norm : 0.0, s_half = counts ? r_half : 0.0;
  eval_wave_tree(s_norm, s_half);
  const uint32_t n_act = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(counts));
  const uint32_t n_rel = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(!pad && (packed >> 3) == -ev.num_undamped));
  const uint32_t n_rob = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(!pad && (flags & kFlagRobust) != 0));
  if (done != 0u && lane == 0) {
    const uint32_t slot = done - 1u;
    EvalRec r;
    r.sum_norm = s_norm; r.sum_half_sq = s_half; r.n_active = n_act; r.n_relin = n_rel; r.n_robust = n_rob; r.pad = 0;
    ev.part[(size_t)slot * ev.n_tiles + tile] = r;
    if (ws == 0u) {
      ev.slot_health[2 * (size_t)slot] = ev.health[0]; ev.slot_health[2 * (size_t)slot + 1] = ev.health[1];
      ev.health[0] = 0ull; ev.health[1] = 0ull;
    }
  }
}

// the metric record of a tile wave (DeviceEval slot 1 + wave): its residual sums (zero where the factor is not active) through the lane
// tree of eval_wave_tree, the counts of ITS factors' flags (packed: the state word as the evaluated sweep left it) through ballots
GBP_DEV void eval_wave_record(DeviceEval* slot, uint32_t lane, int packed, int num_undamped, double s_norm, double s_half) {
  const uint32_t flags = (uint32_t)packed & 7u;
  const bool pad = (flags & kFlagPad) != 0;
  eval_wave_tree(s_norm, s_half);
  const unsigned long long n_act = (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(!pad && (flags & kFlagActive) != 0));
  const unsigned long long n_rel = (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(!pad && (packed >> 3) == -num_undamped));
  const unsigned long long n_rob = (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(!pad && (flags & kFlagRobust) != 0));
  if (lane == 0) {
    DeviceEval o;
    o.sum_norm = s_norm; o.sum_half_sq = s_half; o.n_active = n_act; o.n_relin = n_rel; o.n_robust = n_rob; o.pad = 0;
    *slot = o;
  }
}
// the health words h[0..1] of a metric into its host slot (slot [0] of the metric), and h back to zero for the next one
GBP_DEV void health_handoff(DeviceEval* slots, unsigned long long* h) {
  unsigned long long* out = reinterpret_cast<unsigned long long*>(slots);
  out[0] = __hip_atomic_load(&h[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  out[1] = __hip_atomic_load(&h[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&h[0], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&h[1], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#endif  // __HIP__

}  // namespace gbp
