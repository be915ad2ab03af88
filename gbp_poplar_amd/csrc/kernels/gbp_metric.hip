// kernels/gbp_metric.hip — the metric kernels (means, residual sums, the riding metric's last step, the device-side folds) and
// their launchers.
#pragma once
#include "gbp_tile.hpp"
#include "gbp_metric_math.hpp"

namespace gbp {
using namespace gbpdev;

__global__ __launch_bounds__(256) void k_means(const float* __restrict__ camb, const float* __restrict__ lmkb,
                                               float* __restrict__ cam_mu, float* __restrict__ lmk_mu, uint32_t n_cams,
                                               uint32_t n_lmks, unsigned long long* health, unsigned long long* health_next,
                                               int count_cams) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t == 0) { health_next[0] = 0ull; health_next[1] = 0ull; }   // the NEXT evaluation's counters (double-buffered: no memset launch)
  if (t < n_cams) {
    float x[6];
    solve_pivot<6>(camb + (size_t)t * kCamRec + 8, 6, camb + (size_t)t * kCamRec, x);
    bool finite = true;
    GBP_UNROLL
    for (int i = 0; i < 6; ++i) { cam_mu[(size_t)t * 6 + i] = x[i]; finite &= (x[i] - x[i] == 0.f); }
    if (count_cams) {
      if (!finite) atomicAdd(&health[0], 1ull);
      if (!ldl_pivots_positive<6>(camb + (size_t)t * kCamRec + 8, 6)) atomicAdd(&health[1], 1ull);
    }
  } else if (t - n_cams < n_lmks) {
    const uint32_t l = t - n_cams;
    float x[3];
    solve_pivot<3>(lmkb + (size_t)l * 16 + 4, 3, lmkb + (size_t)l * 16, x);
    bool finite = true;
    GBP_UNROLL
    for (int i = 0; i < 3; ++i) { lmk_mu[(size_t)l * 3 + i] = x[i]; finite &= (x[i] - x[i] == 0.f); }
    if (!finite) atomicAdd(&health[0], 1ull);
    if (!ldl_pivots_positive<3>(lmkb + (size_t)l * 16 + 4, 3)) atomicAdd(&health[1], 1ull);
  }
}

constexpr uint32_t kEvalBlocks = 1024;
uint32_t eval_blocks(uint32_t n_tiles) {
  const uint32_t want = (n_tiles + 3) / 4;
  return want < kEvalBlocks ? (want ? want : 1) : kEvalBlocks;
}

__global__ __launch_bounds__(256) void k_eval(const uint32_t* __restrict__ row_cam, const uint32_t* __restrict__ lmk_idx,
                                              const int* __restrict__ fst_packed, const float4* __restrict__ fac, const float* __restrict__ cam_mu,
                                              const float* __restrict__ lmk_mu, const float* __restrict__ Kd,
                                              int num_undamped, DeviceEval* partials, unsigned long long* health,
                                              unsigned long long* health_out, uint32_t n_tiles) {
  // k_means has finished (stream order).  The words go back to zero: every user of the health areas finds them zero and leaves them so — the
  // launches of k_persist_flow that carry a metric per iteration count into BOTH areas (words 2k, 2k + 1 for iteration k) without a reset.
  if (blockIdx.x == 0 && threadIdx.x == 0) { health_out[0] = health[0]; health_out[1] = health[1]; health[0] = 0ull; health[1] = 0ull; }
  // block j produces S_j (see "THE ORDER OF THE METRIC'S SUMS"): one 256-factor block of the sweep at a time, wave w = tile 4b + w
  __shared__ double sh_d[2][4];
  __shared__ unsigned sh_u[3][4];
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  DeviceEval o;
  o.sum_norm = 0; o.sum_half_sq = 0; o.n_active = 0; o.n_relin = 0; o.n_robust = 0; o.pad = 0;
  for (uint32_t b = blockIdx.x; b < n_tiles / 4; b += gridDim.x) {
    const uint32_t tile = b * 4 + w, p = tile * 64 + lane;
    const int packed = fst_packed[p];
    const uint32_t flags = (uint32_t)packed & 7u;
    const bool pad = (flags & kFlagPad) != 0, active = !pad && (flags & kFlagActive) != 0;
    double s_norm = 0, s_half = 0;
    if (active) {
      const uint32_t cam_i = row_cam[p >> 4], lmk_i = lmk_idx[p];
      const float4 zg = fac[((size_t)tile * kFacG + 13) * 64 + lane];  // floats 52..55: z = .z, .w
      float cm[6], lmu[3];
      for (int i = 0; i < 6; ++i) cm[i] = cam_mu[(size_t)cam_i * 6 + i];
      for (int i = 0; i < 3; ++i) lmu[i] = lmk_mu[(size_t)lmk_i * 3 + i];
      eval_factor(cm, lmu, zg.z, zg.w, Kd, s_norm, s_half);
    }
    eval_wave_tree(s_norm, s_half);
    const unsigned n_act = (unsigned)__popcll(__builtin_amdgcn_ballot_w64(active));
    const unsigned n_rel = (unsigned)__popcll(__builtin_amdgcn_ballot_w64(!pad && (packed >> 3) == -num_undamped));
    const unsigned n_rob = (unsigned)__popcll(__builtin_amdgcn_ballot_w64(!pad && (flags & kFlagRobust) != 0));
    if (lane == 0) { sh_d[0][w] = s_norm; sh_d[1][w] = s_half; sh_u[0][w] = n_act; sh_u[1][w] = n_rel; sh_u[2][w] = n_rob; }
    __syncthreads();
    if (threadIdx.x == 0) {
      o.sum_norm += ((sh_d[0][0] + sh_d[0][1]) + sh_d[0][2]) + sh_d[0][3];
      o.sum_half_sq += ((sh_d[1][0] + sh_d[1][1]) + sh_d[1][2]) + sh_d[1][3];
      o.n_active += sh_u[0][0] + sh_u[0][1] + sh_u[0][2] + sh_u[0][3];
      o.n_relin += sh_u[1][0] + sh_u[1][1] + sh_u[1][2] + sh_u[1][3];
      o.n_robust += sh_u[2][0] + sh_u[2][1] + sh_u[2][2] + sh_u[2][3];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = o;
}

// The riding metric of a piece's LAST iteration, which no sweep follows: the same per-tile records from the same metric records
// (one wave per tile, ride_metric), into slot counter - 1.
__global__ __launch_bounds__(256) void k_eval_ride(const EvalRide ev, const uint32_t* __restrict__ row_cam, const uint32_t* __restrict__ lmk_idx,
                                                   const int* __restrict__ fst_packed, const float4* __restrict__ fac, const float* __restrict__ Kd) {
  const uint32_t ws = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, p = ws * 64 + lane;
  const uint32_t cam_i = row_cam[p >> 4], lmk_i = lmk_idx[p];
  const int packed = fst_packed[p];
  const float4 zg = fac[((size_t)ws * kFacG + 13) * 64 + lane];  // floats 52..55: z = .z, .w
  const float4 q0 = ev.cam_rec[(size_t)cam_i * 3], q1 = ev.cam_rec[(size_t)cam_i * 3 + 1], q2 = ev.cam_rec[(size_t)cam_i * 3 + 2];
  const float4 lq = ev.lmk_mean[lmk_i];
  ride_metric(ev, (uint32_t)__builtin_amdgcn_readfirstlane((int)*ev.counter), ws, ws, lane, packed, zg.z, zg.w, q0, q1, q2, lq, Kd);
}

// The per-tile records k_sweep<EV> left in ring slot blockIdx.x reduced to ONE result, in the order of every other metric (see
// "THE ORDER OF THE METRIC'S SUMS"): thread j forms the block sum S_j k_eval would have produced, thread 0 then adds S_0, S_1, ...
// serially — what the host does with k_eval's block sums, done here so that 56 bytes per iteration cross PCIe instead of 49 KB.
struct EvalSum {       // == gbp_eval_out (include/gbp_mi355x.h)
  double sum_norm, sum_half_sq;
  unsigned long long n_active, n_relin, n_robust, n_nonfinite, n_nonpd;
};
// The last step of every device-side fold: the n_sums <= 1 024 block sums one workgroup staged in LDS (entries >= n_sums hold zeros)
// added serially from 0 by ONE lane, as the host adds k_eval's block sums (sum_eval in gbp_api_eval.cpp); o's health words are the caller's.
GBP_DEV void eval_fold_chain(const double (&sh_d)[2][1024], const unsigned (&sh_u)[3][1024], uint32_t n_sums, EvalSum& o) {
  o.sum_norm = 0; o.sum_half_sq = 0; o.n_active = 0; o.n_relin = 0; o.n_robust = 0;
  for (uint32_t k0 = 0; k0 < n_sums; k0 += 16) {      // sixteen LDS reads in flight, added in order
    double a[16], h[16];
    GBP_UNROLL
    for (int u = 0; u < 16; ++u) { a[u] = sh_d[0][k0 + u]; h[u] = sh_d[1][k0 + u]; }
    GBP_UNROLL
    for (int u = 0; u < 16; ++u)
      if (k0 + (uint32_t)u < n_sums) { o.sum_norm += a[u]; o.sum_half_sq += h[u]; }
    GBP_UNROLL
    for (int u = 0; u < 16; ++u) { o.n_active += sh_u[0][k0 + u]; o.n_relin += sh_u[1][k0 + u]; o.n_robust += sh_u[2][k0 + u]; }
  }
}
__global__ __launch_bounds__(1024) void k_eval_fold(const EvalRide ev, EvalSum* out, uint32_t n_sums) {
  __shared__ double sh_d[2][1024];
  __shared__ unsigned sh_u[3][1024];
  const uint32_t j = threadIdx.x, slot = blockIdx.x, nb = ev.n_tiles / 4;
  const EvalRec* part = ev.part + (size_t)slot * ev.n_tiles;
  double s_norm = 0, s_half = 0;
  unsigned n_act = 0, n_rel = 0, n_rob = 0;
  if (j < n_sums) {
    for (uint32_t b0 = j; b0 < nb; b0 += 4 * n_sums) {      // four blocks' records in flight at once (clamped, unconditional), added in order
      EvalRec w[4][4];
      GBP_UNROLL
      for (int u = 0; u < 4; ++u) {
        const uint32_t b = b0 + (uint32_t)u * n_sums < nb ? b0 + (uint32_t)u * n_sums : b0;
        GBP_UNROLL
        for (int k = 0; k < 4; ++k) w[u][k] = part[4 * (size_t)b + k];
      }
      GBP_UNROLL
      for (int u = 0; u < 4; ++u) {
        if (b0 + (uint32_t)u * n_sums >= nb) break;
        s_norm += ((w[u][0].sum_norm + w[u][1].sum_norm) + w[u][2].sum_norm) + w[u][3].sum_norm;
        s_half += ((w[u][0].sum_half_sq + w[u][1].sum_half_sq) + w[u][2].sum_half_sq) + w[u][3].sum_half_sq;
        n_act += w[u][0].n_active + w[u][1].n_active + w[u][2].n_active + w[u][3].n_active;
        n_rel += w[u][0].n_relin + w[u][1].n_relin + w[u][2].n_relin + w[u][3].n_relin;
        n_rob += w[u][0].n_robust + w[u][1].n_robust + w[u][2].n_robust + w[u][3].n_robust;
      }
    }
  }
  sh_d[0][j] = s_norm; sh_d[1][j] = s_half; sh_u[0][j] = n_act; sh_u[1][j] = n_rel; sh_u[2][j] = n_rob;
  __syncthreads();
  if (j == 0) {
    EvalSum o;
    eval_fold_chain(sh_d, sh_u, n_sums, o);
    o.n_nonfinite = ev.slot_health[2 * (size_t)slot]; o.n_nonpd = ev.slot_health[2 * (size_t)slot + 1];
    out[slot] = o;
  }
}

// sum_eval of gbp_api_eval.cpp on the device, for a caller whose gbp_eval_out records live on the GPU: the DeviceEval records of ONE
// metric (part[0] = its two health words, then its partial sums) reduced to one result, workgroup r taking metric r (part + r *
// stride -> out[r]).  per_wave = 0: part[1 .. nb] are the block sums S_j of k_eval; per_wave = 1: part[1 + t] is the record of tile
// wave t of the persistent kernel and thread b forms B_b = ((w_4b + w_4b+1) + w_4b+2) + w_4b+3 (nb = n_tiles / 4 <= 1 024: no block
// stride on a graph that runs there).  Thread 0 then adds them serially from 0: the additions of "THE ORDER OF THE METRIC'S SUMS".
__global__ __launch_bounds__(1024) void k_eval_fold_part(const DeviceEval* __restrict__ parts, uint32_t stride, uint32_t nb, uint32_t n_tiles,
                                                         int per_wave, EvalSum* out) {
  __shared__ double sh_d[2][1024];
  __shared__ unsigned sh_u[3][1024];
  const uint32_t j = threadIdx.x;
  const DeviceEval* part = parts + (size_t)blockIdx.x * stride;
  double s_norm = 0, s_half = 0;
  unsigned n_act = 0, n_rel = 0, n_rob = 0;      // (one record counts at most the positions of its tiles: 32 bits hold them, the totals are 64-bit)
  if (j < nb) {
    if (per_wave) {
      DeviceEval w[4];
      GBP_UNROLL
      for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t t = 4 * j + k;
        w[k] = part[1 + (t < n_tiles ? t : 4 * j)];      // (clamped, unconditional: four loads in flight)
        if (t >= n_tiles) { w[k].sum_norm = 0; w[k].sum_half_sq = 0; w[k].n_active = 0; w[k].n_relin = 0; w[k].n_robust = 0; }
      }
      s_norm = ((w[0].sum_norm + w[1].sum_norm) + w[2].sum_norm) + w[3].sum_norm;
      s_half = ((w[0].sum_half_sq + w[1].sum_half_sq) + w[2].sum_half_sq) + w[3].sum_half_sq;
      n_act = (unsigned)(w[0].n_active + w[1].n_active + w[2].n_active + w[3].n_active);
      n_rel = (unsigned)(w[0].n_relin + w[1].n_relin + w[2].n_relin + w[3].n_relin);
      n_rob = (unsigned)(w[0].n_robust + w[1].n_robust + w[2].n_robust + w[3].n_robust);
    } else {
      const DeviceEval w = part[1 + j];
      s_norm = w.sum_norm; s_half = w.sum_half_sq;
      n_act = (unsigned)w.n_active; n_rel = (unsigned)w.n_relin; n_rob = (unsigned)w.n_robust;
    }
  }
  sh_d[0][j] = s_norm; sh_d[1][j] = s_half; sh_u[0][j] = n_act; sh_u[1][j] = n_rel; sh_u[2][j] = n_rob;
  __syncthreads();
  if (j == 0) {
    EvalSum o;
    eval_fold_chain(sh_d, sh_u, nb, o);
    const unsigned long long* h = reinterpret_cast<const unsigned long long*>(part);
    o.n_nonfinite = h[0]; o.n_nonpd = h[1];
    out[blockIdx.x] = o;
  }
}

void launch_eval_ride(const EvalRide& ev, const uint32_t* row_cam, const uint32_t* lmk_idx, const int* fst_packed, const float4* fac, const float* K9_dev, hipStream_t s) {
  hipLaunchKernelGGL(k_eval_ride, dim3(ev.n_tiles / 4), dim3(256), 0, s, ev, row_cam, lmk_idx, fst_packed, fac, K9_dev);
}
void launch_eval_fold(const EvalRide& ev, uint32_t n_slots, void* out, hipStream_t s) {
  if (n_slots == 0) return;
  hipLaunchKernelGGL(k_eval_fold, dim3(n_slots), dim3(1024), 0, s, ev, static_cast<EvalSum*>(out), eval_blocks(ev.n_tiles));
}
void launch_eval_fold_part(const DeviceEval* parts, uint32_t stride, uint32_t nb, uint32_t n_tiles, bool per_wave, uint32_t n_records, void* out, hipStream_t s) {
  if (n_records == 0) return;
  hipLaunchKernelGGL(k_eval_fold_part, dim3(n_records), dim3(1024), 0, s, parts, stride, nb, n_tiles, per_wave ? 1 : 0, static_cast<EvalSum*>(out));
}
void launch_means(const float4* camb, const float4* lmkb, float* cam_mu, float* lmk_mu, uint32_t n_cams, uint32_t n_lmks,
                  unsigned long long* health2, unsigned long long* health2_next, bool count_cams, hipStream_t s) {
  hipLaunchKernelGGL(k_means, dim3(blocks_for((uint64_t)n_cams + n_lmks)), dim3(256), 0, s, (const float*)camb,
                     (const float*)lmkb, cam_mu, lmk_mu, n_cams, n_lmks, health2, health2_next, count_cams ? 1 : 0);
}
void launch_eval(const uint32_t* row_cam, const uint32_t* lmk_idx, const int* fst_packed, const float4* fac, const float* cam_mu,
                 const float* lmk_mu, const float* K9_dev, int num_undamped_iters, DeviceEval* partials,
                 unsigned long long* health2, unsigned long long* health2_out, uint32_t n_tiles, hipStream_t s) {
  hipLaunchKernelGGL(k_eval, dim3(eval_blocks(n_tiles)), dim3(256), 0, s, row_cam, lmk_idx, fst_packed, fac, cam_mu, lmk_mu, K9_dev,
                     num_undamped_iters, partials, health2, health2_out, n_tiles);
}

}  // namespace gbp
