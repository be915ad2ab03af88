// kernels/gbp_state_io.hip — the kernels that move state between the caller's arrays and the device records (upload, read,
// keyframe update, snapshot / restore) and their launchers.
#pragma once
#include "gbp_tile.hpp"

namespace gbp {
using namespace gbpdev;

// Snapshot / restore of the arrays a k_persist launch mutates (one launch for all of them): taken before every launch so that
// a launch whose barrier timed out can be undone and replayed on the two-kernel path.  `guard` != NULL: do nothing once the
// abort word is set — the snapshot then still holds the state the FIRST failed launch started from.
__global__ __launch_bounds__(256) void k_copy_segments(const CopySegs t, const unsigned* guard) {
  if (guard && __hip_atomic_load(guard, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;
  for (int sgi = 0; sgi < t.n; ++sgi) {
    const float4* src = static_cast<const float4*>(t.src[sgi]);
    float4* dst = static_cast<float4*>(t.dst[sgi]);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < t.n4[sgi]; i += (size_t)gridDim.x * 256) dst[i] = src[i];
  }
}

// Per-factor scalar state lives in compact per-position planes (FST_PACKED, FST_DAMP: gbp_kernels.h), so READ_PROG's damping /
// damping_count / robust_flag streams (ba.cpp:912-914) are plain copies of them and NEW_KEYFRAME's damping_count / active_flag
// streams (slam.cpp:920,926) move 8 bytes per factor over PCIe.
// ctl bit 0: damping_count := new_count;  bit 1: active flag := bit 2
__global__ __launch_bounds__(256) void k_state_set(int* __restrict__ fst_packed, const int* __restrict__ new_count,
                                                   const uint32_t* __restrict__ ctl, uint32_t n) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint32_t c = ctl[p];
  if (!(c & 3u)) return;
  const int packed = fst_packed[p];
  int count = packed >> 3;
  uint32_t flags = (uint32_t)packed & 7u;
  if (flags & kFlagPad) return;
  if (c & 1u) count = new_count[p];
  if (c & 2u) flags = (c & 4u) ? (flags | kFlagActive) : (flags & ~kFlagActive);
  fst_packed[p] = (int)(((uint32_t)count << 3) | flags);
}

// gbp_upload: 20 bytes per position cross PCIe (read here straight out of the pinned staging buffer when they fit it) instead of the 288 bytes
// of the arrays they go into
__global__ __launch_bounds__(256) void k_upload_scatter(float4* __restrict__ lmsg, const FactorState fs, float4* __restrict__ fac, const float4* __restrict__ st,
                                                        const float* __restrict__ var, uint32_t n) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const float4 s = st[p];
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  GBP_UNROLL
  for (int q = 0; q < kLmsgG; ++q) lmsg[(size_t)p * kLmsgG + q] = z;
  fs.damp[p] = s.x; fs.packed[p] = __float_as_int(s.y); fs.var[p] = var[p];
  fac[((size_t)(p >> 6) * kFacG + 13) * 64 + (p & 63)] = make_float4(0.f, 0.f, s.z, s.w);      // floats 52..55: z = .z, .w
}

// ---- device-resident caller arrays (gbp_api_devio.cpp): gbp_upload / gbp_read / gbp_read_priors / gbp_new_keyframe whose structs hold
// DEVICE pointers.  The twins of what the host path stages and k_upload_scatter / k_state_set spread: same targets, same
// bits, nothing crosses PCIe.  One thread per device POSITION p (pos_edge[p] = file index of its factor, ~0u = pad): the device-order
// side, which carries 80 (upload) / 8 (read, keyframe) bytes per position in whole 16-byte words, is lane-contiguous; the caller's
// file-order arrays (4 - 36 bytes per factor) are gathered / scattered through pos_edge, which runs in file order within a camera, so
// a wave's 4-byte accesses still fall into a few neighbouring lines.  Every position and every factor is written by exactly one lane.
__global__ __launch_bounds__(256) void k_upload_dev(const UploadDev a) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t e = a.pos_edge[p];
  float damping = 0.f, z0 = 0.f, z1 = 0.f, v = 0.f;
  int packed = (int)kFlagPad;
  float m[12];
  GBP_UNROLL
  for (int i = 0; i < 12; ++i) m[i] = 0.f;
  if (e != ~0u) {
    const bool on = a.active_flag[e] == 1u;
    const int count = a.damping_count ? a.damping_count[e] : 0;
    damping = a.damping ? a.damping[e] : 0.f;
    packed = (int)(((uint32_t)count << 3) | (on ? kFlagActive : 0u));
    z0 = a.measurements[2 * (size_t)e];
    z1 = a.measurements[2 * (size_t)e + 1];
    v = a.meas_variances[e];
    if (a.mu && a.om) {
      GBP_UNROLL
      for (int i = 0; i < 9; ++i) m[i] = a.om[(size_t)e * 9 + i];
    }
  }
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  GBP_UNROLL
  for (int q = 0; q < kLmsgG; ++q) a.lmsg[(size_t)p * kLmsgG + q] = z;
  a.fs.damp[p] = damping; a.fs.packed[p] = packed; a.fs.var[p] = v;
  a.fac[((size_t)(p >> 6) * kFacG + 13) * 64 + (p & 63)] = make_float4(0.f, 0.f, z0, z1);
  if (a.mu) {
    GBP_UNROLL
    for (int g = 0; g < kMuG; ++g) a.mu[((size_t)(p >> 6) * kMuG + g) * 64 + (p & 63)] = make_float4(m[4 * g], m[4 * g + 1], m[4 * g + 2], m[4 * g + 3]);
  }
}
// READ_PROG's damping / damping_count / robust_flag streams into the caller's file-order arrays (NULL = skipped)
__global__ __launch_bounds__(256) void k_read_state_dev(const uint32_t* __restrict__ pos_edge, const FactorState fs, float* damping,
                                                        int* damping_count, uint32_t* robust_flag, uint32_t n) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint32_t e = pos_edge[p];
  if (e == ~0u) return;
  const int packed = fs.packed[p];
  if (damping) damping[e] = fs.damp[p];
  if (damping_count) damping_count[e] = packed >> 3;
  if (robust_flag) robust_flag[e] = ((uint32_t)packed & kFlagRobust) ? 1u : 0u;
}
// NEW_KEYFRAME's damping_count / active_flag streams out of the caller's file-order arrays (NULL = unchanged): what k_state_set does
__global__ __launch_bounds__(256) void k_keyframe_state_dev(const uint32_t* __restrict__ pos_edge, int* __restrict__ fst_packed,
                                                            const int* __restrict__ new_count, const uint32_t* __restrict__ active_flag, uint32_t n) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint32_t e = pos_edge[p];
  if (e == ~0u) return;
  const int packed = fst_packed[p];
  int count = packed >> 3;
  uint32_t flags = (uint32_t)packed & 7u;
  if (flags & kFlagPad) return;
  if (new_count) count = new_count[e];
  if (active_flag) flags = active_flag[e] == 1u ? (flags | kFlagActive) : (flags & ~kFlagActive);
  fst_packed[p] = (int)(((uint32_t)count << 3) | flags);
}
// Variable records <-> the caller's row-major arrays: word i of the caller's array (record i / w, word i % w) sits at word
// (i / w) * stride + off + i % w of the padded device records (the element copies pack_cam / pack_lmk and the read paths make on the
// host).  Up to kMaxRecSegs arrays per launch (blockIdx.y).  A lane owns four consecutive words of the CALLER's array — lane-contiguous,
// one 16-byte access where the array's base is 16-byte aligned, four 4-byte ones for a view that is not — and places each word on its own.
template <bool TO_REC>
__global__ __launch_bounds__(256) void k_rec_copy(const RecSegs t) {
  const uint32_t sg = blockIdx.y;
  const uint32_t total = t.total[sg], w = t.w[sg], stride = t.stride[sg], off = t.off[sg];
  uint32_t* caller = static_cast<uint32_t*>(t.caller[sg]);
  uint32_t* rec = static_cast<uint32_t*>(t.rec[sg]);
  const uint64_t i0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= total) return;
  const bool vec = ((uintptr_t)caller & 15u) == 0 && i0 + 4 <= total;
  uint32_t v[4] = {0u, 0u, 0u, 0u};
  size_t at[4];
  GBP_UNROLL
  for (int k = 0; k < 4; ++k) {
    const uint32_t i = (uint32_t)i0 + k, r = i / w;
    at[k] = (size_t)r * stride + off + (i - r * w);
  }
  if (TO_REC) {
    if (vec) { const uint4 q = *reinterpret_cast<const uint4*>(caller + i0); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else {
      GBP_UNROLL
      for (int k = 0; k < 4; ++k) if (i0 + k < total) v[k] = caller[i0 + k];
    }
    GBP_UNROLL
    for (int k = 0; k < 4; ++k) if (i0 + k < total) rec[at[k]] = v[k];
  } else {
    GBP_UNROLL
    for (int k = 0; k < 4; ++k) if (i0 + k < total) v[k] = rec[at[k]];
    if (vec) *reinterpret_cast<uint4*>(caller + i0) = make_uint4(v[0], v[1], v[2], v[3]);
    else {
      GBP_UNROLL
      for (int k = 0; k < 4; ++k) if (i0 + k < total) caller[i0 + k] = v[k];
    }
  }
}

void launch_copy_segments(const CopySegs& t, const unsigned* guard, hipStream_t s) {
  size_t most = 0;
  for (int i = 0; i < t.n; ++i) most = t.n4[i] > most ? t.n4[i] : most;
  const uint32_t blocks = (uint32_t)(most / 256 > 1024 ? 1024 : (most + 255) / 256);
  hipLaunchKernelGGL(k_copy_segments, dim3(blocks ? blocks : 1), dim3(256), 0, s, t, guard);
}
void launch_upload_scatter(float4* lmsg, const FactorState& fs, float4* fac, const float4* st, const float* var, uint32_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_upload_scatter, dim3(blocks_for(n)), dim3(256), 0, s, lmsg, fs, fac, st, var, n);
}
void launch_state_set(int* fst_packed, const int* new_count, const uint32_t* ctl, uint32_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_state_set, dim3(blocks_for(n)), dim3(256), 0, s, fst_packed, new_count, ctl, n);
}
void launch_upload_dev(const UploadDev& a, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_upload_dev, dim3(blocks_for(a.n)), dim3(256), 0, s, a);
}
void launch_read_state_dev(const uint32_t* pos_edge, const FactorState& fs, float* damping, int* damping_count, uint32_t* robust_flag, uint32_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_read_state_dev, dim3(blocks_for(n)), dim3(256), 0, s, pos_edge, fs, damping, damping_count, robust_flag, n);
}
void launch_keyframe_state_dev(const uint32_t* pos_edge, int* fst_packed, const int* new_count, const uint32_t* active_flag, uint32_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_keyframe_state_dev, dim3(blocks_for(n)), dim3(256), 0, s, pos_edge, fst_packed, new_count, active_flag, n);
}
void launch_rec_copy(const RecSegs& t, bool to_rec, hipStream_t s) {
  uint32_t most = 0;
  for (int i = 0; i < t.n; ++i) most = t.total[i] > most ? t.total[i] : most;
  if (t.n == 0 || most == 0) return;
  const dim3 grid(blocks_for(((uint64_t)most + 3) / 4), (uint32_t)t.n);
  if (to_rec) hipLaunchKernelGGL(k_rec_copy<true>, grid, dim3(256), 0, s, t);
  else hipLaunchKernelGGL(k_rec_copy<false>, grid, dim3(256), 0, s, t);
}

}  // namespace gbp
