// stateless/stateless_wave.hpp — the mapping of a kernel that gives every item (a camera, say) one wavefront: kWavesPerBlock items per
// workgroup of 64 * kWavesPerBlock lanes, wave_grid(n) workgroups for n items.  Include it in a HIP translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gbp {
namespace stateless {

constexpr int kWavesPerBlock = 4;      // items per workgroup

// lane 0's value in every lane, as a scalar
__device__ __forceinline__ float lane0(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
// the item of the calling wave (the whole wave's: a scalar); items >= n have to return
__device__ __forceinline__ uint32_t wave_item() {
  return blockIdx.x * kWavesPerBlock + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}
inline dim3 wave_grid(uint32_t n) { return dim3(n / kWavesPerBlock + (n % kWavesPerBlock != 0u)); }

}  // namespace stateless
}  // namespace gbp
