// Every host function csrc/gbp_kernels.h declares, in its order, for the CPU sanitizer build of the C-ABI (tests/test_host_sanitizers.py):
// the host side of the library — every csrc/*.cpp of the product — is compiled with g++ -fsanitize=address,undefined and linked against
// this file instead of gbp_kernels.hip.  The declarations are strong, so a launcher that is missing here, or whose parameters no longer
// match the header, is a link error of that test.  Nothing here computes: a launch without a device is a bug of the test, so every
// launcher aborts; only the pure host functions (grid sizing) return what the real ones return for an unlaunchable graph.
#include "../../gbp_poplar_amd/csrc/gbp_kernels.h"

#include <cstdio>
#include <cstdlib>

namespace gbp {

[[noreturn]] static void no_device(const char* what) {
  std::fprintf(stderr, "kernel_stubs: %s called in the CPU sanitizer build (no device code is linked)\n", what);
  std::abort();
}

PersistGrid persist_grid(uint32_t n_tiles, uint32_t, uint32_t, bool) { return PersistGrid{(n_tiles + 3) / 4, 0u, 0u}; }
void launch_sweep(const SweepArgs&, uint32_t, bool, hipStream_t, bool) { no_device("launch_sweep"); }
void launch_linearise(const SweepArgs&, uint32_t, hipStream_t) { no_device("launch_linearise"); }
void launch_cmsg_expand(const SweepArgs&, uint32_t, float*, hipStream_t) { no_device("launch_cmsg_expand"); }
void launch_beliefs(BeliefArgs, bool, bool, hipStream_t, bool) { no_device("launch_beliefs"); }
void launch_beliefs_cam_peers(BeliefArgs, const float* const*, hipStream_t, bool) { no_device("launch_beliefs_cam_peers"); }
void launch_gather_peers(const float* const*, float*, uint32_t, int, int, hipStream_t) { no_device("launch_gather_peers"); }
void launch_beliefs_cam_slice(BeliefArgs, const float* const*, const CamSlice&, hipStream_t) { no_device("launch_beliefs_cam_slice"); }
void launch_gather_slices(const float4* const*, const BeliefArgs&, int, hipStream_t) { no_device("launch_gather_slices"); }
void launch_eval_fold(const EvalRide&, uint32_t, void*, hipStream_t) { no_device("launch_eval_fold"); }
void launch_eval_fold_part(const DeviceEval*, uint32_t, uint32_t, uint32_t, bool, uint32_t, void*, hipStream_t) { no_device("launch_eval_fold_part"); }
void launch_eval_ride(const EvalRide&, const uint32_t*, const uint32_t*, const int*, const float4*, const float*, hipStream_t) { no_device("launch_eval_ride"); }
int persist_max_resident_blocks() { return 0; }
hipError_t launch_persist(PersistArgs, bool, hipStream_t) { no_device("launch_persist"); }
void launch_copy_segments(const CopySegs&, const unsigned*, hipStream_t) { no_device("launch_copy_segments"); }
bool persist_probe(uint32_t, uint32_t, uint32_t, unsigned*, unsigned*, volatile unsigned*, bool, hipStream_t) { return false; }
void launch_state_set(int*, const int*, const uint32_t*, uint32_t, hipStream_t) { no_device("launch_state_set"); }
void launch_upload_scatter(float4*, const FactorState&, float4*, const float4*, const float*, uint32_t, hipStream_t) { no_device("launch_upload_scatter"); }
void launch_upload_dev(const UploadDev&, hipStream_t) { no_device("launch_upload_dev"); }
void launch_read_state_dev(const uint32_t*, const FactorState&, float*, int*, uint32_t*, uint32_t, hipStream_t) { no_device("launch_read_state_dev"); }
void launch_keyframe_state_dev(const uint32_t*, int*, const int*, const uint32_t*, uint32_t, hipStream_t) { no_device("launch_keyframe_state_dev"); }
void launch_rec_copy(const RecSegs&, bool, hipStream_t) { no_device("launch_rec_copy"); }
void launch_means(const float4*, const float4*, float*, float*, uint32_t, uint32_t, unsigned long long*, unsigned long long*, bool, hipStream_t) { no_device("launch_means"); }
void launch_eval(const uint32_t*, const uint32_t*, const int*, const float4*, const float*, const float*, const float*, int, DeviceEval*,
                 unsigned long long*, unsigned long long*, uint32_t, hipStream_t) { no_device("launch_eval"); }
uint32_t eval_blocks(uint32_t n_tiles) { return (n_tiles + 3) / 4; }
bool lab_launch_sweep_ablated(const SweepArgs&, uint32_t, int, hipStream_t) { return false; }
bool launch_flow_torture(float4*, unsigned long long*, int, int, int, unsigned, unsigned, int, hipStream_t) { no_device("launch_flow_torture"); }
bool debug_math_widths(int, int*, int*) { return false; }
void launch_debug_math(int, const float*, float*, int, hipStream_t) { no_device("launch_debug_math"); }

}  // namespace gbp
