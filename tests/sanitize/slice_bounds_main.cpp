// The camera slices of the sliced peer-memory transport (slice_bounds, csrc/gbp_kernels.h) under ASan + UBSan, on their own: for every
// camera count and world size of the table the slices are monotone, contiguous, cover [0, C) exactly once and none is wider than the
// result buffer a rank allocates for its slice (ceil(C / world) records).  Built and run by tests/test_p2p_slices.py; no device.
#include "../../gbp_poplar_amd/csrc/gbp_kernels.h"

#include <cstdio>
#include <vector>

int main() {
  const uint32_t cams[] = {0u, 1u, 3u, 5u, 64u, 8000u};
  const int worlds[] = {1, 2, 3, 4, 8};
  int bad = 0, checked = 0;
  for (uint32_t C : cams)
    for (int world : worlds) {
      std::vector<int> owners(C, 0);
      const uint32_t widest = (C + (uint32_t)world - 1u) / (uint32_t)world;
      uint32_t expect_lo = 0;
      for (int s = 0; s < world; ++s) {
        uint32_t lo = ~0u, hi = ~0u;
        gbp::slice_bounds(C, world, s, &lo, &hi);
        bool ok = lo == expect_lo && lo <= hi && hi <= C && hi - lo <= widest && hi - lo >= C / (uint32_t)world;
        if (ok)
          for (uint32_t c = lo; c < hi; ++c) owners[c] += 1;
        if (!ok) {
          std::fprintf(stderr, "slice_bounds(%u, %d, %d) = [%u, %u): expected to start at %u, at most %u wide\n", C, world, s, lo, hi, expect_lo, widest);
          ++bad;
        }
        expect_lo = hi;
        ++checked;
      }
      if (expect_lo != C) {
        std::fprintf(stderr, "slice_bounds(%u, %d, .): the last slice ends at %u\n", C, world, expect_lo);
        ++bad;
      }
      for (uint32_t c = 0; c < C; ++c)
        if (owners[c] != 1) {
          std::fprintf(stderr, "slice_bounds(%u, %d, .): camera %u has %d owners\n", C, world, c, owners[c]);
          ++bad;
          break;
        }
    }
  if (bad) return 1;
  std::printf("slice_bounds: ok (%d slices)\n", checked);
  return 0;
}
