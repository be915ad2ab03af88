// The layouts of the peer-memory transports' buffers (ExchangeLayout, ResultLayout: csrc/gbp_comm.hpp) under ASan + UBSan, on their own,
// for world in {1, 2, 3, 8, 64} x C in {0, 1, 3, 5, 1000}.  X: the 2 * world slots of C * 44 floats are pairwise disjoint and tile the
// buffer from 0 to its end without a gap, parity 1 starts world * C * 44 floats behind parity 0, and bytes() — what a rank allocates
// — is that end, or 16 for the empty buffer of C = 0.  R: one parity holds ceil(C / world) records of kCamRes4 float4, parity 1
// starts behind it, and every slice of slice_bounds fits a parity, the empty slices of C < world included.  Built and run by
// tests/test_p2p_transport.py; no device.
#include "../../gbp_poplar_amd/csrc/gbp_comm.hpp"

#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

static int bad = 0;
#define CHECK(cond, ...)                                      \
  do {                                                        \
    if (!(cond)) {                                            \
      std::fprintf(stderr, "world %d, C %u: ", world, C);     \
      std::fprintf(stderr, __VA_ARGS__);                      \
      std::fprintf(stderr, " (%s)\n", #cond);                 \
      ++bad;                                                  \
    }                                                         \
  } while (0)

int main() {
  const int worlds[] = {1, 2, 3, 8, 64};
  const uint32_t cams[] = {0u, 1u, 3u, 5u, 1000u};
  int checked = 0;
  for (int world : worlds)
    for (uint32_t C : cams) {
      const gbp::ExchangeLayout x{world, C};
      const size_t n = (size_t)C * 44;
      CHECK(x.slot_floats() == n, "a slot is %zu floats", x.slot_floats());
      std::vector<std::pair<size_t, size_t>> slots;      // [begin, end) in floats
      for (int p = 0; p < 2; ++p)
        for (int r = 0; r < world; ++r) slots.emplace_back(x.slot(p, r), x.slot(p, r) + n);
      CHECK(slots.size() == 2 * (size_t)world, "%zu slots", slots.size());
      std::sort(slots.begin(), slots.end());
      size_t end = 0;      // sorted, each slot begins where the one before it ended: pairwise disjoint, no gap
      for (const auto& s : slots) {
        CHECK(s.first == end, "a slot begins at float %zu, the one before it ends at %zu", s.first, end);
        end = s.second;
      }
      CHECK(end == 2 * (size_t)world * n, "the slots end at float %zu", end);
      CHECK(x.bytes() == std::max<size_t>(end * sizeof(float), 16), "bytes() = %zu, the slots end at byte %zu", x.bytes(), end * sizeof(float));
      CHECK(x.bytes() >= 16, "bytes() = %zu", x.bytes());
      CHECK(x.slot(1, 0) - x.slot(0, 0) == (size_t)world * C * 44, "parity 1 starts %zu floats behind parity 0", x.slot(1, 0) - x.slot(0, 0));

      const gbp::ResultLayout rl{world, C};
      CHECK(rl.res4() == ((size_t)C + world - 1) / world * gbp::kCamRes4, "res4 = %zu", rl.res4());
      CHECK(rl.parity_offset(0) == 0 && rl.parity_offset(1) == rl.res4(), "parity 1 starts at float4 %zu", rl.parity_offset(1));
      CHECK(rl.bytes() == std::max<size_t>(2 * rl.res4() * 16, 16), "bytes() = %zu", rl.bytes());
      for (int s = 0; s < world; ++s) {
        uint32_t lo = ~0u, hi = ~0u;
        gbp::slice_bounds(C, world, s, &lo, &hi);
        CHECK(lo <= hi && (size_t)(hi - lo) * gbp::kCamRes4 <= rl.res4(), "slice %d = [%u, %u) does not fit %zu float4", s, lo, hi, rl.res4());
      }
      ++checked;
    }
  if (bad) return 1;
  std::printf("exchange_layout: ok (%d shapes)\n", checked);
  return 0;
}
