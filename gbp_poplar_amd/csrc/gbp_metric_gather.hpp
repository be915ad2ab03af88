// gbp_metric_gather.hpp — the cross-rank sum of the per-pass metric records of a burst, as the CLIs' multi-rank loops take it
// (ba_main.cpp, slam_main.cpp through cli_common.hpp).  A rank's gbp_ba_loop leaves the LOCAL shard's sums, one record per pass; the
// launcher has mapped a shared area of [2 parities][world][kMetricBurstMax] records before it forked the ranks; a rank writes its row of
// the burst's parity, passes ONE gbp_comm_barrier and adds the rows in rank order with exactly gbp_eval_global's arithmetic: every field as
// a double, acc = 0 + r0 + r1 ..., the counters back through + 0.5 — the same bits on every rank, and the bits gbp_eval_global returns.
// One barrier per burst suffices: a rank that writes its row of burst b + 2 (the parity of burst b again) has passed the barrier of burst
// b + 1, which every rank reaches only after it has read the rows of burst b — a rank is at most one barrier ahead.
// No HIP and no library call in here: plain C++ on the C-ABI's record, tested as a stand-alone host program
// (tests/sanitize/metric_gather_main.cpp).
#pragma once

#include "../../include/gbp_mi355x.h"

#include <cstddef>
#include <cstdint>

namespace gbp {

constexpr int kMetricBurstMax = 128;      // passes per burst of a multi-rank CLI loop

inline size_t metric_area_bytes(int world) { return sizeof(gbp_eval_out) * 2u * (size_t)world * (size_t)kMetricBurstMax; }

// the row of `rank` in the rows of one parity
inline gbp_eval_out* metric_row(void* area, int world, int parity, int rank) {
  return static_cast<gbp_eval_out*>(area) + ((size_t)(parity & 1) * (size_t)world + (size_t)rank) * (size_t)kMetricBurstMax;
}

// out[k] = sum over the ranks, in rank order, of rows[r * kMetricBurstMax + k], k < n (rows: the [world][kMetricBurstMax] records of one parity)
inline void metric_sum_ranks(const gbp_eval_out* rows, int world, int n, gbp_eval_out* out) {
  for (int k = 0; k < n; ++k) {
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int r = 0; r < world; ++r) {
      const gbp_eval_out& o = rows[(size_t)r * (size_t)kMetricBurstMax + (size_t)k];
      const double mine[7] = {o.sum_norm, o.sum_half_sq, (double)o.n_active, (double)o.n_relin, (double)o.n_robust,
                              (double)o.n_nonfinite, (double)o.n_nonpd};
      for (int i = 0; i < 7; ++i) acc[i] = acc[i] + mine[i];
    }
    gbp_eval_out& s = out[k];
    s.sum_norm = acc[0]; s.sum_half_sq = acc[1]; s.n_active = (uint64_t)(acc[2] + 0.5); s.n_relin = (uint64_t)(acc[3] + 0.5);
    s.n_robust = (uint64_t)(acc[4] + 0.5); s.n_nonfinite = (uint64_t)(acc[5] + 0.5); s.n_nonpd = (uint64_t)(acc[6] + 0.5);
  }
}

}  // namespace gbp
