// The two pure functions of the sharded default loop under ASan + UBSan, on their own: whether the metric rides in the sharded iteration
// (metric_rides, csrc/gbp_transport.hpp) and the CLIs' rank-order sum of a burst's metric records (metric_sum_ranks,
// csrc/gbp_metric_gather.hpp), which must reproduce gbp_eval_global's arithmetic.  Built and run by tests/test_sharded_metric_cpu.py; no
// device, no HIP.
#include "../../gbp_poplar_amd/csrc/gbp_metric_gather.hpp"
#include "../../gbp_poplar_amd/csrc/gbp_transport.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace gbp;

static int bad = 0, checked = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    ++checked;                                                                   \
    if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++bad; } \
  } while (0)

// gbp_eval_global's sum (gbp_api_comm.cpp), restated over `world` records given in rank order
static gbp_eval_out global_sum(const gbp_eval_out* rec, int world) {
  std::vector<double> all((size_t)7 * world);
  for (int r = 0; r < world; ++r) {
    const gbp_eval_out& o = rec[r];
    const double mine[7] = {o.sum_norm, o.sum_half_sq, (double)o.n_active, (double)o.n_relin, (double)o.n_robust, (double)o.n_nonfinite, (double)o.n_nonpd};
    std::memcpy(&all[(size_t)7 * r], mine, sizeof(mine));
  }
  double acc[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int r = 0; r < world; ++r)
    for (int i = 0; i < 7; ++i) acc[i] = acc[i] + all[(size_t)r * 7 + i];
  gbp_eval_out o{};
  o.sum_norm = acc[0]; o.sum_half_sq = acc[1]; o.n_active = (uint64_t)(acc[2] + 0.5); o.n_relin = (uint64_t)(acc[3] + 0.5);
  o.n_robust = (uint64_t)(acc[4] + 0.5); o.n_nonfinite = (uint64_t)(acc[5] + 0.5); o.n_nonpd = (uint64_t)(acc[6] + 0.5);
  return o;
}

static bool same(const gbp_eval_out& a, const gbp_eval_out& b) {
  return std::memcmp(&a.sum_norm, &b.sum_norm, 8) == 0 && std::memcmp(&a.sum_half_sq, &b.sum_half_sq, 8) == 0 && a.n_active == b.n_active &&
         a.n_relin == b.n_relin && a.n_robust == b.n_robust && a.n_nonfinite == b.n_nonfinite && a.n_nonpd == b.n_nonpd;
}

// pass k of rank r: sums whose order matters in fp64 (1e16 + 1 + 1 ... != ... + 1 + 1 + 1e16), counters near 2^32
static gbp_eval_out record(int r, int k, int world) {
  gbp_eval_out o{};
  o.sum_norm = r == 0 ? 1e16 : 1.0 + 0.25 * k;
  o.sum_half_sq = r == world - 1 ? -1e16 : 3.0 + r + 1e-3 * k;
  o.n_active = 4294967295ull - (uint64_t)r;
  o.n_relin = 4294967296ull + (uint64_t)k;
  o.n_robust = (uint64_t)(r * 7 + k);
  o.n_nonfinite = r == 0 ? 1u : 0u;
  o.n_nonpd = (uint64_t)k;
  return o;
}

static void check_sum(int world) {
  const int n = kMetricBurstMax;
  std::vector<char> area(metric_area_bytes(world), (char)0x5a);      // exactly the bytes the launcher maps: ASan sees an index past them
  for (int parity = 0; parity < 2; ++parity) {
    for (int r = 0; r < world; ++r) {
      gbp_eval_out* row = metric_row(area.data(), world, parity, r);
      for (int k = 0; k < n; ++k) row[k] = k == 5 ? gbp_eval_out{} : record(r, k + parity, world);      // pass 5: a record of zeros on every rank
    }
  }
  for (int parity = 0; parity < 2; ++parity) {
    std::vector<gbp_eval_out> out((size_t)n);
    const gbp_eval_out* rows = metric_row(area.data(), world, parity, 0);
    metric_sum_ranks(rows, world, n, out.data());
    bool order_matters = false;
    for (int k = 0; k < n; ++k) {
      std::vector<gbp_eval_out> in((size_t)world), rev((size_t)world);
      for (int r = 0; r < world; ++r) in[(size_t)r] = rows[(size_t)r * kMetricBurstMax + k];
      for (int r = 0; r < world; ++r) rev[(size_t)r] = in[(size_t)(world - 1 - r)];
      CHECK(same(out[(size_t)k], global_sum(in.data(), world)));
      if (!same(global_sum(in.data(), world), global_sum(rev.data(), world))) order_matters = true;
    }
    CHECK(world < 3 || order_matters);      // (a + b == b + a: the reversed order shows from three ranks on)
    const gbp_eval_out zero{};
    CHECK(same(out[5], zero));
    CHECK(out[0].n_active == (uint64_t)world * 4294967295ull - (uint64_t)(world * (world - 1) / 2));
    CHECK(out[0].n_relin == (uint64_t)world * (4294967296ull + (uint64_t)parity));
    CHECK(out[0].n_nonfinite == 1u);
  }
  // the two parities do not overlap and together fill the area
  CHECK(reinterpret_cast<char*>(metric_row(area.data(), world, 1, 0)) - area.data() == (std::ptrdiff_t)(metric_area_bytes(world) / 2));
  CHECK(reinterpret_cast<char*>(metric_row(area.data(), world, 1, world - 1) + kMetricBurstMax) == area.data() + area.size());
}

int main() {
  for (int world : {1, 2, 8}) check_sum(world);
  {  // three ranks, hand-made: the rank order gives (1e16 + 1) + 1 = 1e16, the reversed order (1 + 1) + 1e16 = 1e16 + 2
    std::vector<gbp_eval_out> rows((size_t)3 * kMetricBurstMax);
    rows[0].sum_norm = 1e16; rows[(size_t)kMetricBurstMax].sum_norm = 1.0; rows[(size_t)2 * kMetricBurstMax].sum_norm = 1.0;
    gbp_eval_out out{};
    metric_sum_ranks(rows.data(), 3, 1, &out);
    CHECK(out.sum_norm == 1e16);
    CHECK((1.0 + 1.0) + 1e16 != out.sum_norm);
  }

  // metric_rides: every transport at world 1 and 4
  const Transport all[] = {Transport::Rccl, Transport::HostStaged, Transport::P2p, Transport::P2pSlices};
  for (Transport t : all)
    for (int world : {1, 4}) {
      const char* why = nullptr;
      const bool rides = metric_rides(t, world, true, false, false, &why);
      const bool want = !(t == Transport::P2pSlices && world > 1);
      CHECK(rides == want);
      CHECK(why != nullptr && (rides ? why[0] == 0 : why[0] != 0));
      if (!rides) CHECK(std::strstr(why, transport_name(t)) != nullptr);      // the reason names the transport
      CHECK(metric_rides(t, world, true, false, false, nullptr) == want);     // (no reason asked for)
      // non-hoisted, profiling on, capturing: never, each with a reason of its own
      const char *w1 = nullptr, *w2 = nullptr, *w3 = nullptr;
      CHECK(!metric_rides(t, world, false, false, false, &w1) && w1 && w1[0]);
      CHECK(!metric_rides(t, world, true, true, false, &w2) && w2 && w2[0]);
      CHECK(!metric_rides(t, world, true, false, true, &w3) && w3 && w3[0]);
      CHECK(w1 && w2 && w3 && std::strcmp(w1, w2) != 0 && std::strcmp(w2, w3) != 0 && std::strcmp(w1, w3) != 0);
    }
  for (Transport t : {Transport::Auto, Transport::Measured}) {      // no communicator is ever OF these kinds
    const char* why = nullptr;
    CHECK(!metric_rides(t, 1, true, false, false, &why) && why && why[0]);
  }
  if (bad) { std::printf("metric_gather: %d of %d checks failed\n", bad, checked); return 1; }
  std::printf("metric_gather: ok (%d checks)\n", checked);
  return 0;
}
