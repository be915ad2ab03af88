// gbp_transport.hpp — the transports of the sharded exchange by name, and how the measured transport chooses between them.  The values
// are those of the public gbp_comm_init(ctx, region, transport) argument (include/gbp_mi355x_multi.h).  No HIP in here: the CLIs, plain
// C++ on top of the C-ABI, include it next to the library (gbp_comm.hpp), and the pure functions at the end — who may run
// (eligible_candidates), who won (choose_transport), whether the metric rides in the sharded iteration (metric_rides) — are tested as
// stand-alone host programs (tests/sanitize/transport_choice_main.cpp, metric_gather_main.cpp).
#pragma once

#include <cstdint>
#include <cstring>

namespace gbp {

enum class Transport : int {
  Auto = 0,        // RCCL when every rank sits on its own GPU, host-staged otherwise
  Rccl = 1,
  HostStaged = 2,
  P2p = 3,         // direct peer memory; never chosen by Auto
  P2pSlices = 4,   // the same, cameras reduced in slices; never chosen by Auto
  Measured = 5,    // gbp_comm_init times every transport this group of ranks can form and attaches the fastest
};

constexpr int kCommMaxWorld = 64;

inline const char* transport_name(Transport t) {
  static const char* const names[] = {"none", "rccl", "host-staged", "p2p", "p2p-slices", "measured"};
  return (int)t >= 0 && (int)t <= 5 ? names[(int)t] : "host-staged";
}

// What a rank publishes about itself in the region before any communicator exists (64 bytes: the slot that held the bus id alone).
struct RankFacts {
  char bus[48];           // PCI bus id of the rank's GPU
  uint64_t peer_mask;     // bit r: hipDeviceCanAccessPeer towards rank r's GPU (the same GPU counts); bit `rank` set
  uint32_t has_rccl;      // librccl resolves on this rank (asked only when every rank has a GPU of its own)
  uint32_t pad;
};
static_assert(sizeof(RankFacts) == 64, "RankFacts takes the region's 64-byte per-rank slot");

inline bool same_gpu(const RankFacts& a, const RankFacts& b) { return std::strncmp(a.bus, b.bus, sizeof(a.bus)) == 0; }
inline bool any_shared_gpu(const RankFacts* f, int world) {
  for (int a = 0; a < world; ++a)
    for (int b = a + 1; b < world; ++b)
      if (same_gpu(f[a], f[b])) return true;
  return false;
}

// One thing the measurement can time: a transport, and for the stream-ordered one the schedule of its camera side.
struct Candidate {
  Transport transport = Transport::HostStaged;
  bool two_streams = false;
  bool eligible = false;
  const char* reason = "";      // why not (static text), "" when eligible
};
constexpr int kMaxCandidates = 8;
struct Candidates {
  int n = 0;
  int baseline = -1;            // what transport 0 would have attached (rule for the transport, rule or environment for the schedule)
  Candidate c[kMaxCandidates];
};

// The same list on every rank, from the table every rank holds after the barrier.  single_stream: GBP_COMM_SINGLE_STREAM as the caller
// read it (-1 not set, 0, 1) — where it is set, only that schedule of RCCL is listed.
//   RCCL        one GPU per rank, librccl on every rank
//   p2p(-slices) every pair of ranks on one GPU or with peer access in both directions
//   host-staged always
// The baseline is the rule's choice; where the rule's choice cannot be formed (own GPUs, no librccl), host-staged.
inline Candidates eligible_candidates(const RankFacts* f, int world, int single_stream) {
  Candidates cl;
  const bool shared = any_shared_gpu(f, world);
  bool rccl_all = true, peers_ok = true;
  for (int a = 0; a < world; ++a) {
    rccl_all = rccl_all && f[a].has_rccl != 0;
    for (int b = 0; b < world; ++b)
      if (a != b && !same_gpu(f[a], f[b]) && !(((f[a].peer_mask >> b) & 1u) && ((f[b].peer_mask >> a) & 1u))) peers_ok = false;
  }
  const char* no_rccl = shared ? "two ranks share a GPU" : !rccl_all ? "librccl does not resolve on every rank" : "";
  const char* no_peer = peers_ok ? "" : "no mutual peer access between the ranks' GPUs";
  const bool rule_two = single_stream >= 0 ? single_stream == 0 : world > 2;      // (comm_attach's rule for the schedule)
  auto add = [&](Transport t, bool two, const char* why) {
    Candidate& k = cl.c[cl.n++];
    k.transport = t; k.two_streams = two; k.eligible = why[0] == 0; k.reason = why;
    return cl.n - 1;
  };
  int rccl_rule = -1;
  for (int two = 0; two < 2; ++two) {
    if (single_stream >= 0 && (two == 1) != rule_two) continue;
    const int i = add(Transport::Rccl, two == 1, no_rccl);
    if ((two == 1) == rule_two) rccl_rule = i;
  }
  const int host = add(Transport::HostStaged, false, "");
  add(Transport::P2p, false, no_peer);
  add(Transport::P2pSlices, false, no_peer);
  cl.baseline = !shared && cl.c[rccl_rule].eligible ? rccl_rule : host;
  return cl;
}

// Does the metric of a loop with the metric after every pass (gbp_ba_loop, gbp_iterate_eval_each) ride in the iterations of a ctx WITH a
// communicator — the metric of iteration k collected by the sweep of iteration k + 1, nothing of a burst waiting for the metric — or does
// the ctx run the per-pass loop (gbp_iterate(1), k_means, k_eval, a fold and a host wait per pass)?  It rides when the means are hoisted,
// per-stage profiling is off, the caller is not capturing the ctx's stream, and the transport's camera combine can leave the cameras'
// metric records: every one but the sliced peer-memory transport with more than one rank, whose gathered cameras arrive as finished
// records without them.  *why (may be NULL) = "" when it rides, the reason (static text) when it does not.
inline bool metric_rides(Transport kind, int world, bool hoist, bool profile_stages, bool capturing, const char** why) {
  const char* r = "";
  if (!hoist) r = "per_factor_mu = 1: the belief update computes no hoisted means for the metric to ride with";
  else if (profile_stages) r = "per-stage profiling brackets every launch of a pass";
  else if (capturing) r = "the caller is capturing the ctx's stream";
  else if (kind == Transport::P2pSlices && world > 1) r = "transport p2p-slices with more than one rank: the gathered camera records carry no metric records";
  else if (kind != Transport::Rccl && kind != Transport::HostStaged && kind != Transport::P2p && kind != Transport::P2pSlices)
    r = "the ctx has no communicator of a known transport";
  if (why) *why = r;
  return r[0] == 0;
}

struct Choice {
  int winner = -1, runner_up = -1;        // indices into Candidates::c (runner_up: -1 when nothing else was measured)
  double figure[kMaxCandidates] = {};     // us per exchange, MAX over the ranks; the baseline's: the better of its two; 0 = not measured
  double base_first = 0, base_last = 0, noise = 0;
};

// The decision, from the gathered table alone: table[m * world + r] = what rank r measured (us per exchange) for candidate m, row
// cl.n = the baseline's second measurement.  A candidate's figure is the MAX over the ranks.  The baseline was measured first and last;
// the distance between its two figures is this run's noise estimate, and another candidate wins only if it beats the better of the two
// by MORE than that — ties and noise keep what transport 0 would have attached.  A candidate that is not eligible, or whose figure is not
// a finite positive number on every rank, never wins.
inline Choice choose_transport(const Candidates& cl, const double* table, int world) {
  Choice ch;
  auto row_max = [&](int m) {
    double mx = 0;
    for (int r = 0; r < world; ++r) {
      const double v = table[(size_t)m * world + r];
      if (!(v > 0) || !(v - v == 0)) return 0.0;      // not measured / not finite on some rank
      mx = v > mx ? v : mx;
    }
    return mx;
  };
  ch.base_first = row_max(cl.baseline);
  ch.base_last = row_max(cl.n);
  const double lo = ch.base_first < ch.base_last ? ch.base_first : ch.base_last, hi = ch.base_first < ch.base_last ? ch.base_last : ch.base_first;
  const bool base_ok = lo > 0;
  ch.noise = base_ok ? hi - lo : 0;
  int best = -1, second = -1;      // among the others, by figure (the earlier candidate on a tie)
  for (int i = 0; i < cl.n; ++i) {
    if (i == cl.baseline) { ch.figure[i] = base_ok ? lo : 0; continue; }
    ch.figure[i] = cl.c[i].eligible ? row_max(i) : 0;
    if (!(ch.figure[i] > 0)) continue;
    if (best < 0 || ch.figure[i] < ch.figure[best]) { second = best; best = i; }
    else if (second < 0 || ch.figure[i] < ch.figure[second]) second = i;
  }
  if (best >= 0 && (!base_ok || ch.figure[best] < lo - ch.noise)) {
    ch.winner = best;
    ch.runner_up = base_ok && (second < 0 || lo <= ch.figure[second]) ? cl.baseline : second;
  } else {
    ch.winner = cl.baseline;
    ch.runner_up = best;
  }
  return ch;
}

}  // namespace gbp
