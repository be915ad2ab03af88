// The two pure functions of the measured transport (csrc/gbp_transport.hpp) under ASan + UBSan, on their own: which transports a group
// of ranks may form (eligible_candidates, from the facts table of the region) and which one the gathered timings select
// (choose_transport).  Built and run by tests/test_measured_transport.py; no device, no HIP.
#include "../../gbp_poplar_amd/csrc/gbp_transport.hpp"

#include <cmath>
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

// world ranks; gpu[r] = which GPU rank r sits on; access[a][b] = GPU a reaches GPU b; rccl[r]
static std::vector<RankFacts> facts(int world, const int* gpu, const bool (*access)[4], const bool* rccl) {
  std::vector<RankFacts> f((size_t)world);
  for (int r = 0; r < world; ++r) {
    std::memset(&f[r], 0, sizeof(RankFacts));
    std::snprintf(f[r].bus, sizeof(f[r].bus), "0000:%02x:00.0", 3 + gpu[r]);
    for (int q = 0; q < world; ++q)
      if (gpu[q] == gpu[r] || access[gpu[r]][gpu[q]]) f[r].peer_mask |= (uint64_t)1 << q;
    f[r].has_rccl = rccl[r] ? 1u : 0u;
  }
  return f;
}

static int find(const Candidates& cl, Transport t, bool two) {
  for (int i = 0; i < cl.n; ++i)
    if (cl.c[i].transport == t && cl.c[i].two_streams == two) return i;
  return -1;
}

// table of cl.n + 1 rows, every rank the same figure per row
static std::vector<double> table(const Candidates& cl, int world, const double* us /*[cl.n + 1]*/) {
  std::vector<double> t((size_t)(cl.n + 1) * world);
  for (int m = 0; m <= cl.n; ++m)
    for (int r = 0; r < world; ++r) t[(size_t)m * world + r] = us[m];
  return t;
}

int main() {
  const bool all[4][4] = {{1, 1, 1, 1}, {1, 1, 1, 1}, {1, 1, 1, 1}, {1, 1, 1, 1}};
  const bool none[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  const bool one_way[4][4] = {{1, 1, 1, 1}, {0, 1, 1, 1}, {1, 1, 1, 1}, {1, 1, 1, 1}};      // GPU 1 does not reach GPU 0
  const bool yes[4] = {true, true, true, true}, no[4] = {false, false, false, false}, miss2[4] = {true, true, false, true};
  const int same[4] = {0, 0, 0, 0}, own[4] = {0, 1, 2, 3}, pair[4] = {0, 0, 1, 1};

  // ---- who may run ----
  {  // every rank on ONE GPU (the test rig): no RCCL, everything else; the baseline is host-staged
    for (int world : {2, 4}) {
      const auto f = facts(world, same, none, no);
      const Candidates cl = eligible_candidates(f.data(), world, -1);
      CHECK(cl.n == 5);
      const int r1 = find(cl, Transport::Rccl, false), r2 = find(cl, Transport::Rccl, true), h = find(cl, Transport::HostStaged, false);
      const int p = find(cl, Transport::P2p, false), s = find(cl, Transport::P2pSlices, false);
      CHECK(r1 >= 0 && r2 >= 0 && h >= 0 && p >= 0 && s >= 0);
      CHECK(!cl.c[r1].eligible && !cl.c[r2].eligible && std::strstr(cl.c[r1].reason, "share a GPU"));
      CHECK(cl.c[h].eligible && cl.c[p].eligible && cl.c[s].eligible && cl.c[h].reason[0] == 0);
      CHECK(cl.baseline == h);
    }
  }
  {  // own GPUs, librccl everywhere, full peer access: everything; the baseline is RCCL in the rule's schedule (two streams from 4 ranks)
    for (int world : {2, 4}) {
      const auto f = facts(world, own, all, yes);
      const Candidates cl = eligible_candidates(f.data(), world, -1);
      CHECK(cl.n == 5);
      for (int i = 0; i < cl.n; ++i) CHECK(cl.c[i].eligible);
      CHECK(cl.baseline == find(cl, Transport::Rccl, world > 2));
      // GBP_COMM_SINGLE_STREAM set: that schedule only, and it is the baseline
      for (int ss : {0, 1}) {
        const Candidates ce = eligible_candidates(f.data(), world, ss);
        CHECK(ce.n == 4 && find(ce, Transport::Rccl, ss == 1) < 0 && ce.baseline == find(ce, Transport::Rccl, ss == 0));
      }
    }
  }
  {  // own GPUs without peer access: RCCL and host-staged only
    const auto f = facts(4, own, none, yes);
    const Candidates cl = eligible_candidates(f.data(), 4, -1);
    CHECK(!cl.c[find(cl, Transport::P2p, false)].eligible && !cl.c[find(cl, Transport::P2pSlices, false)].eligible);
    CHECK(std::strstr(cl.c[find(cl, Transport::P2p, false)].reason, "peer access"));
    CHECK(cl.c[find(cl, Transport::Rccl, true)].eligible && cl.baseline == find(cl, Transport::Rccl, true));
  }
  {  // access in one direction only is not mutual
    const auto f = facts(4, own, one_way, yes);
    const Candidates cl = eligible_candidates(f.data(), 4, -1);
    CHECK(!cl.c[find(cl, Transport::P2p, false)].eligible && !cl.c[find(cl, Transport::P2pSlices, false)].eligible);
  }
  {  // librccl missing on one rank: no RCCL for anybody, the baseline falls to host-staged
    const auto f = facts(4, own, all, miss2);
    const Candidates cl = eligible_candidates(f.data(), 4, -1);
    CHECK(!cl.c[find(cl, Transport::Rccl, false)].eligible && std::strstr(cl.c[find(cl, Transport::Rccl, true)].reason, "librccl"));
    CHECK(cl.baseline == find(cl, Transport::HostStaged, false) && cl.c[find(cl, Transport::P2p, false)].eligible);
  }
  {  // two GPUs, two ranks on each, the GPUs reach each other: no RCCL (shared), peer transports allowed; without access: host-staged alone
    const auto f = facts(4, pair, all, yes);
    const Candidates cl = eligible_candidates(f.data(), 4, -1);
    CHECK(!cl.c[find(cl, Transport::Rccl, true)].eligible && cl.c[find(cl, Transport::P2p, false)].eligible);
    const auto g = facts(4, pair, none, yes);
    const Candidates cg = eligible_candidates(g.data(), 4, -1);
    int n_ok = 0;
    for (int i = 0; i < cg.n; ++i) n_ok += cg.c[i].eligible;
    CHECK(n_ok == 1 && cg.c[cg.baseline].transport == Transport::HostStaged);
  }

  // ---- who wins (the one-GPU list: rccl x 2 not eligible, host-staged = baseline, p2p, p2p-slices) ----
  const int world = 4;
  const auto f = facts(world, same, none, no);
  const Candidates cl = eligible_candidates(f.data(), world, -1);
  const int h = find(cl, Transport::HostStaged, false), p = find(cl, Transport::P2p, false), s = find(cl, Transport::P2pSlices, false);
  const int r1 = find(cl, Transport::Rccl, false);
  auto us = [&](double rccl, double host_first, double p2p, double slices, double host_last) {
    std::vector<double> v((size_t)cl.n + 1, 0.0);
    v[r1] = rccl; v[find(cl, Transport::Rccl, true)] = rccl; v[h] = host_first; v[p] = p2p; v[s] = slices; v[cl.n] = host_last;
    return v;
  };
  {  // a tie keeps the baseline
    const Choice ch = choose_transport(cl, table(cl, world, us(0, 60, 60, 60, 60).data()).data(), world);
    CHECK(ch.winner == h && ch.noise == 0 && ch.figure[h] == 60 && ch.figure[p] == 60 && ch.runner_up == p);
  }
  {  // a gain inside the baseline's own spread keeps the baseline: better of the two 60, spread 5, 56 is not below 55
    const Choice ch = choose_transport(cl, table(cl, world, us(0, 60, 56, 70, 65).data()).data(), world);
    CHECK(ch.winner == h && ch.noise == 5 && ch.base_first == 60 && ch.base_last == 65 && ch.runner_up == p);
    // ... exactly at the bound: still the baseline (it must be beaten by MORE than the spread)
    const Choice eq = choose_transport(cl, table(cl, world, us(0, 65, 55, 70, 60).data()).data(), world);
    CHECK(eq.winner == h && eq.figure[h] == 60);
  }
  {  // a clear winner is taken; the runner-up is the next best, the baseline included
    const Choice ch = choose_transport(cl, table(cl, world, us(0, 60, 35, 50, 62).data()).data(), world);
    CHECK(ch.winner == p && ch.runner_up == s && ch.figure[p] == 35);
    const Choice c2 = choose_transport(cl, table(cl, world, us(0, 60, 35, 90, 62).data()).data(), world);
    CHECK(c2.winner == p && c2.runner_up == h);
    const Choice c3 = choose_transport(cl, table(cl, world, us(0, 60, 300, 20, 61).data()).data(), world);
    CHECK(c3.winner == s && c3.runner_up == h);
  }
  {  // a candidate that is not eligible never wins, whatever its row says
    const Choice ch = choose_transport(cl, table(cl, world, us(1, 60, 80, 90, 61).data()).data(), world);
    CHECK(ch.winner == h && ch.figure[r1] == 0 && ch.runner_up == p);
  }
  {  // the figure is the MAX over the ranks: fast on three ranks, slow on one, loses; a rank without a finite positive figure rules it out
    std::vector<double> t = table(cl, world, us(0, 60, 10, 90, 61).data());
    t[(size_t)p * world + 2] = 500;
    const Choice ch = choose_transport(cl, t.data(), world);
    CHECK(ch.winner == h && ch.figure[p] == 500);
    t[(size_t)p * world + 2] = 0;
    CHECK(choose_transport(cl, t.data(), world).winner == h);
    t[(size_t)p * world + 2] = std::nan("");
    CHECK(choose_transport(cl, t.data(), world).winner == h);
  }
  {  // every rank evaluates its own copy of the gathered table and of the facts: the same list, the same answer
    const std::vector<double> t = table(cl, world, us(0, 61.5, 34.25, 50.125, 60.75).data());
    const Choice first = choose_transport(cl, t.data(), world);
    for (int rank = 0; rank < world; ++rank) {
      const std::vector<RankFacts> fr(f);
      const std::vector<double> tr(t);
      const Candidates cr = eligible_candidates(fr.data(), world, -1);
      CHECK(cr.n == cl.n && cr.baseline == cl.baseline);
      for (int i = 0; i < cr.n; ++i) CHECK(cr.c[i].transport == cl.c[i].transport && cr.c[i].two_streams == cl.c[i].two_streams && cr.c[i].eligible == cl.c[i].eligible);
      const Choice ch = choose_transport(cr, tr.data(), world);
      CHECK(ch.winner == first.winner && ch.runner_up == first.runner_up && ch.noise == first.noise);
      CHECK(std::memcmp(ch.figure, first.figure, sizeof(ch.figure)) == 0);
    }
    CHECK(first.winner == p);
  }
  if (bad) return 1;
  std::printf("transport_choice: ok (%d checks)\n", checked);
  return 0;
}
