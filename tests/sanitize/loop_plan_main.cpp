// The pass planner of the loop drivers (PassWalk, csrc/gbp_loop_plan.hpp) under ASan + UBSan, on its own: every walk is compared with
// the loop as the reference writes it (ba/ba.cpp:1001-1008), transcribed once below.  Built and run by tests/test_loop_plan_cpu.py; no
// device, no HIP.
#include "../../gbp_poplar_amd/csrc/gbp_loop_plan.hpp"

#include <cstdio>
#include <vector>

using namespace gbp;

static int bad = 0;
static long checked = 0;
#define CHECK(cond)                                                                                                        \
  do {                                                                                                                     \
    ++checked;                                                                                                             \
    if (!(cond)) {                                                                                                         \
      if (++bad <= 20) std::fprintf(stderr, "line %d: %s  [n %d i0 %u steps %u cap %d inside %d]\n", __LINE__, #cond, g_n, g_i0, g_steps, g_cap, g_inside); \
    }                                                                                                                      \
  } while (0)
static int g_n, g_cap, g_inside;
static unsigned g_i0, g_steps;

// The reference's loop, literally: events in order, 'W' = WEAKEN_PRIORS, 'P' = GBP_PROG, each with the loop index it belongs to.
struct Event { char what; unsigned i; };
static std::vector<Event> literal_loop(int n, unsigned i0, unsigned steps) {
  std::vector<Event> ev;
  unsigned i = i0;
  for (int k = 0; k < n; ++k, ++i) {      // for (i = i0; i < i0 + n; ++i), written so that an i0 near 2^32 wraps instead of ending at once
    if ((i + 1) % 2 == 0 && i < 2 * steps) ev.push_back({'W', i});
    ev.push_back({'P', i});
  }
  return ev;
}

// The walk's events: the weakening in front of a piece, then per pass of the piece its interior weakening (not in front of the
// first) and the pass.  Checks the shape of the pieces on the way.
static std::vector<Event> walk(int n, unsigned i0, unsigned steps2, int cap, bool inside, bool front_done, int* pieces) {
  std::vector<Event> ev;
  *pieces = 0;
  int at = 0;
  PassWalk w(n, i0, steps2, front_done);
  CHECK(w.left() == (n > 0 ? n : 0));
  while (!w.done()) {
    const bool weakens = w.weakens();
    const Piece shown = w.peek(cap, inside);
    const Piece p = w.next(cap, inside);
    CHECK(shown.first == p.first && shown.m == p.m && shown.at == p.at && shown.weaken == p.weaken);
    CHECK(p.m >= 1 && p.m <= cap);                        // none empty, none longer than cap
    CHECK(p.at == at && p.first == i0 + (unsigned)at);    // they tile the passes in order
    CHECK(p.weaken == weakens);
    if (p.m < 1) break;
    if (p.weaken) ev.push_back({'W', p.first});
    for (int k = 0; k < p.m; ++k) {
      const unsigned i = p.first + (unsigned)k;
      if (k > 0 && weakens_before(i, steps2)) {
        CHECK(inside);                                    // weaken_inside = 0: no piece has an interior weakening
        ev.push_back({'W', i});
      }
      ev.push_back({'P', i});
    }
    at += p.m;
    ++*pieces;
    CHECK(w.left() == n - at && (w.done() || w.index() == i0 + (unsigned)at));
  }
  CHECK(at == (n > 0 ? n : 0));
  CHECK(w.peek(cap, inside).m == 0 && !w.weakens());
  return ev;
}

static bool same(const std::vector<Event>& a, const std::vector<Event>& b) {
  if (a.size() != b.size()) return false;
  for (size_t k = 0; k < a.size(); ++k)
    if (a[k].what != b[k].what || a[k].i != b[k].i) return false;
  return true;
}

static void check_one(int n, unsigned i0, unsigned steps, int cap, bool inside) {
  g_n = n; g_i0 = i0; g_steps = steps; g_cap = cap; g_inside = inside;
  const unsigned steps2 = 2u * steps;
  const std::vector<Event> want = literal_loop(n, i0, steps);
  int pieces = 0;
  const std::vector<Event> got = walk(n, i0, steps2, cap, inside, false, &pieces);
  CHECK(same(got, want));                                 // the weakenings: as many, at the same positions; the passes: all, in order
  if (inside && cap >= n) CHECK(pieces == (n > 0 ? 1 : 0));
  if (steps == 0)
    for (const Event& e : got) CHECK(e.what == 'P');
  // front_done: the same walk without the weakening in front of pass i0, which the caller has run
  std::vector<Event> rest = want;
  if (!rest.empty() && rest[0].what == 'W') rest.erase(rest.begin());
  int pieces_fd = 0;
  CHECK(same(walk(n, i0, steps2, cap, inside, true, &pieces_fd), rest));
  CHECK(pieces_fd == pieces);
  // the arithmetic under the walk
  if (n > 0) {
    const int run = weakening_free_run(n, i0, steps2);
    CHECK(run >= 1 && run <= n);
    for (int k = 1; k < run; ++k) CHECK(!weakens_before(i0 + (unsigned)k, steps2));
    CHECK(run == n || weakens_before(i0 + (unsigned)run, steps2));
    CHECK(piece_passes(n, i0, steps2, inside, cap) == (inside ? (n < cap ? n : cap) : (run < cap ? run : cap)));
  }
}

int main() {
  const int caps[6] = {1, 2, 3, 7, 512, 4096};
  for (int n = 0; n <= 40; ++n)
    for (unsigned i0 = 0; i0 <= 12; ++i0)
      for (unsigned steps = 0; steps <= 8; ++steps)
        for (int cap : caps)
          for (int inside = 0; inside < 2; ++inside) check_one(n, i0, steps, cap, inside != 0);
  // unsigned arithmetic at the edges: gbp_ba_loop admits steps < 2^30, so steps2 reaches 2^31 - 2; loop indices round it, round 2^31,
  // above it, and round 2^32, where the index wraps as the literal loop's does
  const unsigned big_steps[3] = {(1u << 30) - 1u, (1u << 30) - 2u, 1u << 29};
  const unsigned big_i0[9] = {(1u << 31) - 5u, (1u << 31) - 3u, (1u << 31) - 2u, (1u << 31) - 1u, 1u << 31, (1u << 31) + 1u, 3000000000u, 0xfffffffau, 0xffffffffu};
  for (unsigned steps : big_steps)
    for (unsigned i0 : big_i0)
      for (int n : {0, 1, 2, 5, 12, 40})
        for (int cap : caps)
          for (int inside = 0; inside < 2; ++inside) check_one(n, i0, steps, cap, inside != 0);
  for (unsigned steps : {0u, 3u, 8u})
    for (unsigned i0 : big_i0)
      for (int inside = 0; inside < 2; ++inside) check_one(12, i0, steps, 7, inside != 0);
  // the largest call: one piece under kNoCap, no overflow in the piece's bookkeeping
  {
    g_n = INT_MAX; g_i0 = 5; g_steps = 0; g_cap = kNoCap; g_inside = 1;
    PassWalk w(INT_MAX, 5u, 0u);
    const Piece p = w.next(kNoCap, true);
    CHECK(p.m == INT_MAX && p.first == 5u && p.at == 0 && !p.weaken && w.done() && w.left() == 0);
  }
  // a negative n is an empty walk
  {
    g_n = -3;
    PassWalk w(-3, 1u, 8u);
    CHECK(w.done() && !w.weakens() && w.left() == 0);
  }
  if (bad) { std::fprintf(stderr, "loop_plan: %d of %ld checks failed\n", bad, checked); return 1; }
  std::printf("loop_plan: ok (%ld checks)\n", checked);
  return 0;
}
