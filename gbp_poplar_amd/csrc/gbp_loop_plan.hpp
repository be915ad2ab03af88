// gbp_loop_plan.hpp — the reference's iteration loop (ba/ba.cpp:1001-1028, slam.cpp:1048-1103) as a plan of pieces.  The loop is
//   for (i = i0; i < i0 + n; ++i) { if ((i + 1) % 2 == 0 && i < 2 * steps) WEAKEN_PRIORS; GBP_PROG; [metric] }
// and every driver of the C-ABI (iterate_passes, iterate_weaken_plain, iterate_passes_eval, gbp_ba_loop, the replay of persist_recover)
// runs it as a sequence of pieces: m passes from loop index `first`, with or without a weakening in front of them.  Where the pieces
// are cut is decided here, once; what a driver does with a piece (a launch of the persistent kernel, a hipGraph replay, the metric
// riding) and with its weakening (a launch of its own, riding in the belief update before it, applied by the kernel) stays with the
// driver.  No HIP in here: pure functions of plain values, tested as a stand-alone host program (tests/sanitize/loop_plan_main.cpp).
#pragma once

#include <climits>
#include <cstdint>

namespace gbp {

// WEAKEN_PRIORS runs in front of pass i iff (i + 1) % 2 == 0 and i < 2 * steps (= steps2).  Loop indices are unsigned and wrap as the
// literal loop's would; gbp_ba_loop admits steps < 2^30, so steps2 itself never wraps.
inline bool weakens_before(unsigned i, unsigned steps2) { return ((i + 1u) % 2u == 0u) && i < steps2; }

// passes from loop index i up to (not including) the next weakening after it, at most n
inline int weakening_free_run(int n, unsigned i, unsigned steps2) {
  int m = 1;
  while (m < n && !weakens_before(i + (unsigned)m, steps2)) ++m;
  return m;
}

// passes from loop index i that ONE piece takes, at most cap of the n left.  weaken_inside: whoever runs the piece applies the
// weakenings in front of its later passes itself (the tagged-record persistent kernel); otherwise the piece ends in front of the next
// weakening (the barrier kernel of the test-hooks build, every run of the two-kernel path).
inline int piece_passes(int n, unsigned i, unsigned steps2, bool weaken_inside, int cap) {
  const int m = weaken_inside ? n : weakening_free_run(n, i, steps2);
  return m < cap ? m : cap;
}

constexpr int kNoCap = INT_MAX;

struct Piece {
  unsigned first = 0;      // loop index of its first pass
  int m = 0;               // passes
  int at = 0;              // passes of the walk in front of it (first = i0 + at)
  bool weaken = false;     // WEAKEN_PRIORS in front of pass `first` is still to be run
};

// The walk over passes i0 .. i0 + n - 1.  front_done: the caller has run the weakening in front of pass i0 (if the loop has one there)
// already — the replay of a logged burst, the rest of a call whose launch did not run — so the first piece reports none.
// peek() shows the next piece under the cap and the rule a consumer can offer at this point; take() moves past it.  A consumer
// whose attempt at a piece did not run peeks again under another rule.
class PassWalk {
 public:
  PassWalk(int n, unsigned i0, unsigned steps2, bool front_done = false)
      : i_(i0), left_(n > 0 ? n : 0), at_(0), steps2_(steps2), front_done_(front_done) {}
  bool done() const { return left_ <= 0; }
  int left() const { return left_; }           // passes still to go
  unsigned index() const { return i_; }        // loop index of the next pass
  bool weakens() const { return !done() && !front_done_ && weakens_before(i_, steps2_); }      // in front of the next pass
  Piece peek(int cap, bool weaken_inside) const {
    Piece p;
    p.first = i_; p.at = at_; p.weaken = weakens();
    p.m = done() ? 0 : piece_passes(left_, i_, steps2_, weaken_inside, cap);
    return p;
  }
  void take(const Piece& p) {
    i_ += (unsigned)p.m; at_ += p.m; left_ -= p.m;
    if (p.m > 0) front_done_ = false;
  }
  Piece next(int cap, bool weaken_inside) {
    const Piece p = peek(cap, weaken_inside);
    take(p);
    return p;
  }

 private:
  unsigned i_;
  int left_, at_;
  unsigned steps2_;
  bool front_done_;
};

}  // namespace gbp
