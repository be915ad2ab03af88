// Where PassWalk (csrc/gbp_loop_plan.hpp) weakens, for triples given on the command line: `loop_plan_walk n i0 steps [n i0 steps ...]`
// prints one line per triple, the loop indices in front of which the walk reports a weakening — pieces that end in front of the next
// weakening, as every run of the two-kernel path consumes them, and pieces of the tagged-record kernel (interior weakenings counted by
// the predicate the kernel applies), which must agree.  tests/test_fuzz_plan_cpu.py compares the lines with the loop the soak's
// generator walks on the oracle.  No device, no HIP.
#include "../../gbp_poplar_amd/csrc/gbp_loop_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace gbp;

static std::vector<unsigned> weakenings(int n, unsigned i0, unsigned steps2, bool inside, int cap) {
  std::vector<unsigned> w;
  PassWalk walk(n, i0, steps2);
  while (!walk.done()) {
    const Piece p = walk.next(cap, inside);
    if (p.weaken) w.push_back(p.first);
    for (int k = 1; k < p.m; ++k)
      if (weakens_before(p.first + (unsigned)k, steps2)) w.push_back(p.first + (unsigned)k);      // only a piece with weaken_inside has any
  }
  return w;
}

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 1) % 3 != 0) {
    std::fprintf(stderr, "usage: loop_plan_walk n i0 steps [n i0 steps ...]\n");
    return 2;
  }
  for (int a = 1; a + 2 < argc; a += 3) {
    const int n = std::atoi(argv[a]);
    const unsigned i0 = (unsigned)std::strtoul(argv[a + 1], nullptr, 10), steps2 = 2u * (unsigned)std::strtoul(argv[a + 2], nullptr, 10);
    const std::vector<unsigned> w = weakenings(n, i0, steps2, false, kNoCap);
    if (w != weakenings(n, i0, steps2, true, 512) || w != weakenings(n, i0, steps2, false, 7)) {
      std::fprintf(stderr, "the consumers' rules disagree for n %d i0 %u steps2 %u\n", n, i0, steps2);
      return 1;
    }
    for (unsigned i : w) std::printf("%u ", i);
    std::printf("\n");
  }
  return 0;
}
