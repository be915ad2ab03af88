// The numbering of the persistent kernel's launches (csrc/gbp_persist_seq.hpp) under ASan + UBSan, on its own: no launch is numbered 0,
// no tag0 is 0, no two launches of one tag period share a tag, a period's first launch is announced exactly once per period, and the
// order of two numbers survives the wrap of the 32-bit counter.  Built and run by tests/test_persist_seq_cpu.py; no device, no HIP.
#include "../../gbp_poplar_amd/csrc/gbp_persist_seq.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace gbp;

static int bad = 0;
static long checked = 0;
static unsigned g_seq;
#define CHECK(cond)                                                                                  \
  do {                                                                                               \
    ++checked;                                                                                       \
    if (!(cond)) {                                                                                   \
      if (++bad <= 20) std::fprintf(stderr, "line %d: %s  [seq %u]\n", __LINE__, #cond, g_seq);     \
    }                                                                                                \
  } while (0)

constexpr unsigned kPeriod = 1u << 19;
constexpr unsigned kMaxIters = 4096;      // kPersistChunk: tags tag0 .. tag0 + kMaxIters of a launch

// every property of one step seq -> next
static unsigned step(unsigned seq) {
  g_seq = seq;
  const unsigned n = persist_next_seq(seq);
  CHECK(n != 0u);
  CHECK((n & kPersistTagSeqMask) != 0u);
  CHECK(persist_tag0(n) != 0u);
  CHECK(n - seq == 1u || n - seq == 2u);                                   // it counts on, skipping at most one number
  CHECK((n - seq == 2u) == (((seq + 1u) & kPersistTagSeqMask) == 0u));      // ... exactly the numbers whose low 19 bits are zero
  CHECK(persist_seq_before(seq, n) && !persist_seq_before(n, seq) && !persist_seq_before(n, n));
  // a launch's 8192 tags do not reach into the next number's
  CHECK(persist_tag0(n) + kMaxIters + 1u > persist_tag0(n));
  CHECK((persist_tag0(n) >> kPersistTagIterBits) == (n & kPersistTagSeqMask));
  CHECK(((persist_tag0(n) + kMaxIters + 1u) >> kPersistTagIterBits) == (n & kPersistTagSeqMask));
  // the first launch of a period is the one behind a skipped number (or the ctx's first)
  CHECK(persist_begins_period(n) == (n - seq == 2u || (seq & kPersistTagSeqMask) == 0u));
  return n;
}

int main() {
  static_assert(kPersistTagSeqBits + kPersistTagIterBits == 32u, "a tag is 32 bits");
  static_assert((1u << kPersistTagIterBits) > kMaxIters + 1u, "tag0 + iteration + 1 stays inside the launch's tags");
  // round every multiple of 2^19 from 0 to 8 * 2^19, round 2^31 and round 2^32: 64 steps each
  std::vector<unsigned> starts;
  for (unsigned k = 0; k <= 8; ++k) starts.push_back(k * kPeriod - 32u);
  starts.push_back(0x80000000u - 32u);
  starts.push_back(0x80000000u + kPeriod - 32u);
  starts.push_back(0xffffffffu - 40u);
  starts.push_back(0u - kPeriod - 32u);
  for (unsigned s0 : starts) {
    unsigned s = s0;
    for (int i = 0; i < 64; ++i) s = step(s);
  }
  // literal values of the wraps
  g_seq = 0;
  CHECK(persist_next_seq(0u) == 1u);
  CHECK(persist_next_seq(kPeriod - 2u) == kPeriod - 1u);
  CHECK(persist_next_seq(kPeriod - 1u) == kPeriod + 1u);
  CHECK(persist_next_seq(kPeriod) == kPeriod + 1u);
  CHECK(persist_next_seq(0xfffffffeu) == 0xffffffffu);
  CHECK(persist_next_seq(0xffffffffu) == 1u);
  CHECK(persist_tag0(kPeriod - 1u) == 0xffffe000u && persist_tag0(kPeriod + 1u) == 0x2000u && persist_tag0(1u) == 0x2000u);
  CHECK(persist_seq_before(0xfffffffdu, 2u) && !persist_seq_before(2u, 0xfffffffdu));
  CHECK(persist_seq_before(0xffffffffu, 1u) && persist_seq_before(0x7ffffff0u, 0x80000010u));
  // two whole periods walked launch by launch, from in front of the 32-bit wrap: inside a period no tag0 twice (so no tag twice: the
  // launches' tag ranges are disjoint, checked above), a period is 2^19 - 1 launches, and its first launch is announced once
  {
    std::vector<unsigned char> seen(kPeriod, 0);
    unsigned s = 0u - kPeriod - 5u;
    long in_period = -1, periods = 0;
    for (long i = 0; i < 2L * kPeriod + 16; ++i) {
      s = persist_next_seq(s);
      g_seq = s;
      CHECK(s != 0u && persist_tag0(s) != 0u);
      if (persist_begins_period(s)) {
        if (in_period >= 0) { CHECK(in_period == (long)kPeriod - 1); ++periods; }
        in_period = 0;
        seen.assign(kPeriod, 0);
      }
      if (in_period >= 0) {
        const unsigned low = s & kPersistTagSeqMask;
        CHECK(!seen[low]);
        seen[low] = 1;
        ++in_period;
      }
    }
    CHECK(periods == 2);
  }
  if (bad) {
    std::fprintf(stderr, "persist_seq: %d of %ld checks failed\n", bad, checked);
    return 1;
  }
  std::printf("persist_seq: ok (%ld checks)\n", checked);
  return 0;
}
