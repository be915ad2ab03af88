// gbp_persist_seq.hpp — the numbering of a ctx's launches of the persistent kernel, as pure arithmetic (no HIP, no ctx: checked on its
// own under ASan + UBSan by tests/sanitize/persist_seq_main.cpp).
//
// Every launch gets a 32-bit number that keeps counting for the life of the ctx (no upload resets it).  Two things derive from it:
//   the word a time-out writes to the host-mapped status word, where 0 means "no launch failed" — so no launch may be numbered 0;
//   the tags of the launch's tagged records, tag0 + iteration + 1 with tag0 = (number mod 2^19) << 13 (an iteration count fits in the 13
//   bits: kPersistChunk <= 4096) — and tag 0 is what a record that nobody has written carries, so tag0 may not be 0 either.
// persist_next_seq therefore skips every number whose low 19 bits are zero: a TAG PERIOD is the 2^19 - 1 launches from one skipped
// number to the next, inside which no two launches share a tag.  Across periods they do, and a shadow that not every launch rewrites (the
// metric means: only launches that carry the metric; the second half of the landmark messages and row sums: only launches of two
// iterations or more) can keep a record of the period before under exactly the tag a launch of this period waits for.  So the launch
// that begins a period (persist_begins_period) is preceded by a clear of the shadows: no record older than one period survives it.
// Launch numbers are compared wrap-safe (persist_seq_before): those of one ctx that are alive together (the log of unvalidated launches)
// lie a handful apart.
#pragma once
#include <cstdint>

namespace gbp {

constexpr unsigned kPersistTagSeqBits = 19;                                  // launch numbers that a tag tells apart: 2^19 - 1 (0 is skipped)
constexpr unsigned kPersistTagSeqMask = (1u << kPersistTagSeqBits) - 1u;
constexpr unsigned kPersistTagIterBits = 32u - kPersistTagSeqBits;           // 13: tag0 + iteration + 1 stays inside the launch's 8192 tags

// the number of the launch behind launch `seq` (seq = 0: no launch yet).  Never a value whose low 19 bits are zero, so never 0.
inline unsigned persist_next_seq(unsigned seq) {
  unsigned n = seq + 1u;
  if ((n & kPersistTagSeqMask) == 0u) n += 1u;
  return n;
}
// the tag in front of the first tag of launch `seq` (its prologue's); never 0 for a number persist_next_seq handed out
inline unsigned persist_tag0(unsigned seq) { return (seq & kPersistTagSeqMask) << kPersistTagIterBits; }
// is `seq` the first launch of a tag period (of the ctx, or behind a skipped number)?  The shadows are cleared in front of it.
inline bool persist_begins_period(unsigned seq) { return (seq & kPersistTagSeqMask) == 1u; }
// launch a was made before launch b (numbers of one ctx less than 2^31 launches apart), across the wrap of the 32-bit number
inline bool persist_seq_before(unsigned a, unsigned b) { return (int32_t)(a - b) < 0; }

}  // namespace gbp
