// gbp_api_eval.cpp — the metric on the device and the loops that carry it.
//   gbp_eval                      eval_reprojection_error (reference ba/util.cpp:74-144) + the counters of ba.cpp:1011-1020
//   gbp_ba_loop                   the BODY of the reference's iteration loop (ba.cpp:1001-1028, slam.cpp:1048-1103): prior weakening,
//                                 GBP_PROG, the metric — with the metric through iterate_passes_eval (one launch of the persistent
//                                 kernel per burst on small graphs, the metric riding in the sweeps (k_sweep<EV> / k_beliefs_ev)
//                                 elsewhere), without it through gbp_api_launch.cpp's iterate_passes
//   include/gbp_mi355x_compat.h   gbp_eval_begin / _end, gbp_iterate_eval, gbp_iterate_eval_each: earlier forms of the same loop
//                                 (gbp_iterate_eval_each = iterate_passes_eval with no weakening)
// gbp_eval, gbp_ba_loop and gbp_iterate_eval_each with an `out` in memory of the ctx's GPU (include/gbp_mi355x.h, "Device-resident arrays"):
// the same launches with their partial sums in device memory, folded on the device (k_eval_fold_part, k_eval_fold) into the caller's
// records; nothing waits — `dev` below.
#include "gbp_ctx.hpp"

#include <algorithm>

using namespace gbp;
using namespace gbp::api;

namespace gbp {
namespace api {

// eval_reprojection_error (util.cpp:74-144) + counters (ba.cpp:1011-1020) over the local shard
// The metric in two halves, so that a caller printing it every iteration (the reference's default loop) can queue the
// NEXT GBP iteration before it waits for the previous metric: begin enqueues k_means + k_eval, which write their result
// DIRECTLY into pinned, device-mapped host memory (slot 0 = the two health counters, slots 1..nb = per-block partials;
// no copy launch) and records an event; end waits for that event only and sums the partials in block order.  Two
// evaluations may be in flight (two result areas).  The health counters are accumulated with atomics in device memory,
// double-buffered so that no memset launch is needed: k_means zeroes the pair the next evaluation will use.
static int eval_alloc(gbp_ctx* c) {
  if (c->metric.area.host) return GBP_OK;
  if (int rc = mapped_alloc(c, c->metric.area, sizeof(DeviceEval) * 1025 * 2)) return rc;
  return event_pair_owned(c, &c->metric.ev[0], &c->metric.ev[1], hipEventDisableTiming);
}

// k_means + k_eval of the current beliefs into result area `area`, its event recorded behind them
int eval_enqueue(gbp_ctx* c, int area, DeviceEval* dev_slots) {
  DeviceEval* slots = dev_slots ? dev_slots : static_cast<DeviceEval*>(c->metric.area.dev) + 1025 * area;
  unsigned long long* h_cur = P<unsigned long long>(c->arr.health) + 2 * area;
  unsigned long long* h_next = P<unsigned long long>(c->arr.health) + 2 * (area ^ 1);
  launch_means(P<float4>(c->arr.camb), P<float4>(c->arr.lmkb), P<float>(c->arr.cam_mu), P<float>(c->arr.lmk_mu), c->C, c->L_loc,
               h_cur, h_next, /*count_cams=*/c->rank == 0, c->stream);
  launch_eval(P<uint32_t>(c->arr.row_cam), P<uint32_t>(c->arr.lmk_idx), P<int>(c->arr.fst_packed), P<float4>(c->arr.fac), P<float>(c->arr.cam_mu), P<float>(c->arr.lmk_mu),
              P<float>(c->arr.dK), c->prm.num_undamped_iters, slots + 1, h_cur, reinterpret_cast<unsigned long long*>(slots), c->n_tiles, c->stream);
  HIPCHK(c, hipGetLastError());
  if (dev_slots) return GBP_OK;
  HIPCHK(c, hipEventRecord(c->metric.ev[area], c->stream));
  c->metric.per_wave[area] = false;
  return GBP_OK;
}

// The two result areas (and their health words) take turns.  next_area: the one the next metric goes to; claim_area, once that metric
// is queued: the turn passes on, and (in_flight) the metric waits for a gbp_eval_end.
static int next_area(const gbp_ctx* c) { return c->metric.parity & 1; }
static void claim_area(gbp_ctx* c, bool in_flight) {
  c->metric.parity ^= 1;
  if (in_flight) c->metric.pending += 1;
}

// Is `out` of fn memory of the ctx's GPU?  Called after the argument and state checks of the call.  Host memory (unregistered, pinned,
// host-registered): *device = false, today's path.  GBP_ERR_INVALID naming `out`: another GPU's memory, managed memory, a landmark-sharded
// ctx (struct_kind), a device address that is not 8-byte aligned; GBP_ERR_STATE: the caller is capturing the ctx's stream.
static int out_kind(gbp_ctx* c, const char* fn, const void* out, bool* device) {
  const void* const members[1] = {out};
  const char* const names[1] = {"out"};
  if (int rc = struct_kind(c, fn, members, names, 1, device)) return rc;
  if (!*device) return GBP_OK;
  *device = false;
  if (reinterpret_cast<uintptr_t>(out) % 8 != 0)
    return fail(c, GBP_ERR_INVALID, std::string(fn) + ": out is device memory that is not 8-byte aligned (a record holds doubles and 64-bit counters)");
  if (stream_is_capturing(c))
    return fail(c, GBP_ERR_STATE, std::string(fn) + ": out is device memory and the ctx's stream is being captured: not supported");
  *device = true;
  return GBP_OK;
}

// the device twin of one result area of k_eval (first use allocates)
static int eval_scratch(gbp_ctx* c) {
  if (c->metric.scratch.p) return GBP_OK;
  return dev_alloc(c, c->metric.scratch, sizeof(DeviceEval) * 1025);
}

// One metric of the current beliefs into the caller's device record: k_means + k_eval as eval_begin queues them (the same health area,
// the parity advanced as one eval_begin / eval_end pair advances it), their partial sums in device memory, the fold behind them.
static int eval_to_device(gbp_ctx* c, gbp_eval_out* out) {
  const int area = next_area(c);
  if (int rc = eval_enqueue(c, area, P<DeviceEval>(c->metric.scratch))) return rc;
  claim_area(c, /*in_flight=*/false);
  launch_eval_fold_part(P<DeviceEval>(c->metric.scratch), 0, eval_blocks(c->n_tiles), c->n_tiles, false, 1, out, c->stream);
  HIPCHK(c, hipGetLastError());
  return GBP_OK;
}

int eval_begin(gbp_ctx* c) {
  if (!c || !c->uploaded) return fail(c, GBP_ERR_STATE, "gbp_eval: upload first");
  if (c->metric.pending >= 2) return fail(c, GBP_ERR_STATE, "gbp_eval_begin: two evaluations already in flight, call gbp_eval_end first");
  if (int rc = settle(c)) return rc;
  if (int rc = eval_alloc(c)) return rc;
  const int area = next_area(c);
  if (int rc = eval_enqueue(c, area)) return rc;
  claim_area(c, /*in_flight=*/true);
  return GBP_OK;
}

// part[0] = the two health counters; then one record per workgroup of k_eval (per_wave = false: nb of them), or one per tile
// wave of k_persist (per_wave = true: n_tiles of them) — the four waves of a workgroup added as k_eval's block reduction adds
// them, ((w0 + w1) + w2) + w3, then the workgroups in order: the same fp64 additions in the same order either way.
static int sum_eval(gbp_ctx* c, const DeviceEval* part, uint32_t nb, gbp_eval_out* o, bool per_wave) {
  std::memset(o, 0, sizeof(*o));
  if (per_wave) {
    for (uint32_t b = 0; b < nb; ++b) {
      DeviceEval w[4] = {};
      for (uint32_t k = 0; k < 4; ++k)
        if (b * 4 + k < c->n_tiles) w[k] = part[1 + b * 4 + k];
      o->sum_norm += ((w[0].sum_norm + w[1].sum_norm) + w[2].sum_norm) + w[3].sum_norm;
      o->sum_half_sq += ((w[0].sum_half_sq + w[1].sum_half_sq) + w[2].sum_half_sq) + w[3].sum_half_sq;
      for (uint32_t k = 0; k < 4; ++k) { o->n_active += w[k].n_active; o->n_relin += w[k].n_relin; o->n_robust += w[k].n_robust; }
    }
  } else {
    for (uint32_t b = 1; b <= nb; ++b) {
      o->sum_norm += part[b].sum_norm; o->sum_half_sq += part[b].sum_half_sq;
      o->n_active += part[b].n_active; o->n_relin += part[b].n_relin; o->n_robust += part[b].n_robust;
    }
  }
  // non-finite guard (replaces the Poplar FP traps of ba.cpp:888-891) + non-PD belief count;
  // cameras are replicated, so only rank 0 counts them
  unsigned long long h[2];
  std::memcpy(h, part, 16);
  o->n_nonfinite = h[0];
  o->n_nonpd = h[1];
  return GBP_OK;
}

int eval_end(gbp_ctx* c, gbp_eval_out* o) {
  if (!c || !o) return GBP_ERR_INVALID;
  if (c->metric.pending < 1) return fail(c, GBP_ERR_STATE, "gbp_eval_end: no evaluation in flight");
  std::memset(o, 0, sizeof(*o));
  const int area = (c->metric.parity + (c->metric.pending == 2 ? 0 : 1)) & 1;   // the OLDEST pending evaluation
  HIPCHK(c, hipEventSynchronize(c->metric.ev[area]));
  if (!c->persist.log.empty()) {
    // the metric may have come out of a k_persist launch: that launch (the oldest logged one for this area) and everything
    // before it have completed — validate them; after a time-out the recovery has re-queued the metric behind the replay
    unsigned upto = 0;
    for (const Burst& b : c->persist.log)
      if (b.kind == BurstKind::MetricAtEnd && b.area == area) { upto = b.seq; break; }
    const bool failed = persist_failed_seq(c) != 0u;
    if (failed || upto)
      if (int rc = persist_check(c, upto)) return rc;
    if (failed) HIPCHK(c, hipEventSynchronize(c->metric.ev[area]));
  }
  c->metric.pending -= 1;
  return sum_eval(c, static_cast<const DeviceEval*>(c->metric.area.host) + 1025 * area, eval_blocks(c->n_tiles), o, c->metric.per_wave[area]);
}

int eval(gbp_ctx* c, gbp_eval_out* o) {
  if (!c || !o || !c->uploaded) return fail(c, GBP_ERR_STATE, "gbp_eval: upload first");
  if (c->metric.pending) return fail(c, GBP_ERR_STATE, "gbp_eval: finish the evaluations in flight (gbp_eval_end) first");
  bool dev = false;
  if (int rc = out_kind(c, "gbp_eval", o, &dev)) return rc;
  if (dev) {      // not blocking (settle: k_means and k_eval are other device work than the launches it validates)
    if (int rc = settle(c)) return rc;
    if (int rc = eval_scratch(c)) return rc;
    return eval_to_device(c, o);
  }
  if (int rc = eval_begin(c)) return rc;
  return eval_end(c, o);
}

}  // namespace api
}  // namespace gbp

namespace {

// the riding metric's view of the ctx (gbp_kernels.h: EvalRide); valid once ev_alloc has run
EvalRide eval_ride(gbp_ctx* c) {
  EvalRide e{};
  e.cam_rec = P<float4>(c->metric.ev_cam); e.lmk_mean = P<float4>(c->metric.ev_lmk); e.part = P<EvalRec>(c->metric.ev_part);
  e.counter = P<unsigned>(c->metric.ev_ctl);
  e.health = reinterpret_cast<unsigned long long*>(static_cast<char*>(c->metric.ev_ctl.p) + 8);
  e.slot_health = reinterpret_cast<unsigned long long*>(static_cast<char*>(c->metric.ev_ctl.p) + 64);
  e.n_tiles = c->n_tiles; e.num_undamped = c->prm.num_undamped_iters;
  return e;
}

// The metric phases of a launch of the persistent kernel: one metric after its last iteration into result area `area`, or (each) one
// after EVERY iteration into the series slots — the host-mapped [kSeriesMax][n_tiles + 1] records persist_setup allocates.
static PersistEval persist_eval(gbp_ctx* c, int area, bool each) {
  PersistEval ev{};
  ev.on = 1;
  ev.cam_mu = P<float>(c->arr.cam_mu); ev.lmk_mu = P<float>(c->arr.lmk_mu);
  ev.num_undamped = c->prm.num_undamped_iters;
  if (each) {
    ev.each = 1;
    ev.stride = c->n_tiles + 1;          // [0] = health copy, then one record per tile wave
    ev.slots = static_cast<DeviceEval*>(c->persist.series.dev);
  } else {
    ev.slots = static_cast<DeviceEval*>(c->metric.area.dev) + 1025 * area;      // [0] = health copy, [1 + tile wave] = partial sums
  }
  ev.health = P<unsigned long long>(c->arr.health) + 2 * area;
  ev.health_next = P<unsigned long long>(c->arr.health) + 2 * (area ^ 1);
  ev.health_each = P<unsigned long long>(c->arr.health);
  return ev;
}

// gbp_iterate(n) followed by gbp_eval_begin() in one call.  On a graph that runs in k_persist the metric rides in the same
// launch (two more phases after the last belief update: what k_means and k_eval compute, bit for bit) — the reference's
// default loop prints the metric after EVERY iteration (ba.cpp:1009-1028), which otherwise costs four launches per iteration.
static int iterate_eval(gbp_ctx* c, int n) {
  if (!c || !c->uploaded) return fail(c, GBP_ERR_STATE, "gbp_iterate_eval: upload first");
  if (n <= 0) return eval_begin(c);
  bool fused = false;
  if (c->metric.pending < 2 && n <= kPersistChunk && c->n_tiles <= 1024)
    if (int rc = persist_ready(c, &fused)) return rc;
  if (fused) {
    if (int rc = eval_alloc(c)) return rc;
    const int area = next_area(c);
    const PersistEval metric = persist_eval(c, area, false);
    TimedSpan sp(c);
    if (int rc = sp.begin()) return rc;
    // A long burst with ONE metric at its end: all but the last iteration in the launch that carries no metric code at all (the
    // instantiation with the metric runs every iteration ~0.5 us slower: 59 us per 100 iterations on fr1xyz against ~10 us for
    // one more launch), the last iteration and the metric in a launch of their own.
    Burst head, tail;
    head.n = n >= 16 ? n - 1 : 0;
    tail.kind = BurstKind::MetricAtEnd; tail.n = n - head.n; tail.area = area;
    BurstOutcome ran = BurstOutcome::Ran;
    if (head.n)
      if (int rc = launch_persist_burst(c, sweep_args(c), head, nullptr, &ran)) return rc;
    if (ran == BurstOutcome::Ran) {      // (the head NotRun: nothing ran, everything on the two-kernel path below)
      if (int rc = launch_persist_burst(c, sweep_args(c), tail, &metric, &ran)) return rc;
      if (ran == BurstOutcome::Ran) {
        if (int rc = sp.commit((uint64_t)n)) return rc;
        HIPCHK(c, hipEventRecord(c->metric.ev[area], c->stream));
        c->metric.per_wave[area] = true;
        claim_area(c, /*in_flight=*/true);
        return GBP_OK;
      }
      if (head.n) {      // the head ran, the ctx then left the persistent path: the last iteration and the metric on the two-kernel path
        if (int rc = sp.commit((uint64_t)head.n)) return rc;
        if (int rc = iterate(c, tail.n)) return rc;
        return eval_begin(c);
      }
    }
  }
  if (int rc = iterate(c, n)) return rc;
  return eval_begin(c);
}

// gbp_iterate_eval_each on a graph that does not run in k_persist: the metric of iteration k rides in the sweep of iteration
// k + 1 (k_sweep<EV>, k_beliefs<EV>: EvalRide in gbp_kernels.h), the iterations replay from a hipGraph like gbp_iterate's (a ctx with a
// communicator: the sharded iteration with its belief update of two launches, launched directly — gbp_api_comm.cpp), the
// host is not involved until the burst has ended: per piece of at most ev_depth iterations (the ring of per-tile records) one
// k_eval_ride for the piece's last iteration and one k_eval_fold, which reduces every slot to one 56-byte result in host-mapped
// memory.  Bit-identical to gbp_iterate(1) + gbp_eval per iteration (same operations, same order of the sums).
static int ev_alloc(gbp_ctx* c) {
  if (c->metric.ev_depth) return GBP_OK;
  const size_t slot_bytes = (size_t)c->n_tiles * sizeof(EvalRec);
  const uint32_t depth = (uint32_t)std::min<size_t>(256, std::max<size_t>(2, ((size_t)128 << 20) / slot_bytes));      // <= 128 MB of ring
  if (int rc = dev_alloc(c, c->metric.ev_cam, (size_t)c->C * 3 * 16)) return rc;
  if (int rc = dev_alloc(c, c->metric.ev_lmk, (size_t)c->L_loc * 16)) return rc;
  if (int rc = dev_alloc(c, c->metric.ev_part, slot_bytes * depth)) return rc;
  if (int rc = dev_alloc(c, c->metric.ev_ctl, 64 + (size_t)depth * 16)) return rc;
  // (dev_alloc zero-fills on the ctx's stream, in front of the first burst that uses the ring: a fill on the NULL stream once raced
  // the first burst's records — a first metric over 3 062 of 200 000 factors — and a device-wide wait stalls every other stream of the process)
  c->metric.ev_depth = depth;
  return GBP_OK;
}
// dev: `out` is the caller's device memory — k_eval_fold writes there, nothing waits.  timed = false: the replay of a burst that gbp_timing has counted.
static int eval_each_ride(gbp_ctx* c, int n, gbp_eval_out* out, bool dev = false, bool timed = true) {
  if (int rc = settle(c)) return rc;
  if (int rc = ev_alloc(c)) return rc;
  if (!dev && sizeof(gbp_eval_out) * (size_t)n > c->metric.ev_results.bytes)       // one 56-byte result per iteration of the burst, host-mapped
    if (int rc = mapped_alloc(c, c->metric.ev_results, sizeof(gbp_eval_out) * std::max<size_t>(1024, (size_t)n))) return rc;
  static_assert(sizeof(gbp_eval_out) == 56, "k_eval_fold writes gbp_eval_out records");
  SweepArgs a = sweep_args(c);
  a.ev = eval_ride(c);
  TimedSpan sp(c);
  if (timed)
    if (int rc = sp.begin()) return rc;
  gbp_eval_out* const results = dev ? out : static_cast<gbp_eval_out*>(c->metric.ev_results.dev);
  for (int done = 0; done < n;) {         // pieces of at most ev_depth iterations, queued behind each other: no host wait in between
    const int m = std::min(n - done, (int)c->metric.ev_depth);
    HIPCHK(c, hipMemsetAsync(c->metric.ev_ctl.p, 0, 64, c->stream));      // iteration counter and health words of this piece
    if (int rc = c->xch.comm ? iterate_sharded_ev(c, a, m) : iterate_plain(c, a, m, true)) return rc;      // (a sharded ctx: launched directly, both schedules)
    launch_eval_ride(a.ev, P<uint32_t>(c->arr.row_cam), P<uint32_t>(c->arr.lmk_idx), P<int>(c->arr.fst_packed), P<float4>(c->arr.fac), P<float>(c->arr.dK), c->stream);
    launch_eval_fold(a.ev, (uint32_t)m, results + done, c->stream);
    HIPCHK(c, hipGetLastError());
    done += m;
  }
  if (timed)
    if (int rc = sp.commit((uint64_t)n)) return rc;
  if (dev) return GBP_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memcpy(out, c->metric.ev_results.host, sizeof(gbp_eval_out) * (size_t)n);
  return GBP_OK;
}

// m <= kSeriesMax passes from loop index i in ONE launch of the persistent kernel with the metric after every one of them (blocking):
// the metric of pass k rides in the sweep phase of pass k + 1 (both only read the beliefs), its partial sums go to host-mapped memory,
// out[k] = what gbp_iterate(1) + gbp_eval_global() would have returned.  *outcome = NotRun: nothing ran; TimedOut: the launch timed out and
// the state (priors and flags too) was restored to the start of the burst — either way the caller runs the passes on the two-kernel path.
static int series_burst(gbp_ctx* c, const Piece& p, unsigned steps2, gbp_eval_out* out, BurstOutcome* outcome) {
  Burst b = burst_of(BurstKind::SeriesHost, p, steps2);
  b.area = next_area(c);      // both health areas are zero between evaluations; this launch leaves them so
  const PersistEval metric = persist_eval(c, b.area, true);
  TimedSpan sp(c);
  if (int rc = sp.begin()) return rc;
  if (int rc = launch_persist_burst(c, sweep_args(c), b, &metric, outcome)) return rc;
  if (*outcome != BurstOutcome::Ran) return GBP_OK;
  if (int rc = sp.end()) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const bool failed = persist_failed_seq(c) != 0u;
  if (int rc = persist_check(c, 0)) return rc;
  if (failed) { *outcome = BurstOutcome::TimedOut; return GBP_OK; }
  if (int rc = sp.commit((uint64_t)p.m)) return rc;
  for (int k = 0; k < p.m; ++k)
    sum_eval(c, static_cast<const DeviceEval*>(c->persist.series.host) + (size_t)k * metric.stride, eval_blocks(c->n_tiles), out + k, true);
  return GBP_OK;
}

// The same launch for a caller whose records live on the GPU, not blocking: the per-pass records go to a device-memory twin of the series
// slots, one workgroup of k_eval_fold_part per pass folds them into out[k] behind the launch (and in front of the next launch, which
// reuses the twin), and the launch stays in the log of unvalidated launches with what a replay needs — whoever validates it later
// (settle / persist_check) and finds that it timed out restores the snapshot and replays it on the riding path into the same records
// (persist_recover: BurstKind::SeriesDevice).  The only host-mapped word involved is the status word of the kernel.
static int series_burst_dev(gbp_ctx* c, const Piece& p, unsigned steps2, gbp_eval_out* out, BurstOutcome* outcome) {
  if (!c->metric.series_twin.p)
    if (int rc = dev_alloc(c, c->metric.series_twin, sizeof(DeviceEval) * (size_t)(c->n_tiles + 1) * kSeriesMax)) return rc;
  Burst b = burst_of(BurstKind::SeriesDevice, p, steps2);
  b.area = next_area(c); b.out = out;
  PersistEval metric = persist_eval(c, b.area, true);
  metric.slots = P<DeviceEval>(c->metric.series_twin);
  TimedSpan sp(c);
  if (int rc = sp.begin()) return rc;
  if (int rc = launch_persist_burst(c, sweep_args(c), b, &metric, outcome)) return rc;
  if (*outcome != BurstOutcome::Ran) return GBP_OK;
  launch_eval_fold_part(metric.slots, metric.stride, eval_blocks(c->n_tiles), c->n_tiles, true, (uint32_t)p.m, out, c->stream);
  HIPCHK(c, hipGetLastError());
  return sp.commit((uint64_t)p.m);
}

// per_factor_mu = 1, per-stage timing, a ctx with a communicator whose metric does not ride: the loop the riding path replaces, with device records — per pass
// gbp_iterate(1), k_means + k_eval into the device scratch, its fold (stream order keeps the scratch until its fold has read it)
static int eval_each_plain_dev(gbp_ctx* c, int m, gbp_eval_out* out) {
  if (int rc = eval_scratch(c)) return rc;
  for (int k = 0; k < m; ++k) {
    if (int rc = iterate(c, 1)) return rc;
    if (int rc = eval_to_device(c, out + k)) return rc;
  }
  return GBP_OK;
}

}  // namespace

// The driver of passes WITH the metric after every one of them (gbp_iterate_eval_each: i0 = steps2 = 0; gbp_ba_loop), blocking:
// passes i0 .. i0 + n - 1 of the reference's loop (ba.cpp:1001-1028), WEAKEN_PRIORS in front of pass i iff weakens_before(i, steps2),
// GBP_PROG, the metric.  On a graph that runs in the persistent kernel the passes are launches of at most kSeriesMax (PassWalk):
// k_persist_flow applies WeakenPriorVertex itself in front of its later passes, only a weakening in front of a launch's first pass is
// a launch of its own.  Everywhere else — and after a recovered time-out — each run of passes up to the next weakening carries the
// metric in its sweeps (eval_each_ride; a ctx with a communicator: where metric_rides says so, gbp_transport.hpp), or is the loop it
// replaces, two metrics in flight.
// dev: out[] is memory of the ctx's GPU and nothing here blocks — launches of the persistent kernel queue behind the unvalidated ones
// as gbp_iterate's do (persist_ready), the other paths wait for those first (settle) as every other kind of device work does.
// replay: persist_recover, for a SeriesDevice launch that timed out — the state is the one the launch started from, the weakening in
// front of its first pass included; the ctx has left the persistent path and rides (it ran there: hoisted, one GPU, no communicator),
// whatever the caller has set since; gbp_timing has counted the passes.
int gbp::api::iterate_passes_eval(gbp_ctx* c, int n, unsigned i0, unsigned steps2, gbp_eval_out* out, bool dev, bool replay) {
  for (PassWalk w(n, i0, steps2, /*front_done=*/replay); !w.done();) {
    if (w.weakens())
      if (int rc = weaken_priors(c)) return rc;
    if (!dev)
      if (int rc = settle(c)) return rc;
    bool fused = false;
    if (eval_blocks(c->n_tiles) == (c->n_tiles + 3) / 4)
      if (int rc = persist_ready(c, &fused)) return rc;
    if (fused) {
      const Piece p = w.peek((int)kSeriesMax, persist_tagged(c));
      BurstOutcome ran;
      if (int rc = dev ? series_burst_dev(c, p, steps2, out + p.at, &ran) : series_burst(c, p, steps2, out + p.at, &ran)) return rc;
      if (ran == BurstOutcome::Ran) { w.take(p); continue; }
    }
    if (dev)
      if (int rc = settle(c)) return rc;
    const Piece p = w.next(kNoCap, /*weaken_inside=*/false);
    bool ride = replay || (c->hoist && plain_single_gpu(c));
    if (c->xch.comm) {      // a ctx with a communicator: the decision and its record (gbp_comm_describe: "metric")
      ride = metric_rides(c->xch.comm->kind(), c->world, c->hoist, c->tm.profile_stages, stream_is_capturing(c), &c->xch.metric_reason);
      c->xch.metric_last = ride ? 1 : 2;
      (ride ? c->xch.metric_riding : c->xch.metric_per_pass) += (uint64_t)p.m;
    }
    if (ride) {
      if (int rc = eval_each_ride(c, p.m, out + p.at, dev, /*timed=*/!replay)) return rc;
    } else if (dev) {
      if (int rc = eval_each_plain_dev(c, p.m, out + p.at)) return rc;
    } else {
      int collected = p.at;
      for (int k = 0; k < p.m; ++k) {
        if (int rc = iterate(c, 1)) return rc;
        if (int rc = eval_begin(c)) return rc;
        if (c->metric.pending == 2) { if (int rc = eval_end(c, out + collected)) return rc; ++collected; }
      }
      while (collected < p.at + p.m) { if (int rc = eval_end(c, out + collected)) return rc; ++collected; }
    }
  }
  return GBP_OK;
}

static int iterate_eval_each(gbp_ctx* c, int n, gbp_eval_out* out) {
  if (!c || !c->uploaded) return fail(c, GBP_ERR_STATE, "gbp_iterate_eval_each: upload first");
  if (n < 0 || (n > 0 && !out)) return fail(c, GBP_ERR_INVALID, "gbp_iterate_eval_each: n >= 0 and an array of n results");
  if (c->metric.pending) return fail(c, GBP_ERR_STATE, "gbp_iterate_eval_each: finish the evaluations in flight (gbp_eval_end) first");
  bool dev = false;
  if (out)
    if (int rc = out_kind(c, "gbp_iterate_eval_each", out, &dev)) return rc;
  if (dev) return iterate_passes_eval(c, n, 0, 0, out, true);
  if (int rc = settle(c)) return rc;                  // blocking call: nothing of this ctx stays in flight across it
  return iterate_passes_eval(c, n, 0, 0, out);
}

// n passes of the body of the reference's iteration loop (ba.cpp:1001-1028) from loop index iter0.  Without the metric (out == NULL)
// not blocking, like gbp_iterate: ONE iterate_passes call — the weakening in front of a launch of the persistent kernel a launch of its
// own, every other one riding in such a launch or in the belief update of the iteration before it.
// A sharded ctx, per-stage timing and a caller's capture keep gbp_iterate's own paths: one call per run of passes up to the next weakening.
static int ba_loop(gbp_ctx* c, int n, unsigned iter0, unsigned steps, gbp_eval_out* out) {
  if (!c || !c->uploaded) return fail(c, GBP_ERR_STATE, "gbp_ba_loop: upload first");
  if (n < 0) return fail(c, GBP_ERR_INVALID, "gbp_ba_loop: n >= 0");
  if (steps >= (1u << 30)) return fail(c, GBP_ERR_INVALID, "gbp_ba_loop: steps < 2^30 (the loop's test is iter < 2 * steps)");
  const unsigned steps2 = 2u * steps;
  if (out) {
    if (c->metric.pending) return fail(c, GBP_ERR_STATE, "gbp_ba_loop: finish the evaluations in flight (gbp_eval_end) first");
    bool dev = false;
    if (int rc = out_kind(c, "gbp_ba_loop", out, &dev)) return rc;
    return iterate_passes_eval(c, n, iter0, steps2, out, dev);
  }
  if (plain_single_gpu(c)) return n ? iterate_passes(c, n, iter0, steps2) : GBP_OK;
  for (PassWalk w(n, iter0, steps2); !w.done();) {
    if (w.weakens())
      if (int rc = weaken_priors(c)) return rc;
    if (int rc = iterate(c, w.next(kNoCap, /*weaken_inside=*/false).m)) return rc;
  }
  return GBP_OK;
}

GBP_EXPORT(gbp_eval, c, (gbp_ctx* c, gbp_eval_out* o), (c, o)) { return eval(c, o); }
GBP_EXPORT(gbp_eval_begin, c, (gbp_ctx* c), (c)) { return eval_begin(c); }
GBP_EXPORT(gbp_eval_end, c, (gbp_ctx* c, gbp_eval_out* o), (c, o)) { return eval_end(c, o); }
GBP_EXPORT(gbp_iterate_eval, c, (gbp_ctx* c, int n), (c, n)) { return iterate_eval(c, n); }
GBP_EXPORT(gbp_iterate_eval_each, c, (gbp_ctx* c, int n, gbp_eval_out* out), (c, n, out)) { return iterate_eval_each(c, n, out); }
GBP_EXPORT(gbp_ba_loop, c, (gbp_ctx* c, int n, unsigned iter0, unsigned steps, gbp_eval_out* out), (c, n, iter0, steps, out)) {
  return ba_loop(c, n, iter0, steps, out);
}
