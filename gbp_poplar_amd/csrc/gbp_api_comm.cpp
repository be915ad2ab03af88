// gbp_api_comm.cpp — the landmark-sharded ctx (include/gbp_mi355x_multi.h): communicator glue, the sharded iteration and
// gbp_eval_global.  Replaces `--ipus N` (reference ba/ba.cpp:414-417,617-649: Poplar compiles the inter-IPU exchange into the
// program): one process per GPU, each rank owns a landmark range and every factor incident to it; per iteration ONE all-gather of
// the [C x 44] camera partial sums (csrc/gbp_comm.*: RCCL over xGMI, or the host-staged transport when ranks share a GPU), every
// rank then adds prior + partials in rank order — bit-identical camera beliefs on all ranks.
#include "gbp_ctx.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace gbp;
using namespace gbp::api;

namespace gbp {
namespace api {

// A peer-memory transport exchanges through the communicator's own buffer: send_dev / recv_dev are this rank's slot / the whole
// [world][C][44] of the NEXT exchange (re-bound after every exchange).  No-op for the other transports.
static void bind_exchange(gbp_ctx* c) {
  if (PeerComm* pc = peers(c->xch.comm)) {
    c->xch.send_dev = pc->send_slot();
    c->xch.recv_dev = pc->next_block();
  }
}

// plain exchange on the ctx's stream (LINEARISE, refreshes) or on s: partials in send_dev -> recv_dev of every rank
int exchange_now(gbp_ctx* c, hipStream_t s) {
  COMMCHK(c, c->xch.comm->all_gather(static_cast<const float*>(c->xch.send_dev), static_cast<float*>(c->xch.recv_dev),
                                 (size_t)c->C * kCamRec, s ? s : c->stream, e_));
  bind_exchange(c);
  return GBP_OK;
}

// the exchange without a copy: stream sync + ONE region barrier; *p = the parity it closed, whose slots the readers behind it take in place
static int advance_exchange(gbp_ctx* c, PeerComm* pc, int* p) {
  COMMCHK(c, pc->advance(c->stream, p, e_));
  bind_exchange(c);
  return GBP_OK;
}

// a new problem (gbp_upload): what the exchange gathers into starts from zero
int zero_exchange(gbp_ctx* c) {
  if (PeerComm* pc = peers(c->xch.comm)) HIPCHK(c, pc->zero(c->stream));
  else if (exch(c) && c->xch.recv_dev) HIPCHK(c, hipMemsetAsync(c->xch.recv_dev, 0, (size_t)c->world * c->C * kCamRec * 4, c->stream));
  return GBP_OK;
}

// ---- who combines the cameras ----------------------------------------------------------------------------------------------------
// | transport                  | in the iteration (single stream, behind the partial_only launch)                                 | prior-only refresh (refresh_beliefs_from_partials)                                |
// | RCCL, host-staged          | all_gather into recv_dev, then launch_beliefs(b, true, false) with gathered = recv_dev            | launch_beliefs(b, true, do_lmk) with gathered = recv_dev                           |
// | p2p                        | advance, then launch_beliefs_cam_peers(b, table of that parity)                                   | launch_beliefs_cam_peers(b, last table), then launch_beliefs(b, false, true) if do_lmk |
// | p2p-slices, world > 1      | advance (barrier A); launch_beliefs_cam_slice; stream sync; barrier (B); launch_gather_slices     | as p2p                                                                             |
// | p2p-slices, world = 1      | advance, then launch_beliefs(b, true, false) with gathered = own slot of that parity              | launch_beliefs(b, true, do_lmk) with gathered = own slot of the last parity        |
// | no communicator, world > 1 | not this path (caller's exchange)                                                                 | gathered = recv_dev; error "exchange buffers not set" without one                  |
// | no communicator, world = 1 | not this path                                                                                     | gathered = local, b.world = 1                                                      |
// Return codes by cause: GBP_ERR_HIP (a launch, a synchronisation), GBP_ERR_COMM (the exchange).

// the iteration's column: the exchange and the camera combine on the ctx's stream; x1 (profiling): recorded behind the all-gather.
// roll = 1: the end of an iteration; 0: the same launches as a recomputation of what the ctx holds (the measured transport's rounds)
// ev: the iteration carries the metric — the combine is the iteration's LAST belief launch: it leaves the cameras' metric records and
// advances the burst's counter (gbp_kernels.h: BeliefArgs.ev_split).  Never with roll = 0, never on the sliced transport with world > 1.
static void ride_args(gbp_ctx* c, BeliefArgs& b, const EvalRide* ev, bool last) {
  if (!ev) return;
  b.ev = *ev;
  b.ev_split = (last ? 0 : kEvNotLast) | (c->rank == 0 ? 0 : kEvNoCamHealth);
}
static int combine_cameras_in_iteration(gbp_ctx* c, hipEvent_t x1, int roll, const EvalRide* ev) {
  BeliefArgs b = belief_args(c);
  b.roll = roll;
  ride_args(c, b, ev, true);
  PeerComm* pc = peers(c->xch.comm);
  int p = 0;
  switch (c->xch.comm->kind()) {
    case Transport::P2p:
      if (int rc = advance_exchange(c, pc, &p)) return rc;
      launch_beliefs_cam_peers(b, pc->peer_table(p), c->stream, ev != nullptr);
      break;
    case Transport::P2pSlices:
      if (c->world == 1) {      // nothing to share: no peer kernel
        if (int rc = advance_exchange(c, pc, &p)) return rc;
        b.gathered = pc->last_own_slot();
        launch_beliefs(b, true, false, c->stream, ev != nullptr);
        break;
      }
      if (ev) return fail(c, GBP_ERR_STATE, "the sliced exchange carries no metric records");      // (metric_rides keeps such a ctx per-pass)
      // the reduce of this rank's slice of the cameras (sums in rank order out of every peer's partials, the camera chain, once per
      // camera), then the gather of the other slices' finished records — every rank ends with the tables the full combine leaves
      if (int rc = advance_exchange(c, pc, &p)) return rc;
      CamSlice sl;
      slice_bounds(c->C, c->world, c->rank, &sl.lo, &sl.hi);
      sl.res = pc->result_buffer(p);
      launch_beliefs_cam_slice(b, pc->peer_table(p), sl, c->stream);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipStreamSynchronize(c->stream));
      COMMCHK(c, c->xch.comm->barrier(e_));
      launch_gather_slices(pc->result_table(p), b, c->rank, c->stream);
      break;
    default:
      if (int rc = exchange_now(c)) return rc;
      if (x1) HIPCHK(c, hipEventRecord(x1, c->stream));
      b.gathered = static_cast<const float*>(c->xch.recv_dev);
      launch_beliefs(b, true, false, c->stream, ev != nullptr);
      break;
  }
  HIPCHK(c, hipGetLastError());
  return GBP_OK;
}

// the refresh's column: b as the caller set it up (roll, weaken)
int refresh_cameras(gbp_ctx* c, BeliefArgs& b, bool do_lmk) {
  PeerComm* pc = peers(c->xch.comm);
  const Transport kind = c->xch.comm ? c->xch.comm->kind() : Transport::Auto;      // (Auto: no communicator)
  if (kind == Transport::P2p || (kind == Transport::P2pSlices && c->world > 1)) {
    // the last exchange's partials are read where they lie; the landmark half, which needs nothing from other ranks, in a launch of its own
    launch_beliefs_cam_peers(b, pc->last_table(), c->stream);
    if (do_lmk) launch_beliefs(b, false, true, c->stream);
  } else {
    if (kind == Transport::P2pSlices) {
      b.gathered = pc->last_own_slot();      // (recv_dev is the parity of the NEXT exchange)
    } else if (!exch(c)) {
      b.gathered = P<float>(c->arr.local); b.world = 1;
    } else {
      if (!c->xch.recv_dev) return fail(c, GBP_ERR_STATE, "exchange buffers not set");
      b.gathered = static_cast<const float*>(c->xch.recv_dev);
    }
    launch_beliefs(b, true, do_lmk, c->stream);
  }
  HIPCHK(c, hipGetLastError());
  return GBP_OK;
}

// The two-stream schedule (RCCL): the communication stream (highest priority) takes the whole camera side of the exchange — local
// partial sums, then the all-gather — right after the sweep; the landmark half of the belief update, which needs nothing from other
// ranks, runs beside it on the main stream.  x0 / x1 (profiling): a bracket around the camera side on its stream.
// ev: the landmark half leaves its metric means and health counts, the combine behind the join is the iteration's last belief launch.
static int enqueue_cameras_two_streams(gbp_ctx* c, hipEvent_t x0, hipEvent_t x1, int roll = 1, const EvalRide* ev = nullptr) {
  HIPCHK(c, hipEventRecord(c->xch.ev_fork, c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->xch.stream, c->xch.ev_fork, 0));
  if (x0) HIPCHK(c, hipEventRecord(x0, c->xch.stream));
  enqueue_cam_partials(c, static_cast<float*>(c->xch.send_dev), c->xch.stream);
  if (int rc = exchange_now(c, c->xch.stream)) return rc;
  if (x1) HIPCHK(c, hipEventRecord(x1, c->xch.stream));
  HIPCHK(c, hipEventRecord(c->xch.ev_join, c->xch.stream));
  BeliefArgs b = belief_args(c);
  b.roll = roll;
  ride_args(c, b, ev, false);
  launch_beliefs(b, false, true, c->stream, ev != nullptr);
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->xch.ev_join, 0));
  b.gathered = static_cast<const float*>(c->xch.recv_dev);
  ride_args(c, b, ev, true);
  launch_beliefs(b, true, false, c->stream, ev != nullptr);
  HIPCHK(c, hipGetLastError());
  return GBP_OK;
}

// ONE stream: the local camera partial sums ride in the launch of the landmark half (camera blocks write send_dev and leave,
// landmark blocks do the rank-local belief update), so an iteration is sweep -> beliefs -> exchange -> combine: three kernels and
// one collective.  Still no host wait with a stream-ordered transport.
// ev: the partial_only launch carries the landmarks' share of the metric (its camera blocks none), the combine the cameras'.
static int enqueue_cameras_one_stream(gbp_ctx* c, hipEvent_t x0, hipEvent_t x1, int roll = 1, const EvalRide* ev = nullptr) {
  BeliefArgs b = belief_args(c);
  b.cam_local = static_cast<float*>(c->xch.send_dev);
  b.partial_only = 1;
  b.roll = roll;
  ride_args(c, b, ev, false);
  launch_beliefs(b, true, true, c->stream, ev != nullptr);
  if (x0) HIPCHK(c, hipEventRecord(x0, c->stream));
  return combine_cameras_in_iteration(c, x1, roll, ev);
}

// One iteration of a sharded ctx: sweep, then the camera side of the exchange and the belief update in one of the two schedules.
// With a stream-ordered transport (RCCL) nothing here blocks the host, so the sequence can be captured into a hipGraph.
// ev: the iteration carries the metric (a.ev set by the caller: eval_each_ride) — the sweep collects the metric of the iteration before
// it, the belief launches leave this one's metric records.  Such iterations are launched directly, never from the captured graph (graph.sharded).
static int enqueue_sharded_iteration(gbp_ctx* c, const SweepArgs& a, bool ev = false) {
  if (c->tm.profile_stages) {
    if (c->tm.pending_sweep_ev.size() >= 256) drain_sweep_events(c);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (int rc = event_pair(c, &e0, &e1)) return rc;
    c->tm.pending_sweep_ev.push_back({e0, e1});
    HIPCHK(c, hipEventRecord(e0, c->stream));
    launch_sweep(a, c->n_tiles, c->hoist, c->stream, ev);
    HIPCHK(c, hipEventRecord(e1, c->stream));
  } else {
    launch_sweep(a, c->n_tiles, c->hoist, c->stream, ev);
  }
  hipEvent_t x0 = nullptr, x1 = nullptr;     // profiling: how long the camera side of the exchange takes on its stream
  if (c->tm.profile_stages && c->xch.comm->stream_ordered()) {
    if (int rc = event_pair(c, &x0, &x1)) return rc;
    c->tm.pending_exch_ev.push_back({x0, x1});
  }
  const EvalRide* r = ev ? &a.ev : nullptr;
  return c->xch.comm->stream_ordered() && !c->xch.single_stream ? enqueue_cameras_two_streams(c, x0, x1, 1, r) : enqueue_cameras_one_stream(c, x0, x1, 1, r);
}

// n sharded iterations that carry the metric, inside a piece of eval_each_ride (which owns the ring, the counter and the timing bracket)
int iterate_sharded_ev(gbp_ctx* c, const SweepArgs& a, int n) {
  for (int k = 0; k < n; ++k) {
    if (int rc = enqueue_sharded_iteration(c, a, true)) return rc;
    c->xch.warm++;
  }
  return GBP_OK;
}

int iterate_sharded(gbp_ctx* c, int n) {
  const SweepArgs a = sweep_args(c);
  TimedSpan sp(c);
  if (int rc = sp.begin()) return rc;
  int left = n;
  // Measured (config-5 shard shape, 1-rank communicator): direct launches 0.186 ms per iteration, the captured graph with
  // its cross-stream fork/join nodes 0.191 ms — the path is not host-bound, so the graph is opt-in (graph_unroll > 0).
  const bool can_graph = c->xch.comm->stream_ordered() && !c->tm.profile_stages && c->graph.sharded && !c->graph.failed &&
                         c->stream == c->own_stream;
  // RCCL sets itself up lazily (channels, proxy threads): a few direct iterations must have run before a capture
  while (left > 0 && (!can_graph || c->xch.warm < 3 || left < c->prm.graph_unroll)) {
    if (int rc = enqueue_sharded_iteration(c, a)) return rc;
    c->xch.warm++;
    --left;
  }
  if (left >= c->prm.graph_unroll && can_graph) {
    if (!c->graph.exec) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed);
      int rc = GBP_OK;
      if (e == hipSuccess) {
        for (int i = 0; i < c->prm.graph_unroll && rc == GBP_OK; ++i) rc = enqueue_sharded_iteration(c, a);
        e = hipStreamEndCapture(c->stream, &c->graph.g);
        if (e == hipSuccess && rc == GBP_OK) e = hipGraphInstantiate(&c->graph.exec, c->graph.g, nullptr, nullptr, 0);
      }
      if (e != hipSuccess || rc != GBP_OK) {     // no graph for this ctx: direct launches (identical results)
        (void)hipGetLastError();
        drop_graph(c);
        c->graph.failed = true;
      } else {
        c->graph.iters = c->prm.graph_unroll;
      }
    }
    while (c->graph.exec && left >= c->graph.iters) {
      HIPCHK(c, hipGraphLaunch(c->graph.exec, c->stream));
      left -= c->graph.iters;
    }
  }
  for (; left > 0; --left)
    if (int rc = enqueue_sharded_iteration(c, a)) return rc;
  if (int rc = sp.end()) return rc;
  if (!c->xch.comm->stream_ordered() || c->tm.profile_stages) HIPCHK(c, hipStreamSynchronize(c->stream));
  return sp.commit(c->tm.profile_stages ? 0 : (uint64_t)n);    // with profiling the sweep brackets count the iterations
}

}  // namespace api
}  // namespace gbp

// ---- communicator: the exchange step owned by the library (RCCL over xGMI from the C++ host) ------------------------
// the second stream of the two-stream schedule, made when first needed.  Highest priority: the all-gather is issued while the
// landmark half of k_beliefs fills the GPU; it must not queue behind those blocks (the camera combine of every rank waits for it)
static int ensure_comm_stream(gbp_ctx* c) {
  if (c->xch.stream || c->xch.single_stream) return GBP_OK;
  int least = 0, greatest = 0;
  HIPCHK(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
  HIPCHK(c, hipStreamCreateWithPriority(&c->xch.stream, hipStreamNonBlocking, greatest));
  return GBP_OK;
}

static int comm_attach(gbp_ctx* c, gbp::Comm* comm) {
  if (int rc = settle(c)) { delete comm; return rc; }
  c->xch.comm = comm;
  // A second HSA queue makes every dispatch of the main queue slower (measured: +10 us per sharded iteration on the
  // config-5 shard shape, 0.183 vs 0.174 ms with a 1-rank communicator), so overlapping the all-gather with the
  // landmark beliefs (~20 us of cover) only pays once the all-gather itself takes longer than that: 4 ranks and more.
  // GBP_COMM_SINGLE_STREAM=0/1 overrides the rule (measurements).
  const char* ss = std::getenv("GBP_COMM_SINGLE_STREAM");
  c->xch.single_stream = ss ? ss[0] == '1' : c->world <= 2;
  drop_graph(c);
  // IN-PLACE all-gather: this rank's partial sums are written straight into its own slot of the gathered buffer
  // (sendbuff == recvbuff + rank * count is the in-place form of ncclAllGather: the collective then moves only what comes from
  // other ranks — with a 1-rank communicator nothing at all, where the out-of-place form was a 5 us copy kernel per iteration,
  // profiles/r06_sharded_timeline.md).  (zero-filled on the ctx's stream, in front of everything that uses it)
  bind_exchange(c);      // p2p: the communicator's own buffer
  if (!peers(comm)) {
    if (!c->xch.xrecv.p)
      if (int rc = dev_alloc(c, c->xch.xrecv, (size_t)c->world * c->C * kCamRec * 4)) return rc;
    c->xch.recv_dev = c->xch.xrecv.p;
    c->xch.send_dev = static_cast<float*>(c->xch.xrecv.p) + (size_t)c->rank * c->C * kCamRec;
  }
  c->xch.metric_last = 0; c->xch.metric_riding = c->xch.metric_per_pass = 0; c->xch.metric_reason = "";
  if (int rc = ensure_comm_stream(c)) return rc;
  if (!c->xch.ev_fork)
    if (int rc = event_create(c, &c->xch.ev_fork, hipEventDisableTiming)) return rc;
  if (!c->xch.ev_join)
    if (int rc = event_create(c, &c->xch.ev_join, hipEventDisableTiming)) return rc;
  c->xch.warm = 0;
  return GBP_OK;
}

GBP_EXPORT_T(int, 0, gbp_device_count, (void), ()) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

GBP_EXPORT(gbp_set_device, nullptr, (int device), (device)) {
  if (hipSetDevice(device) != hipSuccess) return fail(nullptr, GBP_ERR_NO_DEVICE, "gbp_set_device: no such device");
  return GBP_OK;
}

GBP_EXPORT_T(size_t, 0, gbp_comm_region_bytes, (uint32_t n_cams, int world), (n_cams, world)) {
  if (world < 1 || world > gbp::kCommMaxWorld) return 0;      // (gbp_comm_region_init refuses such a world as well)
  return gbp::comm_region_bytes(n_cams, world);
}

GBP_EXPORT(gbp_comm_region_init, nullptr, (void* region, size_t bytes, uint32_t n_cams, int world), (region, bytes, n_cams, world)) {
  if (!region) return GBP_ERR_INVALID;
  return gbp::comm_region_init(region, bytes, n_cams, world) == 0 ? GBP_OK : GBP_ERR_INVALID;
}

GBP_EXPORT_VOID(gbp_comm_region_abort, (void* region), (region)) { if (region) gbp::comm_region_abort(region); }

GBP_EXPORT(gbp_comm_region_selftest, nullptr, (void* region, int rank, int world, int rounds), (region, rank, world, rounds)) {
  if (!region || world < 1 || rank < 0 || rank >= world) return GBP_ERR_INVALID;
  std::string err;
  const int rc = gbp::comm_region_selftest(region, rank, world, rounds, err);
  if (rc != 0) return fail(nullptr, GBP_ERR_COMM, "gbp_comm_region_selftest: " + err);
  return GBP_OK;
}

// ---- transport 5: the exchange chosen by measurement -------------------------------------------------------------------------------
// Which transport is fastest depends on the machine (ranks sharing a GPU, PCIe or xGMI between them, how many processes the device
// schedules), and the rules of transport 0 were written without one to measure on.  gbp_comm_init(ctx, region, 5) therefore forms, one
// after the other, every communicator this group of ranks CAN form (eligible_candidates, from facts published before any exists: a
// creation that fails raises the region's abort flag for good), attaches each to the ctx as comm_attach does and times what differs
// between them — the camera side of the sharded iteration (local partials, exchange, combine, the landmark half beside them) — with
// roll = 0: the launches recompute, from the same row sums, messages and priors, the tables the ctx already holds, as a prior-only
// refresh does.  What transport 0 would have attached (the baseline) is timed first and last; choose_transport (gbp_transport.hpp)
// decides from the table every rank has gathered.  Collective; every rank leaves with the same transport and schedule.
namespace {

constexpr int kMeasureWarmup = 3;      // untimed rounds (RCCL sets its channels up lazily; iterate_sharded waits for as many)
constexpr int kMeasureReps = 10;       // timed rounds
constexpr int kMeasureCappedReps = 2;  // ... of a candidate whose warm-up alone outlasted the baseline's whole first measurement

using clk = std::chrono::steady_clock;
inline double us_since(clk::time_point t0) { return std::chrono::duration<double, std::micro>(clk::now() - t0).count(); }

// n rounds back to back; *us = wall clock from the first enqueue until the ctx's stream has drained (what a rank waits for)
int time_rounds(gbp_ctx* c, bool two_streams, int n, double* us) {
  const auto t0 = clk::now();
  for (int i = 0; i < n; ++i)
    if (int rc = two_streams ? enqueue_cameras_two_streams(c, nullptr, nullptr, 0) : enqueue_cameras_one_stream(c, nullptr, nullptr, 0)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *us = us_since(t0);
  return GBP_OK;
}

struct Measurement {
  int reps = 0;
  double mine = 0;          // us per exchange on this rank
  double total_max = 0;     // warm-up + timed rounds, us, MAX over the ranks
};

// One measurement of the attached communicator in one schedule.  cap_us > 0: the baseline's first total — a candidate whose warm-up
// alone took longer on some rank gets kMeasureCappedReps timed rounds (agreed through the gather: every rank runs the same rounds).
// row[r] = rank r's figure.
int measure_attached(gbp_ctx* c, bool two_streams, double cap_us, Measurement* m, double* row) {
  c->xch.single_stream = !two_streams;
  if (int rc = ensure_comm_stream(c)) return rc;
  double warm = 0, timed = 0, all[2 * gbp::kCommMaxWorld];
  if (int rc = time_rounds(c, two_streams, kMeasureWarmup, &warm)) return rc;
  COMMCHK(c, c->xch.comm->all_gather_host(&warm, all, 1, e_));      // (ends in a barrier: the timed rounds start together)
  double warm_max = 0;
  for (int r = 0; r < c->world; ++r) warm_max = std::max(warm_max, all[r]);
  m->reps = cap_us > 0 && warm_max > cap_us ? kMeasureCappedReps : kMeasureReps;
  if (int rc = time_rounds(c, two_streams, m->reps, &timed)) return rc;
  m->mine = timed / m->reps;
  const double out[2] = {m->mine, warm + timed};
  COMMCHK(c, c->xch.comm->all_gather_host(out, all, 2, e_));
  m->total_max = 0;
  for (int r = 0; r < c->world; ++r) { row[r] = all[2 * r]; m->total_max = std::max(m->total_max, all[2 * r + 1]); }
  return GBP_OK;
}

// the ctx without its communicator, which the caller keeps or (destroy) drops the way gbp_destroy does, behind a barrier of the group
int comm_detach(gbp_ctx* c, bool destroy) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->xch.stream) HIPCHK(c, hipStreamSynchronize(c->xch.stream));
  gbp::Comm* k = c->xch.comm;
  c->xch.comm = nullptr; c->xch.send_dev = nullptr; c->xch.recv_dev = nullptr;
  if (!destroy || !k) return GBP_OK;
  std::string e;
  const int rc = k->barrier(e);      // nobody is inside an exchange of it any more
  delete k;
  return rc == 0 ? GBP_OK : fail(c, GBP_ERR_COMM, "exchange: " + e);
}

std::string candidate_name(const gbp::Candidate& k) {
  std::string n = gbp::transport_name(k.transport);
  if (k.transport == gbp::Transport::Rccl) n += k.two_streams ? " (two streams)" : " (one stream)";
  return n;
}

int comm_init_measured_body(gbp_ctx* c, void* region, gbp::Comm** kept) {
  using gbp::Transport;
  std::string err;
  gbp::RankFacts facts[gbp::kCommMaxWorld];
  if (gbp::comm_region_facts(region, c->rank, c->world, facts, err) != 0) return fail(c, GBP_ERR_COMM, "gbp_comm_init: " + err);
  const char* ss = std::getenv("GBP_COMM_SINGLE_STREAM");
  const gbp::Candidates cl = gbp::eligible_candidates(facts, c->world, ss ? (ss[0] == '1' ? 1 : 0) : -1);
  const gbp::Candidate& base = cl.c[cl.baseline];
  // (RCCL is made at most once: it is eligible only where it is also the baseline's transport, whose communicator is kept)
  auto attach_new = [&](Transport t) -> int {
    gbp::Comm* k = gbp::comm_create_in_region(region, c->rank, c->world, t, c->C, err);
    if (!k) return fail(c, GBP_ERR_COMM, "gbp_comm_init: " + err);
    return comm_attach(c, k);
  };
  if (c->world == 1) {      // nothing to measure
    if (int rc = attach_new(base.transport)) return rc;
    c->xch.selected_by = "rule";
    c->xch.measured = "[]";
    return GBP_OK;
  }
  // the order: the baseline; what else runs on its communicator (RCCL's other schedule); the other transports, each made once; the baseline again
  std::vector<int> order{cl.baseline};
  for (int pass = 0; pass < 2; ++pass)
    for (int i = 0; i < cl.n; ++i)
      if (i != cl.baseline && cl.c[i].eligible && (cl.c[i].transport == base.transport) == (pass == 0)) order.push_back(i);
  order.push_back(cl.baseline);
  std::vector<double> table((size_t)(cl.n + 1) * (size_t)c->world, 0.0);
  Measurement ms[gbp::kMaxCandidates + 1];
  double cap_us = 0;
  for (size_t step = 0; step < order.size(); ++step) {
    const gbp::Candidate& k = cl.c[order[step]];
    const int row = step + 1 == order.size() ? cl.n : order[step];
    if (!c->xch.comm || c->xch.comm->kind() != k.transport) {
      if (c->xch.comm) {      // the baseline's communicator waits for its second measurement, every other one has had its only
        const bool keep = c->xch.comm->kind() == base.transport;
        if (keep) *kept = c->xch.comm;
        if (int rc = comm_detach(c, !keep)) return rc;
      }
      if (k.transport == base.transport && *kept) {
        gbp::Comm* b = *kept;
        *kept = nullptr;
        if (int rc = comm_attach(c, b)) return rc;
      } else if (int rc = attach_new(k.transport)) {
        return rc;
      }
    }
    if (int rc = measure_attached(c, k.two_streams, cap_us, &ms[row], &table[(size_t)row * c->world])) return rc;
    if (step == 0) cap_us = ms[row].total_max;
  }
  const gbp::Choice ch = gbp::choose_transport(cl, table.data(), c->world);
  const gbp::Candidate& win = cl.c[ch.winner];
  if (c->xch.comm->kind() != win.transport) {
    if (int rc = comm_detach(c, true)) return rc;
    if (int rc = attach_new(win.transport)) return rc;
  }
  c->xch.single_stream = !win.two_streams;
  if (int rc = ensure_comm_stream(c)) return rc;
  if (c->xch.single_stream && c->xch.stream) {      // the second queue was only measured: it would slow every dispatch of the first
    HIPCHK(c, hipStreamSynchronize(c->xch.stream));
    HIPCHK(c, hipStreamDestroy(c->xch.stream));
    c->xch.stream = nullptr;
  }
  if (c->uploaded) {      // the winner's exchange buffers hold the partials the ctx's camera tables were made from, as after an iteration
    double us = 0;
    if (int rc = time_rounds(c, win.two_streams, 1, &us)) return rc;
  }
  c->xch.warm = 0;
  // the record
  const int base_row = ch.base_first <= ch.base_last ? cl.baseline : cl.n;
  std::string js = "[";
  char buf[320];
  for (int i = 0; i < cl.n; ++i) {
    const gbp::Candidate& k = cl.c[i];
    std::snprintf(buf, sizeof(buf), "%s{\"transport\": \"%s\", \"two_streams\": %s, \"eligible\": %s", i ? ", " : "", gbp::transport_name(k.transport),
                  k.two_streams ? "true" : "false", k.eligible ? "true" : "false");
    js += buf;
    if (!k.eligible) {
      js += std::string(", \"reason\": \"") + k.reason + "\"}";
      continue;
    }
    const int row = i == cl.baseline ? base_row : i;
    std::snprintf(buf, sizeof(buf), ", \"us_per_exchange\": %.3f, \"us_this_rank\": %.3f, \"reps\": %d", ch.figure[i], table[(size_t)row * c->world + c->rank], ms[row].reps);
    js += buf;
    if (i == cl.baseline) {
      std::snprintf(buf, sizeof(buf), ", \"baseline\": true, \"us_first\": %.3f, \"us_last\": %.3f", ch.base_first, ch.base_last);
      js += buf;
    }
    if (i == ch.winner) js += ", \"chosen\": true";
    js += "}";
  }
  c->xch.measured = js + "]";
  c->xch.selected_by = "measurement";
  std::snprintf(buf, sizeof(buf), "info: gbp_comm_init: measured %d rounds each, chose %s at %.1f us per exchange", kMeasureReps, candidate_name(win).c_str(), ch.figure[ch.winner]);
  std::string info = buf;
  if (ch.runner_up >= 0) {
    std::snprintf(buf, sizeof(buf), ", runner-up %s at %.1f us", candidate_name(cl.c[ch.runner_up]).c_str(), ch.figure[ch.runner_up]);
    info += buf;
  }
  std::snprintf(buf, sizeof(buf), "; what transport 0 attaches (%s): %.1f us first, %.1f us last", candidate_name(base).c_str(), ch.base_first, ch.base_last);
  info += buf;
  c->err = c->err.rfind("info:", 0) == 0 ? c->err + " | " + info : info;      // (behind gbp_create's own line, if the ctx still holds it)
  return GBP_OK;
}

int comm_init_measured(gbp_ctx* c, void* region) {
  gbp::Comm* kept = nullptr;
  const int rc = comm_init_measured_body(c, region, &kept);
  if (rc != GBP_OK) gbp::comm_region_abort(region);      // the other ranks leave their barriers with an error instead of waiting
  if (kept && kept != c->xch.comm) delete kept;
  return rc;
}

}  // namespace

GBP_EXPORT(gbp_comm_init, c, (gbp_ctx* c, void* region, int transport), (c, region, transport)) {
  if (!c || !region) return GBP_ERR_INVALID;
  if (c->xch.comm) return fail(c, GBP_ERR_STATE, "gbp_comm_init: the ctx already has a communicator");
  if (transport == (int)gbp::Transport::Measured) return comm_init_measured(c, region);
  std::string err;
  gbp::Comm* comm = gbp::comm_create_from_region(region, c->rank, c->world, static_cast<gbp::Transport>(transport), c->C, err);
  if (!comm) return fail(c, GBP_ERR_COMM, "gbp_comm_init: " + err);
  c->xch.selected_by = transport == (int)gbp::Transport::Auto ? "rule" : "caller";
  return comm_attach(c, comm);
}

GBP_EXPORT(gbp_comm_unique_id, nullptr, (void* id128), (id128)) {
  std::string err;
  if (!id128) return GBP_ERR_INVALID;
  if (gbp::comm_unique_id(id128, err) != 0) return fail(nullptr, GBP_ERR_COMM, "gbp_comm_unique_id: " + err);
  return GBP_OK;
}

GBP_EXPORT(gbp_comm_init_rccl, c, (gbp_ctx* c, const void* id128), (c, id128)) {
  if (!c || !id128) return GBP_ERR_INVALID;
  if (c->xch.comm) return fail(c, GBP_ERR_STATE, "gbp_comm_init_rccl: the ctx already has a communicator");
  std::string err;
  gbp::Comm* comm = gbp::comm_create_rccl(id128, c->rank, c->world, err);
  if (!comm) return fail(c, GBP_ERR_COMM, "gbp_comm_init_rccl: " + err);
  return comm_attach(c, comm);
}

// ---- what a first multi-GPU run wants on record (bench.py preflight) ---------------------------------------------------
GBP_EXPORT(gbp_comm_describe, c, (gbp_ctx* c, char* buf, size_t cap), (c, buf, cap)) {
  if (!c || !buf || cap == 0) return GBP_ERR_INVALID;
  int dev = 0;
  char bus[64] = {0};
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetPCIBusId(bus, sizeof(bus), dev);
  const std::string lib = c->xch.comm ? c->xch.comm->library_path() : "";
  char head[1024];
  std::snprintf(head, sizeof(head), "{\"rank\": %d, \"world\": %d, \"device\": %d, \"pci_bus_id\": \"%s\", \"transport\": \"%s\", \"library\": \"%s\", "
                                    "\"library_version\": %d, \"two_streams\": %s, \"selected_by\": \"%s\"",
                c->rank, c->world, dev, bus, c->xch.comm ? c->xch.comm->name() : "none", lib.c_str(), c->xch.comm ? c->xch.comm->library_version() : 0,
                (c->xch.comm && !c->xch.single_stream) ? "true" : "false", c->xch.selected_by);
  // transport 5: what gbp_comm_init timed, one entry per candidate (an empty list with one rank: nothing to measure)
  // how the loops with the metric (gbp_ba_loop, gbp_iterate_eval_each) have run on this ctx since gbp_comm_init: the path of the last burst
  char metric[512];
  const bool rides = c->xch.metric_last == 1;
  std::snprintf(metric, sizeof(metric), ", \"metric\": {\"path\": \"%s\", \"passes_riding\": %llu, \"passes_per_pass\": %llu, \"reason\": \"%s\"}",
                c->xch.metric_last == 0 ? "none" : rides ? "riding" : "per-pass", (unsigned long long)c->xch.metric_riding,
                (unsigned long long)c->xch.metric_per_pass, rides ? "" : c->xch.metric_reason);
  const std::string text = std::string(head) + (c->xch.measured.empty() ? "" : ", \"measured\": " + c->xch.measured) + metric + "}";
  std::snprintf(buf, cap, "%s", text.c_str());
  if (text.size() + 1 > cap) return fail(c, GBP_ERR_INVALID, "gbp_comm_describe: the text needs " + std::to_string(text.size() + 1) + " bytes");
  return GBP_OK;
}

// 0: the whole sharded iteration on ONE stream (sweep, beliefs + local partials, all-gather, combine); 1: the camera side of
// the exchange (local partials, all-gather) on a second, highest-priority stream beside the landmark beliefs.  Results are
// identical; which is faster depends on what the all-gather costs against ~10 us of second-queue overhead — measure
// (bench.py does, 20 iterations each) instead of guessing.
GBP_EXPORT(gbp_comm_set_schedule, c, (gbp_ctx* c, int two_streams), (c, two_streams)) {
  if (!c || !c->xch.comm) return fail(c, GBP_ERR_STATE, "gbp_comm_set_schedule: the ctx has no communicator");
  if (int rc = settle(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->xch.stream) HIPCHK(c, hipStreamSynchronize(c->xch.stream));
  drop_graph(c);
  c->xch.single_stream = two_streams == 0;
  return ensure_comm_stream(c);
}

// `reps` all-gathers of the camera partial buffers back to back on the ctx's stream (collective: every rank calls it);
// *avg_us = mean duration between two events.  The buffers keep their content (the gather of the same partials).
GBP_EXPORT(gbp_comm_probe, c, (gbp_ctx* c, int reps, double* avg_us), (c, reps, avg_us)) {
  if (!c || !c->xch.comm || !avg_us || reps < 1) return fail(c, GBP_ERR_STATE, "gbp_comm_probe: needs a communicator, reps >= 1");
  if (PeerComm* pc = peers(c->xch.comm)) {
    // p2p: this rank's slot of the next parity still holds the partials of two exchanges ago — give it the last ones, so that every
    // exchange of the probe (both parities) moves the same partials and leaves what a refresh reads unchanged
    HIPCHK(c, hipMemcpyAsync(c->xch.send_dev, pc->last_own_slot(), (size_t)c->C * kCamRec * 4, hipMemcpyDeviceToDevice, c->stream));
  }
  if (!c->xch.comm->stream_ordered()) {      // host-staged, p2p: wall clock around blocking exchanges
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < reps; ++i)
      if (int rc = exchange_now(c)) return rc;
    *avg_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
    return GBP_OK;
  }
  if (int rc = exchange_now(c)) return rc;     // warm (lazy channel set-up)
  HIPCHK(c, hipEventRecord(c->tm.reps_begin, c->stream));
  for (int i = 0; i < reps; ++i)
    if (int rc = exchange_now(c)) return rc;
  HIPCHK(c, hipEventRecord(c->tm.reps_end, c->stream));
  HIPCHK(c, hipEventSynchronize(c->tm.reps_end));
  float ms = 0;
  HIPCHK(c, hipEventElapsedTime(&ms, c->tm.reps_begin, c->tm.reps_end));
  *avg_us = 1e3 * ms / reps;
  return GBP_OK;
}

GBP_EXPORT_T(const char*, "none", gbp_comm_transport, (const gbp_ctx* c), (c)) { return (c && c->xch.comm) ? c->xch.comm->name() : "none"; }

GBP_EXPORT(gbp_comm_barrier, c, (gbp_ctx* c), (c)) {
  if (!c || !c->xch.comm) return GBP_ERR_STATE;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  COMMCHK(c, c->xch.comm->barrier(e_));
  return GBP_OK;
}

// gbp_eval over ALL shards: local sums gathered over the ranks and added in rank order (same bits on every rank)
GBP_EXPORT(gbp_eval_global, c, (gbp_ctx* c, gbp_eval_out* o), (c, o)) {
  if (!c || !o) return GBP_ERR_INVALID;
  const int rc = eval(c, o);
  if (rc != GBP_OK || !c->xch.comm) return rc;
  const double mine[7] = {o->sum_norm, o->sum_half_sq, (double)o->n_active, (double)o->n_relin, (double)o->n_robust,
                          (double)o->n_nonfinite, (double)o->n_nonpd};
  double all[7 * gbp::kCommMaxWorld];
  COMMCHK(c, c->xch.comm->all_gather_host(mine, all, 7, e_));
  double acc[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int r = 0; r < c->world; ++r)
    for (int i = 0; i < 7; ++i) acc[i] = acc[i] + all[r * 7 + i];
  o->sum_norm = acc[0]; o->sum_half_sq = acc[1]; o->n_active = (uint64_t)(acc[2] + 0.5); o->n_relin = (uint64_t)(acc[3] + 0.5);
  o->n_robust = (uint64_t)(acc[4] + 0.5); o->n_nonfinite = (uint64_t)(acc[5] + 0.5); o->n_nonpd = (uint64_t)(acc[6] + 0.5);
  return GBP_OK;
}
