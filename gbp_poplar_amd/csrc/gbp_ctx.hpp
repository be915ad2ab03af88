// gbp_ctx.hpp — the ONE internal header of the C-ABI implementation (include/gbp_mi355x*.h): the context, the helpers every
// translation unit shares, and the macro through which every exported function is defined.
//
//   gbp_api_ctx.cpp      life cycle + the host-stream programs: gbp_create / gbp_destroy, WRITE, READ, READ_PRIORS, NEW_KEYFRAME,
//                        gbp_sync, gbp_set_stream, gbp_timing                                   (ba.cpp:659-937, slam.cpp:913-928)
//   gbp_api_launch.cpp   what a program launches: LINEARISE, GBP_PROG (hipGraph replay / direct launches), WEAKEN_PRIORS, the
//                        split-phase iteration, and iterate_passes — the driver of passes without the metric (gbp_iterate,
//                        gbp_ba_loop without the metric)                                       (ba.cpp:863-865,890-905)
//   gbp_api_persist.cpp  the persistent kernel's launches: co-residency probe, snapshot, log of unvalidated launches (one typed
//                        Burst each), recovery — the replay of every BurstKind
//   gbp_api_eval.cpp     the metric on the device (util.cpp:74-144): gbp_eval*, gbp_iterate_eval, and iterate_passes_eval — the
//                        driver of passes with the metric after each (gbp_iterate_eval_each, gbp_ba_loop)  (ba.cpp:1001-1053)
//   gbp_loop_plan.hpp    where those drivers cut the reference's loop into pieces and where its weakenings fall (PassWalk): pure, no HIP
//   gbp_api_comm.cpp     sharded ctx: communicator glue, the sharded iteration, gbp_eval_global  (ba.cpp:414-417,617-649)
//   gbp_api_devio.cpp    WRITE, READ, READ_PRIORS, NEW_KEYFRAME for callers whose arrays live on the ctx's GPU (device pointers)
//   gbp_api_debug.cpp    the test hooks of include/gbp_mi355x_debug.h (test-hooks builds only)
//
// Replaces the Poplar graph / compute-set wiring of the reference (ba/ba.cpp:45-371, 659-937): where the reference maps vertices
// to IPU tiles and connects tensor slices, gbp_create sorts factors into device order (gbp_layout.cpp), builds the tile-coalesced
// arrays the kernels stream, and the launch TUs record the sequence of one iteration as a hipGraph.
#pragma once
#include "../../include/gbp_mi355x.h"
#include "../../include/gbp_mi355x_multi.h"
#include "../../include/gbp_mi355x_compat.h"
#ifdef GBP_BUILD_TEST_HOOKS
#include "../../include/gbp_mi355x_debug.h"
#endif
#include "gbp_comm.hpp"
#include "gbp_export.hpp"
#include "gbp_kernels.h"
#include "gbp_layout.hpp"
#include "gbp_loop_plan.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <utility>
#include <vector>

namespace gbp {
namespace api {
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};
// pinned host memory that the device reads and writes through `dev` (hipHostMallocMapped)
struct MappedBuf {
  void* host = nullptr;
  void* dev = nullptr;
  size_t bytes = 0;
};
}  // namespace api
}  // namespace gbp

struct gbp_ctx {
  using DevBuf = gbp::api::DevBuf;
  using MappedBuf = gbp::api::MappedBuf;
  // ---- the problem, the shard, the sizes of the device order, the stream: set by gbp_create (gbp_api_ctx.cpp), read by every unit ----
  uint32_t C = 0, L = 0, E = 0;       // global sizes
  uint32_t lmk_begin = 0, lmk_end = 0, L_loc = 0, E_loc = 0;
  int rank = 0, world = 1;
  float K[9];
  gbp_params prm;
  gbp::Layout lay;                         // device order (host side): position <-> file edge, rows, slots, tile order
  uint32_t Ep = 0, n_tiles = 0, n_rows = 0;
  int device = 0;                      // the GPU this ctx lives on (current device of gbp_create)
  bool use_tile_perm = false;
  bool use_seg_live = false;
  uint32_t sweep_policy = 0;           // kPol* bits of SweepArgs.policy for this graph's shape (sweep_policy_for)
  uint32_t sweep_issue = gbp::kSweepIssue;  // kIssue* bits of SweepArgs.issue (gbp_debug_force_sweep_policy + kPolForceLateRelin: the other order)
  bool hoist = true;  // per-variable belief means (k_sweep<true>); false = literal per-factor mu/oldmu tensors
  hipStream_t own_stream = nullptr, stream = nullptr;
  bool uploaded = false, beliefs_valid = false;
  bool lmk_half_done = false;          // gbp_iterate_local already refreshed the landmark beliefs of this iteration
  // ---- what the ctx owns on the HIP side (gbp_api_ctx.cpp): each kind is registered in one place and released by gbp_destroy, in
  // this order: events, device memory (dev_alloc), pinned memory (mapped_alloc), the two streams last ----
  std::vector<hipEvent_t*> events;     // the named events (event_create / event_pair_owned); pairs in flight live in their containers (tm.spans, tm.pending_*)
  std::vector<DevBuf*> all;
  std::vector<MappedBuf*> mapped;
  uint64_t dev_bytes = 0;
  // ---- the per-factor and per-variable device arrays: allocated by gbp_create (gbp_api_ctx.cpp), streamed by every launch ----
  struct Arrays {
    DevBuf fst_packed, fst_damp, fst_var;      // [Ep] the per-factor state planes (gbp_kernels.h)
    DevBuf row_cam, lmk_idx, fac, cmsg, mu, lmsg, camb, camp, lmkb, lmkp, rowp, local, d_cam_row_ptr, d_row_slot, d_lmk_ptr, cwf, lwf,
        cscale, lscale, cam_mu, lmk_mu, dK, hmu_c, hmu_l, clin, d_lmk_fpos, d_lmk_ix, health, tile_perm;
    DevBuf cmsg_lit;                     // CMSG_LIT (gbp_kernels.h): allocated by the first gbp_linearise that finds camera messages live
    bool cmsg_zero = true;               // no sweep has been set up since the zero fill of the last upload: every CMSG record is kCmsgZero
    DevBuf idx_arena;                    // the index arrays of the device order (row_cam, lmk_idx, lmk_fpos, lmk_ix, the row / landmark pointers, row_slot, K, tile_perm: views into it)
    DevBuf st_a, st_b;                   // [Ep] scratch of the per-factor state set kernel
    std::vector<uint8_t> active_host;    // [Ep] host shadow of the active flags (hoist guard of gbp_new_keyframe)
    // device-resident caller arrays (gbp_api_devio.cpp)
    DevBuf d_pos_edge;                   // [Ep] lay.pos_edge on the device; allocated by the first call that passes device pointers
    bool active_host_stale = false;      // a device-pointer call changed the active flags: the shadow is read back before its next use
    DevBuf seg_live;                     // [n_tiles] which segments (four positions) of a tile hold a factor (view into idx_arena; SweepArgs.seg_live)
  } arr;
  // ---- staging (gbp_api_ctx.cpp: H2D, D2H) ----
  struct Stage {
    // host -> device copies of small graphs go through this pinned, device-mapped buffer and a copy kernel (gbp_api_ctx.cpp: H2D)
    MappedBuf buf;
    size_t hint = 0;                     // what gbp_upload will stage: the buffer is pinned once, at that size (gbp_create)
  } stage;
  // ---- the captured iterations (gbp_api_launch.cpp; a sharded ctx: captured by gbp_api_comm.cpp) ----
  struct Graphs {
    hipGraph_t g = nullptr;
    hipGraphExec_t exec = nullptr;
    int iters = 0;
    bool failed = false;                 // a capture / instantiation failed once: direct launches from then on
    // the same for iterations that carry the metric (k_sweep<EV> + k_beliefs<EV>: gbp_iterate_eval_each beyond k_persist)
    hipGraph_t g_ev = nullptr;
    hipGraphExec_t exec_ev = nullptr;
    bool sharded = false;                // gbp_params.graph_unroll > 0 was asked for explicitly (see iterate_sharded)
  } graph;
  // ---- the metric (gbp_api_eval.cpp) ----
  struct Metric {
    DevBuf ev_cam, ev_lmk, ev_part, ev_ctl;   // metric records of the belief owners, ring of per-tile partial sums, counter + health words
    uint32_t ev_depth = 0;               // slots of the ring = iterations per piece of a burst
    MappedBuf ev_results;                // pinned + device-mapped: one gbp_eval_out per iteration of a burst (k_eval_fold)
    MappedBuf area;                      // pinned + device-mapped: k_eval writes the metric partials + health counters here
    // the metric into gbp_eval_out records on the GPU (gbp_eval / gbp_ba_loop / gbp_iterate_eval_each with a device `out`): the same
    // records in DEVICE memory, folded by k_eval_fold_part; allocated by the first call that needs them
    DevBuf scratch;                      // [1025] one result area of k_eval
    DevBuf series_twin;                  // [kSeriesMax][n_tiles + 1] the series slots of the persistent kernel
    int parity = 0, pending = 0;
    bool per_wave[2] = {false, false};   // result area written by k_persist (one record per tile wave) or by k_eval (one per workgroup)
    hipEvent_t ev[2] = {nullptr, nullptr};
  } metric;
  // ---- the persistent kernel (gbp_api_persist.cpp) ----
  enum class BurstKind {
    Plain,         // gbp_iterate, gbp_ba_loop without the metric
    MetricAtEnd,   // gbp_iterate_eval (metric in eval area `area`)
    SeriesHost,    // eval_each / gbp_ba_loop with metrics (blocking)
    SeriesDevice,  // the same with the results going to the caller's device records `out` (not blocking: the recovery replays passes and metrics)
  };
  // One launch of the persistent kernel: what launch_persist_burst is asked for, and — with seq filled in — its entry in the log
  struct Burst {
    BurstKind kind = BurstKind::Plain;
    int n = 0;                           // passes
    int area = 0;                        // the metric's result / health area (every kind but Plain)
    unsigned first = 0, steps2 = 0;      // steps2 != 0: the launch weakens priors itself (gbp_ba_loop: loop index of its first pass, twice the --steps)
    void* out = nullptr;                 // SeriesDevice: the caller's records
    unsigned seq = 0;                    // its number among the launches of the ctx (launch_persist_burst)
  };
  struct Persist {
    // k_persist (small graphs): n iterations in one launch
    bool ok = false;                     // bursts run inside k_persist (eligible, co-resident, no time-out since the last upload)
    bool eligible = false;               // what `ok` returns to at the next gbp_upload after a recovered time-out
    bool coop = false;                   // launched with hipLaunchCooperativeKernel (co-residency guaranteed by the runtime / driver)
    // A launch whose barrier timed out (workgroups not co-resident: e.g. another process holds CUs) is UNDONE and replayed on the
    // two-kernel path: every launch is preceded by a snapshot of the arrays it mutates (one copy kernel, skipped once the abort
    // word is set), later launches of the ctx return at once, and the host — at the next point where it synchronises anyway —
    // restores the snapshot and replays the logged launches from the first failed one on.
    DevBuf pflow;                        // tagged shadows of k_persist_flow (PersistFlow), one allocation
    gbp::PersistFlow flow{};                  // the tagged shadows of k_persist_flow
    size_t flow_bytes = 0;               // the shadows (and their redundant copies): what the first launch of a tag period clears (gbp_persist_seq.hpp)
    uint32_t flow_total4 = 0;            // test-hooks builds: float4 of the shadows (the redundant copies of gbp_debug_persist_verify follow them)
    bool use_flow = true;                // test-hooks build: gbp_debug_persist_flow(ctx, 0) / GBP_PERSIST_FLOW=0 run the barrier kernel of rounds 3-4 instead
    std::vector<Burst> log;              // launched, completion not yet validated
    unsigned seq = 0;                    // the number of the last launch (0: none yet); the next one: persist_next_seq (gbp_persist_seq.hpp)
    DevBuf psnap;                        // snapshot arena
    gbp::CopySegs snap_save{}, snap_restore{};
    double probe_ms = 0;                 // gbp_create: what the co-residency probe took (the first kernel launch of the process: code-object load included)
    DevBuf psync;                        // barrier words
    MappedBuf status;                    // pinned + device-mapped: raised by the kernel if a barrier gave up (read: persist_failed_seq)
    unsigned epoch_base = 0;             // arrivals the barrier counter has seen so far (it keeps counting across launches)
    MappedBuf series;                    // gbp_iterate_eval_each: [kSeriesMax metrics][1 + workgroups] slots, same kind of memory (read by gbp_api_eval.cpp)
  } persist;
  // ---- the exchange of a sharded ctx (gbp_api_comm.cpp) ----
  struct Exchange {
    void* send_dev = nullptr;
    void* recv_dev = nullptr;
    // library-owned exchange (gbp_comm_init*): communicator, buffers, a second stream so the all-gather overlaps the
    // rank-local landmark half of the belief update (fork / join through two events: capturable into the hipGraph)
    gbp::Comm* comm = nullptr;
    DevBuf xrecv;                        // [world][C][44] gathered camera partials; this rank writes its own slot (in-place all-gather)
    hipStream_t stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int warm = 0;                        // sharded iterations run directly so far (RCCL must have run before a capture)
    bool single_stream = false;          // all-gather on the main stream, no second queue (default for world <= 2)
    const char* selected_by = "caller";  // gbp_comm_describe: who chose the transport — "caller", "rule" (transport 0) or "measurement" (5)
    std::string measured;                // transport 5: the JSON list of what gbp_comm_init timed, one entry per candidate ("" for the others)
    // gbp_comm_describe's "metric" member: passes with the metric since gbp_comm_init, by path (gbp_transport.hpp: metric_rides)
    int metric_last = 0;                 // 0 none yet, 1 the last burst rode in the sharded iteration, 2 it ran the per-pass loop
    uint64_t metric_riding = 0, metric_per_pass = 0;
    const char* metric_reason = "";      // why the last per-pass burst did not ride (static text)
  } xch;
  // ---- timing and profiling (the brackets: gbp_api_ctx.cpp; recorded by the units that launch) ----
  struct Span { hipEvent_t a, b; };
  struct Timing {
    hipEvent_t reps_begin = nullptr, reps_end = nullptr;   // bracket of a run of repeated launches that the call itself waits for (gbp_comm_probe, gbp_debug_time_sweep)
    // gbp_iterate does not block the host: each call is bracketed by an event pair that is read later (gbp_timing, or
    // when the ring is full), so a caller that evaluates the metric every iteration pays ONE host synchronisation per
    // iteration (inside gbp_eval), not two
    std::vector<Span> spans;             // recorded, not yet read
    std::vector<Span> span_pool;         // reusable event pairs
    bool profile_stages = false;
    std::vector<Span> pending_sweep_ev;  // split-phase profiling: brackets not yet read
    double sweep_ms = 0, belief_ms = 0, total_ms = 0, exchange_ms = 0;
    std::vector<Span> pending_exch_ev;   // profiling: brackets of partials + all-gather
    uint64_t timed_iters = 0;
  } tm;
  // ---- texts (every unit: fail(), gbp_last_error) ----
  std::string warn;                    // text of the last recovered incident (also left in `err`, the call returns GBP_OK)
  std::string err;
};

namespace gbp {
namespace api {
using Burst = gbp_ctx::Burst;
using BurstKind = gbp_ctx::BurstKind;

// ---- errors -----------------------------------------------------------------------------------------------------------------
// (fail(), guarded() and the GBP_EXPORT macros: gbp_export.hpp)

#define HIPCHK(ctx, expr)                                                                          \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return ::gbp::api::fail(ctx, GBP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

#define COMMCHK(ctx, expr)                                                       \
  do {                                                                           \
    std::string e_;                                                              \
    if ((expr) != 0) return ::gbp::api::fail(ctx, GBP_ERR_COMM, "exchange: " + e_); \
  } while (0)

// ---- gbp_api_ctx.cpp --------------------------------------------------------------------------------------------------------
std::string& create_error();                                 // thread-local text of the last failed gbp_create / ctx-less call
int dev_alloc(gbp_ctx* c, DevBuf& b, size_t bytes);         // zero-filled device memory owned by the ctx (fill ordered on c->stream)
// Pinned, device-mapped host memory owned by the ctx, at least `bytes` of it (not filled).  A buffer that is too small is freed and
// pinned again at the new size — its contents are lost, and the caller has made sure that nothing on the device still uses it.
int mapped_alloc(gbp_ctx* c, MappedBuf& b, size_t bytes);
// Events owned by the ctx.  event_create / event_pair_owned: *e is a member of the ctx, destroyed with it.  event_pair: both events or
// none, handed to the caller's container (spans, span_pool, pending_*), which gbp_destroy walks as well.
int event_create(gbp_ctx* c, hipEvent_t* e, unsigned flags);
int event_pair(gbp_ctx* c, hipEvent_t* a, hipEvent_t* b, unsigned flags = hipEventDefault);
int event_pair_owned(gbp_ctx* c, hipEvent_t* a, hipEvent_t* b, unsigned flags);
template <class T> inline T* P(DevBuf& b) { return static_cast<T*>(b.p); }
// does this ctx combine camera partials through exchange buffers (sharded, or a 1-rank communicator)?
inline bool exch(const gbp_ctx* c) { return c->world > 1 || c->xch.comm != nullptr; }
// The host -> device copies of ONE call (gbp_create, gbp_upload, gbp_new_keyframe).  The first small and the first medium-sized
// hipMemcpy of a process cost 11 - 15 ms and 7 - 9 ms on this stack (set-up of two copy paths inside the runtime, profiles/exp_first_copy.hip)
// — more than the 1 500 iterations of a `ba fr1xyz` run.  A call that moves at most kStageMax bytes therefore stages its pieces in one
// pinned, device-mapped buffer and moves them with k_copy_segments on the ctx's stream (first launch 0.4 ms, then PCIe speed); larger
// calls use hipMemcpy, where those milliseconds do not matter.  put() copies out of `src` before it returns; end() returns with
// everything on the device (it synchronises the ctx's stream).
struct H2D {
  static constexpr size_t kStageMax = (size_t)32 << 20;
  gbp_ctx* c = nullptr;
  bool direct = true;
  size_t used = 0;
  CopySegs segs{};
  int begin(gbp_ctx* ctx, size_t total_bytes, int pieces);
  int put(void* dst_dev, const void* src, size_t bytes);      // dst: a whole DevBuf or a 16-byte aligned piece whose padded size is inside one
  int stage(const void* src, size_t bytes, const void** dev);  // staged only (!direct): the bytes where a kernel of the caller's reads them
  int end();
  int flush();
  // room for `bytes` (padded to whole float4s) in the staging buffer, at *off, and one copy segment queued: out of it to dst_dev, or
  // (dst_dev == NULL) into it from src_dev.  Launches the queued segments first when kMaxCopySegs of them wait.
  int queue(size_t bytes, void* dst_dev, const void* src_dev, size_t* off);
};
// ... and the device -> host copies of one call (gbp_read, gbp_read_priors), the same way round: get() queues, end() returns with every
// destination filled (the first device -> host hipMemcpy of a process pays the same set-up when no host -> device one came before it)
struct D2H {
  struct Out { void* dst; size_t off, bytes; };
  H2D up;
  std::vector<Out> pending;
  int begin(gbp_ctx* ctx, size_t total_bytes, int pieces);
  int get(void* dst_host, const void* src_dev, size_t bytes);
  int end();
};
// timing brackets of the iterate calls (read later: gbp_timing, or when the ring is full)
int resolve_spans(gbp_ctx* c, bool wait);
// The bracket of one iterate call.  begin() records its start event; end() its end event, handing the pair to c->tm.spans; commit(n)
// ends it (unless end() already has), counts n timed iterations and marks the beliefs valid.  A span that was never ended (an
// error return) gives its events back to c->tm.span_pool.
class TimedSpan {
 public:
  explicit TimedSpan(gbp_ctx* c) : c_(c) {}
  TimedSpan(const TimedSpan&) = delete;
  TimedSpan& operator=(const TimedSpan&) = delete;
  ~TimedSpan() { if (open_) c_->tm.span_pool.push_back(sp_); }
  int begin();
  int end();
  int commit(uint64_t n);
 private:
  gbp_ctx* c_;
  gbp_ctx::Span sp_{};
  bool open_ = false;
};
void drain_sweep_events(gbp_ctx* c);
// The construction knobs of the device order and the cache policy of the sweep: the defaults are the product.  Only the
// test-hooks build can change them (gbp_debug_layout_options / gbp_debug_force_sweep_policy: measurements and tests).
extern LayoutOptions g_layout_options;
extern int g_force_sweep_policy;
extern int g_force_seg_skip;      // -1: by shape; 0 / 1: never / always skip the all-pad segments in the sweep (gbp_debug_force_seg_skip)

// Per-factor scalar state lives in three planes indexed by device position (gbp_kernels.h)
inline FactorState factor_state(gbp_ctx* c) { return FactorState{P<int>(c->arr.fst_packed), P<float>(c->arr.fst_damp), P<float>(c->arr.fst_var)}; }
inline size_t tile_off(uint32_t p, int G, int f) {  // float offset of float f of position p in a G-group tiled array
  return (((size_t)(p >> 6) * G + (f >> 2)) * 64 + (p & 63)) * 4 + (f & 3);
}

// ---- gbp_api_launch.cpp -----------------------------------------------------------------------------------------------------
SweepArgs sweep_args(gbp_ctx* c, bool sweeps = true);      // sweeps = false: for a launch that runs no sweep (k_linearise, the hooks)
BeliefArgs belief_args(gbp_ctx* c);
void weaken_args(gbp_ctx* c, BeliefArgs& b);                  // the prior arrays WeakenPriorVertex writes (b.weaken is the caller's)
void drop_graph(gbp_ctx* c);
// (where the reference's loop weakens and how the drivers below cut it into pieces: gbp_loop_plan.hpp)
// camera beliefs from stored partials (single GPU: the local sums; sharded: recv_dev) + landmark beliefs re-summed.  roll = true
// at the end of an iteration, false for prior-only refreshes (WEAKEN_PRIORS, NEW_KEYFRAME, LINEARISE).
int refresh_beliefs_from_partials(gbp_ctx* c, bool roll, bool do_lmk = true, bool weaken = false);
void enqueue_iteration(gbp_ctx* c, const SweepArgs& a, bool ev = false, bool weaken_after = false);
void enqueue_cam_partials(gbp_ctx* c, float* dst, hipStream_t s = nullptr);
int iterate_plain(gbp_ctx* c, const SweepArgs& a, int n, bool ev = false);                      // hipGraph replays + remainder
int iterate_weaken_plain(gbp_ctx* c, const SweepArgs& a, int n, unsigned i0, unsigned steps2);  // the same with the loop's weakenings riding (the one in front of pass i0: the caller's)
int iterate_passes(gbp_ctx* c, int n, unsigned i0, unsigned steps2);  // the driver of passes without the metric (single GPU), weakenings included
int iterate(gbp_ctx* c, int n);                              // GBP_PROG x n: persistent kernel / hipGraph / sharded
int weaken_priors(gbp_ctx* c);                               // WEAKEN_PRIORS

// ---- gbp_api_persist.cpp ----------------------------------------------------------------------------------------------------
constexpr int kPersistChunk = 4096;      // iterations per k_persist launch (a launch cannot be pre-empted: ~60 ms at 15 us each)
// What became of a burst, beside the status code of the call (GBP_OK with every one of them)
enum class BurstOutcome {
  Ran,
  NotRun,      // launch_persist_burst: nothing ran, the ctx has left the persistent path
  TimedOut,    // series_burst (blocking): the launch ran, timed out, and the state was restored to the start of the burst
};
// the status word the kernel raises (host-mapped; valid once persist_setup has allocated it): the number of the first launch of this
// ctx that gave up at a wait, 0 while none has
inline volatile unsigned& persist_status_word(const gbp_ctx* c) { return *static_cast<volatile unsigned*>(c->persist.status.host); }
inline unsigned persist_failed_seq(const gbp_ctx* c) { return persist_status_word(c); }
// do this ctx's bursts hand off through tagged records (k_persist_flow, which also weakens in front of its later passes: PassWalk's
// weaken_inside)?  Not the barrier kernel of the test-hooks build.
inline bool persist_tagged(const gbp_ctx* c) { return c->persist.use_flow && c->persist.flow.lmsg != nullptr; }
int persist_setup(gbp_ctx* c, const gbp_params* prm, bool sharded);   // gbp_create: probe, snapshot arena, tagged shadows (or none: not eligible)
void persist_forget(gbp_ctx* c);                            // gbp_destroy: its launches have ended, nobody waits for this ctx again
int persist_reset(gbp_ctx* c);                              // gbp_upload: a fresh start for the persistent path
// Every entry point that enqueues other device work, or changes what the launches in flight depend on, first makes sure they
// completed without a time-out (and repairs the state if one did): free when nothing is in flight.
int settle(gbp_ctx* c);
int persist_check(gbp_ctx* c, unsigned upto);               // the stream has been synchronised / an event behind launch `upto` completed
bool stream_is_capturing(gbp_ctx* c);
// One GPU, no communicator, no per-stage profiling, the ctx's stream not being captured right now (asked on every call): the ctx whose
// passes the drivers of this library plan themselves (iterate_passes, the riding metric, the persistent kernel)
inline bool plain_single_gpu(gbp_ctx* c) { return !c->xch.comm && c->world == 1 && !c->tm.profile_stages && !stream_is_capturing(c); }
int persist_ready(gbp_ctx* c, bool* yes);                   // may the next burst run inside the persistent kernel?
// the launch that runs piece p of a loop with weakenings under steps2 (area and out: the caller's)
inline Burst burst_of(BurstKind kind, const Piece& p, unsigned steps2) { Burst b; b.kind = kind; b.n = p.m; b.first = p.first; b.steps2 = steps2; return b; }
// b.n passes in ONE launch of the persistent kernel (+ the metric phases `ev`, for every kind but Plain); logged as b with its seq
int launch_persist_burst(gbp_ctx* c, const SweepArgs& a, const gbp_ctx::Burst& b, const PersistEval* ev, BurstOutcome* outcome);

// ---- gbp_api_eval.cpp -------------------------------------------------------------------------------------------------------
// k_means + k_eval of the current beliefs with the health words of area `area`, into that result area (host-mapped, its event recorded
// behind them) or into dev_slots (device memory, [1025]: no event)
int eval_enqueue(gbp_ctx* c, int area, DeviceEval* dev_slots = nullptr);
// The driver of passes with the metric after each (gbp_iterate_eval_each, gbp_ba_loop): passes i0 .. i0 + n - 1 of the reference's loop,
// out[k] = the metric after pass i0 + k.  dev: out is memory of the ctx's GPU, nothing blocks.  replay: the recovery of a timed-out
// SeriesDevice launch (persist_recover) runs its passes through the same driver, off the persistent path, into the same records.
int iterate_passes_eval(gbp_ctx* c, int n, unsigned i0, unsigned steps2, gbp_eval_out* out, bool dev = false, bool replay = false);
int eval_begin(gbp_ctx* c);
int eval_end(gbp_ctx* c, gbp_eval_out* o);
int eval(gbp_ctx* c, gbp_eval_out* o);

// ---- gbp_api_devio.cpp ------------------------------------------------------------------------------------------------------
// What kind of memory a caller's pointer is (hipPointerGetAttributes): host = pageable or pinned / registered host memory (today's
// path); device = memory of the ctx's GPU.  Leaves no error behind in the runtime (an unregistered pointer is reported as one).
enum PtrKind { kPtrHost = 0, kPtrDevice = 1, kPtrOtherDevice = 2, kPtrManaged = 3 };
inline PtrKind ptr_kind(const gbp_ctx* c, const void* p) {
  hipPointerAttribute_t at;
  std::memset(&at, 0, sizeof(at));
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return kPtrHost; }
  if (at.type == hipMemoryTypeManaged || at.isManaged) return kPtrManaged;
  if (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeArray) return at.device == c->device ? kPtrDevice : kPtrOtherDevice;
  return kPtrHost;
}
// One struct of a call: every non-NULL member must be of the kind of the first.  *device = the struct holds device pointers.
// GBP_ERR_INVALID (text names the member): a mix, another GPU's memory, managed memory, a landmark-sharded ctx.
int struct_kind(gbp_ctx* c, const char* fn, const void* const* members, const char* const* names, int n, bool* device);
// The device-pointer forms of the four programs (gbp_api_devio.cpp).
int devio_upload(gbp_ctx* c, const gbp_state_in* in);
int devio_read(gbp_ctx* c, gbp_state_out* out);
int devio_read_priors(gbp_ctx* c, gbp_priors_out* out);
int devio_new_keyframe(gbp_ctx* c, const gbp_kf_update* upd);
int devio_refresh_active_shadow(gbp_ctx* c);   // c->arr.active_host from the device (after a device-pointer call changed the flags)

// ---- gbp_api_comm.cpp -------------------------------------------------------------------------------------------------------
int exchange_now(gbp_ctx* c, hipStream_t s = nullptr);      // plain all-gather of the camera partials on the ctx's stream (or on s)
int iterate_sharded(gbp_ctx* c, int n);
int iterate_sharded_ev(gbp_ctx* c, const SweepArgs& a, int n);   // n iterations with the metric riding (a.ev set), launched directly
int zero_exchange(gbp_ctx* c);                              // gbp_upload: the gathered partials (of both parities) cleared on the ctx's stream
int refresh_cameras(gbp_ctx* c, BeliefArgs& b, bool do_lmk);   // the launches of refresh_beliefs_from_partials, by transport

}  // namespace api
}  // namespace gbp
