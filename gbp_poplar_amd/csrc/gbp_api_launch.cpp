// gbp_api_launch.cpp — what the programs of the list launch (include/gbp_mi355x.h):
//   gbp_linearise        LINEARISE_PROG   reference ba/ba.cpp:890-893   belief refresh + k_linearise
//   gbp_iterate          GBP_PROG x n     ba.cpp:895-905                persistent kernel / hipGraph replay / direct launches: iterate_passes,
//                                                                       the driver gbp_ba_loop without the metric shares
//   gbp_weaken_priors    WEAKEN_PRIORS    ba.cpp:863-865                ONE k_beliefs launch (the prior owners scale on their way into the sums)
//   gbp_prepare          Engine::load     ba.cpp:936-937                hipGraph capture + instantiation, runs nothing
// and the split-phase form of the iteration (include/gbp_mi355x_multi.h) for callers that run the exchange themselves.
#include "gbp_ctx.hpp"

#include <algorithm>

using namespace gbp;
using namespace gbp::api;

namespace gbp {
namespace api {

// (every path that runs sweeps — direct launches, graph captures, the persistent kernel — takes its arguments from here, so from here
// on the camera messages count as live: what gbp_linearise_factors looks at)
SweepArgs sweep_args(gbp_ctx* c, bool sweeps) {
  if (sweeps) c->arr.cmsg_zero = false;
  SweepArgs a;
  a.row_cam = P<uint32_t>(c->arr.row_cam); a.lmk_idx = P<uint32_t>(c->arr.lmk_idx); a.fac = P<float4>(c->arr.fac); a.cmsg = P<float4>(c->arr.cmsg);
  a.cmsg_lit = P<float4>(c->arr.cmsg_lit);
  a.mu = P<float4>(c->arr.mu); a.lmsg = P<float4>(c->arr.lmsg); a.fst_packed = P<int>(c->arr.fst_packed); a.fst_damp = P<float>(c->arr.fst_damp); a.fst_var = P<float>(c->arr.fst_var); a.camb = P<float4>(c->arr.camb); a.lmkb = P<float4>(c->arr.lmkb);
  a.rowp = P<float4>(c->arr.rowp);
  a.cam_mu = P<float4>(c->arr.hmu_c); a.lmk_mu = P<float4>(c->arr.hmu_l); a.cam_lin = P<float4>(c->arr.clin);
  std::memcpy(a.K, c->K, sizeof(a.K));
  a.hp.maxeta_damping = c->prm.maxeta_damping; a.hp.num_undamped_iters = c->prm.num_undamped_iters;
  a.hp.dmu_threshold = c->prm.dmu_threshold; a.hp.min_linear_iters = c->prm.min_linear_iters;
  a.hp.nstds = c->prm.nstds; a.hp.relin_mode = c->prm.relin_mode;
  a.variant = c->prm.reserved[0];      // read by the experiments build only
  a.tile_perm = c->use_tile_perm ? P<uint32_t>(c->arr.tile_perm) : nullptr;
  a.seg_live = c->use_seg_live ? P<uint32_t>(c->arr.seg_live) : nullptr;
  a.policy = c->sweep_policy;
  a.issue = c->sweep_issue;
  a.ev = EvalRide{};
  return a;
}

void drop_graph(gbp_ctx* c) {
  if (c->graph.exec) { (void)hipGraphExecDestroy(c->graph.exec); c->graph.exec = nullptr; }
  if (c->graph.g) { (void)hipGraphDestroy(c->graph.g); c->graph.g = nullptr; }
  if (c->graph.exec_ev) { (void)hipGraphExecDestroy(c->graph.exec_ev); c->graph.exec_ev = nullptr; }
  if (c->graph.g_ev) { (void)hipGraphDestroy(c->graph.g_ev); c->graph.g_ev = nullptr; }
  c->graph.iters = 0;
}

BeliefArgs belief_args(gbp_ctx* c) {
  BeliefArgs b{};
  b.rowp = P<float>(c->arr.rowp); b.cam_row_ptr = P<uint32_t>(c->arr.d_cam_row_ptr); b.cam_prior = P<float>(c->arr.camp);
  b.row_slot = c->lay.row_slot.empty() ? nullptr : P<uint32_t>(c->arr.d_row_slot);
  b.cam_local = P<float>(c->arr.local); b.gathered = nullptr; b.world = c->world;
  b.camb = P<float>(c->arr.camb); b.cam_mu = P<float4>(c->arr.hmu_c); b.cam_lin = P<float4>(c->arr.clin); b.n_cams = c->C;
  b.lmk_prior = P<float4>(c->arr.lmkp); b.lmsg = P<float4>(c->arr.lmsg); b.lmk_ptr = P<uint32_t>(c->arr.d_lmk_ptr);
  b.lmk_fpos = P<uint32_t>(c->arr.d_lmk_fpos); b.lmk_ix = P<uint32_t>(c->arr.d_lmk_ix);
  b.lmkb = P<float4>(c->arr.lmkb); b.lmk_mu = P<float4>(c->arr.hmu_l); b.n_lmks = c->L_loc;
  b.partial_only = 0; b.hoist = c->hoist ? 1 : 0; b.roll = 0;
  b.lmk_blocks = 0; b.lmk_xcd_order = c->prm.tile_order != 1 ? 1 : 0;
  return b;
}

void weaken_args(gbp_ctx* c, BeliefArgs& b) {
  b.cam_prior_rw = P<float>(c->arr.camp); b.cam_scale = P<float>(c->arr.cscale); b.cam_wflag = P<uint32_t>(c->arr.cwf);
  b.lmk_prior_rw = P<float4>(c->arr.lmkp); b.lmk_scale = P<float>(c->arr.lscale); b.lmk_wflag = P<uint32_t>(c->arr.lwf);
}


// camera beliefs from stored partials (single GPU: d_local; multi: recv_dev) + landmark beliefs re-summed.
// roll = true at the end of an iteration (the sweep has consumed the current means), false for
// prior-only refreshes (WEAKEN_PRIORS, NEW_KEYFRAME, LINEARISE).
int refresh_beliefs_from_partials(gbp_ctx* c, bool roll, bool do_lmk, bool weaken) {
  BeliefArgs b = belief_args(c);
  if (weaken) {
    b.weaken = 1;
    weaken_args(c, b);
  }
  b.roll = roll ? 1 : 0;
  return refresh_cameras(c, b, do_lmk);      // (which launches, by transport: gbp_api_comm.cpp)
}

// one iteration: k_sweep + k_beliefs; ev: the instantiations that carry the metric (a.ev filled in by the caller)
// weaken_after: WEAKEN_PRIORS follows this iteration with nothing reading the beliefs in between — its belief update takes the
// weakened priors straight away (WeakenPriorVertex rides in k_beliefs as in gbp_weaken_priors): the same beliefs, means and
// mean changes as {k_beliefs; k_beliefs(weaken)} leave, in one launch
void enqueue_iteration(gbp_ctx* c, const SweepArgs& a, bool ev, bool weaken_after) {
  launch_sweep(a, c->n_tiles, c->hoist, c->stream, ev);
  BeliefArgs b = belief_args(c);
  b.roll = 1;
  if (weaken_after) {
    b.weaken = 1;
    weaken_args(c, b);
  }
  if (ev) b.ev = a.ev;
  launch_beliefs(b, true, true, c->stream, ev);
}

// local camera partials only (before an exchange / before a prior-only refresh)
void enqueue_cam_partials(gbp_ctx* c, float* dst, hipStream_t s) {
  BeliefArgs b = belief_args(c);
  b.cam_local = dst; b.partial_only = 1;
  launch_beliefs(b, true, false, s ? s : c->stream);
}

// Capture `graph_unroll` single-GPU iterations once (nothing is executed by a capture).  Any failure leaves the stream
// out of capture mode, drops the partial graph and falls back to direct launches for the life of the ctx (results are
// identical either way).
static bool ensure_graph(gbp_ctx* c, const SweepArgs& a, bool ev = false) {
  hipGraph_t& g = ev ? c->graph.g_ev : c->graph.g;
  hipGraphExec_t& x = ev ? c->graph.exec_ev : c->graph.exec;
  if (x) return true;
  if (c->graph.failed || c->prm.graph_unroll <= 0 || c->stream != c->own_stream) return false;
  hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal);
  if (e == hipSuccess) {
    for (int i = 0; i < c->prm.graph_unroll; ++i) enqueue_iteration(c, a, ev);
    e = hipStreamEndCapture(c->stream, &g);          // also ends a capture that was invalidated on the way
    if (e == hipSuccess) e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    drop_graph(c);
    c->graph.failed = true;
    return false;
  }
  c->graph.iters = c->prm.graph_unroll;
  return true;
}

// GBP_PROG x n on the two-kernel path: replay of a captured hipGraph of `graph_unroll` iterations, remainder launched directly.
// (ev: the iterations carry the metric — a.ev set, see eval_each_ride; their launches depend on the iteration only through a
// counter in device memory, so they replay from a graph of their own)
int iterate_plain(gbp_ctx* c, const SweepArgs& a, int n, bool ev) {
  int left = n;
  bool use_graph = (c->stream == c->own_stream) && c->prm.graph_unroll > 0 && n >= c->prm.graph_unroll && !c->graph.failed;
  if (use_graph && !(ev ? c->graph.exec_ev : c->graph.exec)) use_graph = ensure_graph(c, a, ev);
  if (use_graph) {
    while (left >= c->graph.iters) {
      HIPCHK(c, hipGraphLaunch(ev ? c->graph.exec_ev : c->graph.exec, c->stream));
      left -= c->graph.iters;
    }
  }
  for (; left > 0; --left) enqueue_iteration(c, a, ev);
  HIPCHK(c, hipGetLastError());
  return GBP_OK;
}

// Passes i0 .. i0 + n - 1 of the reference's loop WITHOUT the metric on the two-kernel path of a single-GPU ctx, the weakening in
// front of pass i0 (if any) already done by the caller: a weakening in front of a later pass rides in the belief update of the
// iteration before it (enqueue_iteration: weaken_after), the runs between them replay from the hipGraph.
int iterate_weaken_plain(gbp_ctx* c, const SweepArgs& a, int n, unsigned i0, unsigned steps2) {
  for (PassWalk w(n, i0, steps2, /*front_done=*/true); !w.done();) {
    const Piece p = w.next(kNoCap, /*weaken_inside=*/false);
    const bool weaken_after = !w.done();      // the run's last iteration takes the weakened priors in its belief update
    if (int rc = iterate_plain(c, a, p.m - (weaken_after ? 1 : 0))) return rc;
    if (weaken_after) {
      enqueue_iteration(c, a, false, true);
      HIPCHK(c, hipGetLastError());
    }
  }
  return GBP_OK;
}

// The driver of passes WITHOUT the metric (gbp_iterate: steps2 = 0; gbp_ba_loop without the metric): passes i0 .. i0 + n - 1 of the
// reference's loop on a single-GPU ctx; not blocking.  Small graphs run them inside the persistent kernel, in launches of at most
// kPersistChunk passes (a launch cannot be pre-empted) that apply the weakenings in front of their later passes themselves — only a
// weakening in front of a launch's first pass is a launch of its own; everything else — and the rest of the passes once the ctx has
// left the persistent path — runs on the two-kernel path (iterate_weaken_plain).
int iterate_passes(gbp_ctx* c, int n, unsigned i0, unsigned steps2) {
  PassWalk w(n, i0, steps2);
  if (w.weakens())
    if (int rc = weaken_priors(c)) return rc;
  bool persist = false;
  if (n >= 2)                          // a single iteration is as fast from two launches (measured)
    if (int rc = persist_ready(c, &persist)) return rc;
  if (!persist)
    if (int rc = settle(c)) return rc;
  const SweepArgs a = sweep_args(c);
  TimedSpan sp(c);
  if (int rc = sp.begin()) return rc;
  while (persist && !w.done()) {
    const Piece p = w.peek(kPersistChunk, persist_tagged(c));
    BurstOutcome ran;
    if (int rc = launch_persist_burst(c, a, burst_of(BurstKind::Plain, p, steps2), nullptr, &ran)) return rc;
    if (ran != BurstOutcome::Ran) break;
    w.take(p);
    if (!w.done()) {
      if (w.weakens())
        if (int rc = weaken_priors(c)) return rc;
      if (int rc = persist_ready(c, &persist)) return rc;
    }
  }
  if (!w.done()) {      // (settle: free unless the ctx has just left the persistent path with launches in flight)
    if (int rc = settle(c)) return rc;
    if (int rc = iterate_weaken_plain(c, a, w.left(), w.index(), steps2)) return rc;
  }
  HIPCHK(c, hipGetLastError());
  return sp.commit((uint64_t)n);
}

// GBP_PROG x n (ba.cpp:895-905).
int iterate(gbp_ctx* c, int n) {
  if (!c || !c->uploaded) return fail(c, GBP_ERR_STATE, "gbp_iterate: upload first");
  if (n <= 0) return GBP_OK;
  if (c->xch.comm) {
    if (int rc = settle(c)) return rc;
    return iterate_sharded(c, n);
  }
  if (c->world > 1)
    return fail(c, GBP_ERR_STATE, "sharded ctx without a communicator: gbp_comm_init first, or use gbp_iterate_begin / exchange / gbp_iterate_end");
  if (c->stream != c->own_stream && stream_is_capturing(c)) {
    // the caller is capturing its own stream (gbp_set_stream) into a graph: plain kernel launches only — no persistent kernel
    // (host-computed barrier targets), no timing events that would become graph nodes, no capture of our own inside theirs
    if (int rc = settle(c)) return rc;
    const SweepArgs a = sweep_args(c);
    for (int i = 0; i < n; ++i) enqueue_iteration(c, a);
    HIPCHK(c, hipGetLastError());
    c->beliefs_valid = true;
    return GBP_OK;
  }
  if (c->tm.profile_stages) {
    // Per-stage timing: all n iterations are queued back to back with a hipEvent before / between / after the
    // two kernels, and read after ONE synchronisation, so a bracket holds the kernel (plus the ~1 us
    // dependent-launch gap), not the idle-queue start-up latency a per-iteration sync would add.
    if (int rc = settle(c)) return rc;
    const SweepArgs a = sweep_args(c);
    TimedSpan sp(c);
    if (int rc = sp.begin()) return rc;
    struct Events {   // freed on every exit path
      std::vector<hipEvent_t> v;
      ~Events() { for (hipEvent_t e : v) if (e) (void)hipEventDestroy(e); }
    } evs;
    evs.v.assign(2 * (size_t)n + 1, nullptr);
    std::vector<hipEvent_t>& ev = evs.v;
    for (auto& e : ev) HIPCHK(c, hipEventCreate(&e));
    HIPCHK(c, hipEventRecord(ev[0], c->stream));
    for (int i = 0; i < n; ++i) {
      launch_sweep(a, c->n_tiles, c->hoist, c->stream);
      HIPCHK(c, hipEventRecord(ev[2 * i + 1], c->stream));
      BeliefArgs b = belief_args(c);
      b.roll = 1;
      launch_beliefs(b, true, true, c->stream);
      HIPCHK(c, hipEventRecord(ev[2 * i + 2], c->stream));
    }
    HIPCHK(c, hipEventSynchronize(ev[2 * (size_t)n]));
    for (int i = 0; i < n; ++i) {
      float a_ms = 0, b_ms = 0;
      HIPCHK(c, hipEventElapsedTime(&a_ms, ev[2 * i], ev[2 * i + 1]));
      HIPCHK(c, hipEventElapsedTime(&b_ms, ev[2 * i + 1], ev[2 * i + 2]));
      c->tm.sweep_ms += a_ms; c->tm.belief_ms += b_ms;
    }
    HIPCHK(c, hipGetLastError());
    return sp.commit((uint64_t)n);
  }
  return iterate_passes(c, n, 0, 0);
}

// WEAKEN_PRIORS (ba.cpp:863-865): WeakenPriorVertex on every variable, then prog_ub.
int weaken_priors(gbp_ctx* c) {
  if (!c || !c->uploaded) return fail(c, GBP_ERR_STATE, "gbp_weaken_priors: upload first");
  if (int rc = settle(c)) return rc;
  return refresh_beliefs_from_partials(c, false, true, /*weaken=*/true);      // ONE launch: the prior owners scale on their way into the sums
}

}  // namespace api
}  // namespace gbp

GBP_EXPORT(gbp_iterate, c, (gbp_ctx* c, int n), (c, n)) { return iterate(c, n); }
GBP_EXPORT(gbp_weaken_priors, c, (gbp_ctx* c), (c)) { return weaken_priors(c); }

GBP_EXPORT(gbp_refresh_begin, c, (gbp_ctx* c), (c)) {
  if (!c || !c->uploaded) return fail(c, GBP_ERR_STATE, "upload first");
  if (int rc = settle(c)) return rc;
  float4* dst = exch(c) ? static_cast<float4*>(c->xch.send_dev) : P<float4>(c->arr.local);
  if (!dst) return fail(c, GBP_ERR_STATE, "exchange buffers not set");
  enqueue_cam_partials(c, reinterpret_cast<float*>(dst));
  HIPCHK(c, hipGetLastError());
  return GBP_OK;
}

GBP_EXPORT(gbp_refresh_end, c, (gbp_ctx* c), (c)) {
  if (!c || !c->uploaded) return fail(c, GBP_ERR_STATE, "upload first");
  if (int rc = settle(c)) return rc;
  const int rc = refresh_beliefs_from_partials(c, false);
  if (rc == GBP_OK) c->beliefs_valid = true;
  return rc;
}

GBP_EXPORT(gbp_linearise_factors, c, (gbp_ctx* c), (c)) {
  if (!c || !c->uploaded) return fail(c, GBP_ERR_STATE, "upload first");
  if (int rc = settle(c)) return rc;
  if (!c->arr.cmsg_zero && !c->arr.cmsg_lit.p) {
    // LINEARISE under live messages: k_linearise rewrites the potentials the kCmsgDerived records derive their Lambda from, so it
    // first makes those records literal (gbp_kernels.h: CMSG) — in a side array that only such a call pays for.  A captured graph
    // holds the sweep's arguments without it: dropped, the next burst captures again.
    if (int rc = dev_alloc(c, c->arr.cmsg_lit, (size_t)c->Ep * kCmsgLitG * 16)) return rc;
    drop_graph(c);
  }
  launch_linearise(sweep_args(c, /*sweeps=*/false), c->n_tiles, c->stream);
  HIPCHK(c, hipGetLastError());
  return GBP_OK;
}

// LINEARISE_PROG (ba.cpp:890-893): prog_ub, then RelineariseFactorVertex on every factor.
GBP_EXPORT(gbp_linearise, c, (gbp_ctx* c), (c)) {
  if (!c || !c->uploaded) return fail(c, GBP_ERR_STATE, "gbp_linearise: upload first");
  if (c->world > 1 && !c->xch.comm)
    return fail(c, GBP_ERR_STATE, "sharded ctx without a communicator: gbp_comm_init first, or use refresh_begin / exchange / refresh_end / linearise_factors");
  int rc = gbp_refresh_begin(c);
  if (rc == GBP_OK && c->xch.comm) rc = exchange_now(c);
  if (rc == GBP_OK) rc = gbp_refresh_end(c);
  if (rc == GBP_OK) rc = gbp_linearise_factors(c);
  return rc;
}

GBP_EXPORT(gbp_iterate_begin, c, (gbp_ctx* c), (c)) {
  if (!c || !c->uploaded) return fail(c, GBP_ERR_STATE, "upload first");
  if (int rc = settle(c)) return rc;
  float4* dst = exch(c) ? static_cast<float4*>(c->xch.send_dev) : P<float4>(c->arr.local);
  if (!dst) return fail(c, GBP_ERR_STATE, "exchange buffers not set");
  if (c->tm.profile_stages) {  // bracket the sweep launch; the pair is read (and timed_iters counted) by gbp_timing
    if (c->tm.pending_sweep_ev.size() >= 256) drain_sweep_events(c);   // bounded: long profiled runs never pile up events
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (int rc = event_pair(c, &e0, &e1)) return rc;
    c->tm.pending_sweep_ev.push_back({e0, e1});
    HIPCHK(c, hipEventRecord(e0, c->stream));
    launch_sweep(sweep_args(c), c->n_tiles, c->hoist, c->stream);
    HIPCHK(c, hipEventRecord(e1, c->stream));
  } else {
    launch_sweep(sweep_args(c), c->n_tiles, c->hoist, c->stream);
  }
  enqueue_cam_partials(c, reinterpret_cast<float*>(dst));
  HIPCHK(c, hipGetLastError());
  return GBP_OK;
}

// The landmark half of the belief update needs nothing from other ranks: a caller may run it while the
// all-gather of the camera partials is in flight (between gbp_iterate_begin and gbp_iterate_end).
GBP_EXPORT(gbp_iterate_local, c, (gbp_ctx* c), (c)) {
  if (!c || !c->uploaded) return fail(c, GBP_ERR_STATE, "upload first");
  if (int rc = settle(c)) return rc;
  BeliefArgs b = belief_args(c);
  b.roll = 1;
  launch_beliefs(b, false, true, c->stream);
  HIPCHK(c, hipGetLastError());
  c->lmk_half_done = true;
  return GBP_OK;
}

GBP_EXPORT(gbp_iterate_end, c, (gbp_ctx* c), (c)) {
  if (!c || !c->uploaded) return fail(c, GBP_ERR_STATE, "upload first");
  if (int rc = settle(c)) return rc;
  const int rc = refresh_beliefs_from_partials(c, true, !c->lmk_half_done);
  c->lmk_half_done = false;
  if (rc == GBP_OK) c->beliefs_valid = true;
  return rc;
}

// One-off costs of the multi-iteration path, paid on request instead of inside the first gbp_iterate(n >= graph_unroll):
// graph capture + instantiation + upload of the executable graph.  Executes no iteration.
GBP_EXPORT(gbp_prepare, c, (gbp_ctx* c), (c)) {
  if (!c || !c->uploaded) return fail(c, GBP_ERR_STATE, "gbp_prepare: upload first");
  if (int rc = settle(c)) return rc;
  if (c->xch.comm || c->world > 1) return GBP_OK;               // sharded iterations run from direct launches by default
  if (c->persist.ok) return GBP_OK;                         // multi-iteration bursts run inside k_persist: nothing to capture
  if (ensure_graph(c, sweep_args(c))) (void)hipGraphUpload(c->graph.exec, c->stream);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GBP_OK;
}
