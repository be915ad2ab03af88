// gbp_api_devio.cpp — the four programs that move state, for a caller whose arrays live on the ctx's GPU (include/gbp_mi355x.h,
// "Device-resident arrays"): gbp_upload / gbp_read / gbp_read_priors / gbp_new_keyframe land here when their struct holds device
// pointers (gbp_api_ctx.cpp: struct_kind).  Same targets and same bits as the host-pointer forms, which stage through pinned memory:
// here kernels read and write the caller's file-order arrays directly (kernels/gbp_state_io.hip, "device-resident caller arrays"), everything
// is queued on the ctx's stream and nothing waits for it.
#include "gbp_ctx.hpp"

using namespace gbp;
using namespace gbp::api;

namespace {

// lay.pos_edge on the device: built by the first device-pointer call of a ctx (the one call of these that blocks: a staged copy)
int need_pos_edge(gbp_ctx* c) {
  if (c->arr.d_pos_edge.p) return GBP_OK;
  if (int rc = dev_alloc(c, c->arr.d_pos_edge, (size_t)c->Ep * 4)) return rc;
  H2D up;
  if (int rc = up.begin(c, (size_t)c->Ep * 4, 1)) return rc;
  if (int rc = up.put(c->arr.d_pos_edge.p, c->lay.pos_edge.data(), (size_t)c->Ep * 4)) return rc;
  return up.end();
}

// Launches of the persistent kernel that are still unvalidated are waited for first, as before every other kind of device work
// (settle: free when none is in flight).  A ctx that left the persistent path after a recovered time-out gets its fresh start.
// Otherwise the reset gbp_upload makes (persist_reset: barrier words and persist.epoch_base back to zero, behind a stream
// synchronisation) is not needed: the two are only ever used as a pair — the kernel waits for epoch_base + its own arrivals on a
// counter that keeps counting across launches, wrap-safe — the tags of the tagged records come from persist.seq, which no upload
// resets: it counts on for the life of the ctx, skipping the numbers that would make tag 0 or launch number 0, and the launch that
// begins a new period of 2^19 - 1 tags clears the shadows first (gbp_persist_seq.hpp), so an upload has nothing to do for them — and
// with the log empty and the status word zero there is nothing else persist_reset would change.  Leaving it out is what keeps
// this call from blocking.
int settle_for_upload(gbp_ctx* c) {
  if (int rc = settle(c)) return rc;
  if (c->persist.status.host && (c->persist.ok != c->persist.eligible || persist_failed_seq(c) != 0u)) return persist_reset(c);
  return GBP_OK;
}

void seg(RecSegs& t, const void* caller, void* rec, size_t records, uint32_t w, uint32_t stride, uint32_t off) {
  if (!caller || records == 0) return;
  const int i = t.n++;
  t.caller[i] = const_cast<void*>(caller); t.rec[i] = rec;
  t.total[i] = (uint32_t)(records * w); t.w[i] = w; t.stride[i] = stride; t.off[i] = off;
}

}  // namespace

namespace gbp {
namespace api {

// WRITE_PROG from device arrays: what gbp_upload does, with k_upload_dev + k_rec_copy in place of the host gather, the staging
// buffer and k_upload_scatter.  Not blocking.  mu / oldmu: see the header (the caller's duty; read only with per_factor_mu).
int devio_upload(gbp_ctx* c, const gbp_state_in* in) {
  if (int rc = settle_for_upload(c)) return rc;
  if (int rc = need_pos_edge(c)) return rc;
  c->arr.active_host.assign(c->Ep, 0);
  c->arr.active_host_stale = true;
  for (DevBuf* b : {&c->arr.fac, &c->arr.cmsg, &c->arr.rowp, &c->arr.local, &c->arr.camb, &c->arr.lmkb, &c->arr.hmu_c, &c->arr.hmu_l, &c->arr.clin, &c->arr.camp, &c->arr.lmkp, &c->arr.cscale, &c->arr.cwf, &c->arr.lscale, &c->arr.lwf})
    HIPCHK(c, hipMemsetAsync(b->p, 0, b->bytes, c->stream));
  c->arr.cmsg_zero = true;      // (the fill of CMSG: every record kCmsgZero)
  UploadDev a{};
  a.pos_edge = P<uint32_t>(c->arr.d_pos_edge);
  a.damping = in->damping; a.damping_count = in->damping_count; a.active_flag = in->active_flag;
  a.measurements = in->measurements; a.meas_variances = in->meas_variances;
  a.om = in->oldmu ? in->oldmu : in->mu;
  a.lmsg = P<float4>(c->arr.lmsg); a.fs = factor_state(c); a.fac = P<float4>(c->arr.fac);
  a.mu = c->hoist ? nullptr : P<float4>(c->arr.mu);
  a.n = c->Ep;
  launch_upload_dev(a, c->stream);
  HIPCHK(c, hipGetLastError());
  RecSegs t{};
  seg(t, in->cam_priors_eta, c->arr.camp.p, c->C, 6, kCamRec, 0);
  seg(t, in->cam_priors_lambda, c->arr.camp.p, c->C, 36, kCamRec, 8);
  seg(t, in->lmk_priors_eta, c->arr.lmkp.p, c->L, 3, 16, 0);
  seg(t, in->lmk_priors_lambda, c->arr.lmkp.p, c->L, 9, 16, 4);
  seg(t, in->cam_scaling, c->arr.cscale.p, c->C, 1, 1, 0);
  seg(t, in->cam_weaken_flag, c->arr.cwf.p, c->C, 1, 1, 0);
  seg(t, in->lmk_scaling, c->arr.lscale.p, c->L, 1, 1, 0);
  seg(t, in->lmk_weaken_flag, c->arr.lwf.p, c->L, 1, 1, 0);
  launch_rec_copy(t, true, c->stream);
  HIPCHK(c, hipGetLastError());
  if (int rc = zero_exchange(c)) return rc;      // (as gbp_upload)
  c->uploaded = true;
  c->beliefs_valid = false;
  return GBP_OK;
}

// READ_PROG into device arrays.  Not blocking: the arrays are valid for work queued behind the call on the ctx's stream, or after gbp_sync.
int devio_read(gbp_ctx* c, gbp_state_out* o) {
  if (int rc = settle(c)) return rc;
  if (o->damping || o->damping_count || o->robust_flag) {
    if (int rc = need_pos_edge(c)) return rc;
    launch_read_state_dev(P<uint32_t>(c->arr.d_pos_edge), factor_state(c), o->damping, o->damping_count, o->robust_flag, c->Ep, c->stream);
    HIPCHK(c, hipGetLastError());
  }
  RecSegs t{};
  seg(t, o->cam_beliefs_eta, c->arr.camb.p, c->C, 6, kCamRec, 0);
  seg(t, o->cam_beliefs_lambda, c->arr.camb.p, c->C, 36, kCamRec, 8);
  seg(t, o->lmk_beliefs_eta, c->arr.lmkb.p, c->L, 3, 16, 0);
  seg(t, o->lmk_beliefs_lambda, c->arr.lmkb.p, c->L, 9, 16, 4);
  launch_rec_copy(t, false, c->stream);
  HIPCHK(c, hipGetLastError());
  return GBP_OK;
}

// READ_PRIORS into device arrays, the same way
int devio_read_priors(gbp_ctx* c, gbp_priors_out* o) {
  if (int rc = settle(c)) return rc;
  RecSegs t{};
  seg(t, o->cam_priors_eta, c->arr.camp.p, c->C, 6, kCamRec, 0);
  seg(t, o->cam_priors_lambda, c->arr.camp.p, c->C, 36, kCamRec, 8);
  seg(t, o->lmk_priors_eta, c->arr.lmkp.p, c->L, 3, 16, 0);
  seg(t, o->lmk_priors_lambda, c->arr.lmkp.p, c->L, 9, 16, 4);
  launch_rec_copy(t, false, c->stream);
  HIPCHK(c, hipGetLastError());
  return GBP_OK;
}

// NEW_KEYFRAME from device arrays: the per-factor scalars edited in place (k_keyframe_state_dev), priors (both halves of a pair
// given, as on the host path) and weaken flags copied, then the prior-only belief refresh.  Not blocking.  The guard of the host
// path against a factor that is activated with a count that lets it relinearise on its first sweep (hoisted means) would need the
// counts on the host: the caller's duty here (the header says so).
int devio_new_keyframe(gbp_ctx* c, const gbp_kf_update* u) {
  if (int rc = settle(c)) return rc;
  if (u->damping_count || u->active_flag) {
    if (int rc = need_pos_edge(c)) return rc;
    launch_keyframe_state_dev(P<uint32_t>(c->arr.d_pos_edge), P<int>(c->arr.fst_packed), u->damping_count, u->active_flag, c->Ep, c->stream);
    HIPCHK(c, hipGetLastError());
    if (u->active_flag) c->arr.active_host_stale = true;
  }
  RecSegs t{};
  if (u->cam_priors_eta && u->cam_priors_lambda) {
    HIPCHK(c, hipMemsetAsync(c->arr.camp.p, 0, c->arr.camp.bytes, c->stream));      // (the pads of a record: pack_cam writes zeros)
    seg(t, u->cam_priors_eta, c->arr.camp.p, c->C, 6, kCamRec, 0);
    seg(t, u->cam_priors_lambda, c->arr.camp.p, c->C, 36, kCamRec, 8);
  }
  if (u->lmk_priors_eta && u->lmk_priors_lambda) {
    HIPCHK(c, hipMemsetAsync(c->arr.lmkp.p, 0, c->arr.lmkp.bytes, c->stream));
    seg(t, u->lmk_priors_eta, c->arr.lmkp.p, c->L, 3, 16, 0);
    seg(t, u->lmk_priors_lambda, c->arr.lmkp.p, c->L, 9, 16, 4);
  }
  seg(t, u->cam_weaken_flag, c->arr.cwf.p, c->C, 1, 1, 0);
  seg(t, u->lmk_weaken_flag, c->arr.lwf.p, c->L, 1, 1, 0);
  launch_rec_copy(t, true, c->stream);
  HIPCHK(c, hipGetLastError());
  return refresh_beliefs_from_partials(c, false);
}

// the host shadow of the active flags (hoist guard of the host-pointer gbp_new_keyframe) read back from the state plane; blocking
int devio_refresh_active_shadow(gbp_ctx* c) {
  std::vector<int32_t> packed(c->Ep);
  D2H down;
  if (int rc = down.begin(c, (size_t)c->Ep * 4, 1)) return rc;
  if (down.up.direct) HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = down.get(packed.data(), c->arr.fst_packed.p, (size_t)c->Ep * 4)) return rc;
  if (int rc = down.end()) return rc;
  c->arr.active_host.assign(c->Ep, 0);
  for (size_t p = 0; p < c->Ep; ++p) c->arr.active_host[p] = ((uint32_t)packed[p] & (kFlagActive | kFlagPad)) == kFlagActive;
  c->arr.active_host_stale = false;
  return GBP_OK;
}

}  // namespace api
}  // namespace gbp
