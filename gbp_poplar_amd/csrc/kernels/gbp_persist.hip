// kernels/gbp_persist.hip — k_persist_flow, the co-residency probe, the grid and placement of a persistent launch and its
// launcher.
#pragma once
#include "gbp_tile.hpp"
#include "gbp_vertex.hpp"
#include "gbp_metric_math.hpp"
#include "gbp_persist_support.hpp"
#ifdef GBP_BUILD_TEST_HOOKS
#include "../hooks/gbp_persist_barrier.hip"      // k_persist<EV>: the barrier kernel of rounds 3-4 (reference of the tests, A/B runs) — launch_persist names it
#endif

namespace gbp {
using namespace gbpdev;

// =================================================================================================
// k_persist_flow: k_persist without device-wide barriers (PersistFlow in gbp_kernels.h).  Same roles, same per-lane arithmetic in
// the same order — bit-identical results — but every hand-off is a dependency on DATA: a consumer re-loads the tagged records it
// needs until they carry the iteration it waits for.  Why the two halves suffice: a tile wave overwrites its records of iteration
// it when it produces those of it + 2, for which it needed the beliefs of it + 1 of ALL of its variables, whose owners produced them
// after reading the tile's records of it + 1 — after those of it; and the other way round.  Launches without the metric only.
// A wait is bounded like k_persist's barriers (1.5 s, abort word, *status): the wave then returns and the host restores the
// snapshot and replays on the two-kernel path.
// =================================================================================================
// EV: the launch carries the metric (A.ev, as in k_persist<true>): the metric means of iteration k are tagged records too (F.emc,
// F.eml), the tile waves evaluate their residuals one iteration later behind their belief-phase role, the health counters are
// per-iteration device words that block 0 hands to the host's slots behind the ONE barrier such a launch ends with.
template <bool EV, bool VER = false>
__global__ __launch_bounds__(256) void k_persist_flow(const PersistArgs A) {
  using Xw = XwBufT<VER>;
  const bool ev_on = EV && A.ev.on != 0;
  const SweepArgs& a = A.s;
  const BeliefArgs& b = A.b;
  const PersistFlow& F = A.f;
  const uint32_t wib = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (__hip_atomic_load(A.sync + 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;      // (see k_persist)
  uint32_t bid, nblk;
  if (!persist_place(A, bid, nblk)) return;
  const uint32_t w = bid * 4 + wib;
  __shared__ float4 lm_stage[4][64 * 4];
  __shared__ float sh[4][48];
  float4* stage = lm_stage[wib];
  const uint32_t mir = VER ? F.mirror4 : 0u;
  unsigned long long* const verr = VER ? F.verify_errors : nullptr;
  // ONE descriptor (the shadows are one allocation, F.lmsg its start) + a scalar byte offset per array
  const auto off_of = [&](const float4* q) { return (uint32_t)(reinterpret_cast<const char*>(q) - reinterpret_cast<const char*>(F.lmsg)); };
  const Xw S_lmsg(F.lmsg, mir, verr), S_rowp(F.lmsg, mir, verr, off_of(F.rowp)), S_camb(F.lmsg, mir, verr, off_of(F.camb)),
      S_cmu(F.lmsg, mir, verr, off_of(F.cmu)), S_clin(F.lmsg, mir, verr, off_of(F.clin)), S_lmkb(F.lmsg, mir, verr, off_of(F.lmkb)),
      S_lmu(F.lmsg, mir, verr, off_of(F.lmu));
  const Xw S_emc(F.lmsg, mir, verr, off_of(F.emc)), S_eml(F.lmsg, mir, verr, off_of(F.eml));
  const uint32_t nC = b.n_cams, nL = b.n_lmks, Ep = A.n_tiles * 64u, n_rows = A.n_tiles * 4u;

  // ---- phase-A role: sweep tile w; the factor's potential and both of its messages stay in registers ----
  const bool has_tile = w < A.n_tiles;
  const uint32_t tile = has_tile ? w : 0u, p = tile * 64 + lane;
  const uint32_t lm_tile4 = tile * 256u;
  float fac[56], cm[28], lm[16];
  uint32_t cam_i = 0, lmk_i = 0;
  bool fac_dirty = false;
  if (has_tile) {
    cam_i = a.row_cam[p >> 4];
    lmk_i = a.lmk_idx[p];
    tile_regs_load(a, tile, lane, stage, [&](uint32_t i4) { return a.lmsg[i4]; }, fac, cm, lm);
  }
  // A pad position names camera pos_cam (its row's, or camera 0 in a row of pads only) and landmark 0 without being a factor of either:
  // no owner waits for it, so an owner is not held back until the pad lane has read a record.  A landmark group without a factor (waits
  // for nothing) or a camera ahead of an all-pad tile then overwrites the half the pad lane polls, and the lane would wait for a tag
  // that is gone until the time-out.  A pad is never active: factor_update and the metric read none of these records for it, so a pad
  // lane takes whatever its loads return and waits for nothing.
  const bool pad_lane = has_tile && ((uint32_t)__float_as_int(lm[13]) & kFlagPad) != 0u;
  float K[9];
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) K[i] = a.K[i];

  // ---- phase-B role: camera v, or landmarks 16 (v - C) .. + 15 (4 lanes each); numbered across the workgroups as in k_persist ----
  // (EV: waves [C + G, 2C + G), where the grid has them, take the METRIC mean of camera v - (C + G): k_persist's metric roles)
  // A.separate: the roles are dealt to the waves WITHOUT a tile first (whole workgroups behind the tiles', one role per workgroup
  // before a second one), cameras, then metric means, then landmark groups: a wave that owns a camera then sweeps no tile, and
  // nothing it does behind its publication (the metric's residuals, the fp64 solves of a metric mean) delays a sweep that every
  // camera waits for.  v below is the role in k_persist's numbering either way.
  const uint32_t v_met0 = nC + A.n_lmk_groups;
  const uint32_t v = persist_role(bid, wib, nblk, A.n_tiles, nC, A.n_lmk_groups, A.n_met, A.separate);
  const bool cam_wave = v < nC;
  const bool lmk_wave = !cam_wave && (v - nC) < A.n_lmk_groups;
  const bool met_wave = ev_on && v >= v_met0 && v - v_met0 < nC;
  const bool cam_has_met_wave = cam_wave && ev_on && (A.separate ? A.n_met != 0u : v_met0 + v < nblk * 4u);
  const uint32_t camv = met_wave ? v - v_met0 : v;
  const uint32_t cj = lane;
  const bool cam_live = (cam_wave || met_wave) && cj < (uint32_t)kCamRec;
  uint32_t r0 = 0, r1 = 0;
  float cam_prior_j = 0.f;
  float4 cam_cur0 = make_float4(0.f, 0.f, 0.f, 0.f), cam_cur1 = cam_cur0;
  // where element cj of a row's 44-float record sits in the row's tagged record (row16_sums_store: lane q of the row's last quad holds
  // the groups q, q + 4, q + 8 = twelve floats = four tagged records)
  const uint32_t rg = cj >> 2, rn = 4u * (rg >> 2) + (cj & 3u);
  const uint32_t row_f4 = 4u * (rg & 3u) + rn / 3u, row_c = rn % 3u;
  const uint32_t cb_s0 = flow_camb_src(3u * lane), cb_s1 = flow_camb_src(3u * lane + 1u), cb_s2 = flow_camb_src(3u * lane + 2u);   // lanes 0..9
  if (cam_wave || met_wave) {
    r0 = b.cam_row_ptr[camv]; r1 = b.cam_row_ptr[camv + 1];
    if (cam_live) cam_prior_j = b.cam_prior[(size_t)camv * kCamRec + cj];
  }
  if (cam_wave) { cam_cur0 = a.cam_mu[(size_t)v * 4]; cam_cur1 = a.cam_mu[(size_t)v * 4 + 1]; }
  // WEAKEN_PRIORS inside the launch (PersistArgs.w_first / w_steps2): every wave that holds a prior keeps its variable's flag and
  // scaling in registers and applies WeakenPriorVertex (gbp_codelets.cpp:176-197: a flag in 1 .. 5 scales the prior and counts down) in
  // front of the iterations the reference's loop weakens before; the owners write prior and flag back with the last iteration
  const bool weakens = A.w_steps2 != 0u;
  uint32_t wf = 0;              // the camera's / the landmark's weaken flag
  float wscale = 1.f;
  bool weakened = false;        // did this launch change this wave's prior?
  if (weakens && (cam_wave || met_wave)) { wf = b.cam_wflag[camv]; wscale = b.cam_scale[camv]; }
  const uint32_t l = lmk_wave ? (v - nC) * 16 + (lane >> 2) : 0u, q4 = lane & 3;
  const bool lmk_live = lmk_wave && l < nL;
  uint4 ix = make_uint4(0u, 0u, 0u, 0u);
  float pr3[3] = {0.f, 0.f, 0.f};
  float4 lmk_cur = make_float4(0.f, 0.f, 0.f, 0.f);
  uint32_t lp0 = 0, lp1 = 0;
  const uint32_t l_e0 = q4 == 0u ? 0u : 4u + 3u * (q4 - 1u);      // first float of this lane's triple in the 16-float landmark record
  if (lmk_live) {
    ix = reinterpret_cast<const uint4*>(b.lmk_ix)[(size_t)l * 4 + q4];
    const float* pr = reinterpret_cast<const float*>(b.lmk_prior) + (size_t)l * 16 + l_e0;
    pr3[0] = pr[0]; pr3[1] = pr[1]; pr3[2] = pr[2];
    lmk_cur = a.lmk_mu[(size_t)l * 2];
    lp0 = b.lmk_ptr[l]; lp1 = b.lmk_ptr[l + 1];
    if (weakens) { wf = b.lmk_wflag[l]; wscale = b.lmk_scale[l]; }
  }
  const uint32_t deg = (uint32_t)__shfl((int)ix.x, 0, 4);
  uint32_t pos[32];
  GBP_UNROLL
  for (int k = 0; k < 15; ++k) {
    const uint32_t e = ((k + 1) & 3) == 0 ? ix.x : ((k + 1) & 3) == 1 ? ix.y : ((k + 1) & 3) == 2 ? ix.z : ix.w;
    pos[k] = (uint32_t)__shfl((int)e, (k + 1) >> 2, 4);
  }
  GBP_UNROLL
  for (int k = 0; k < 15; ++k) {
    const uint32_t p2 = b.lmk_fpos[lp0 + (15u + (uint32_t)k < deg ? 15u + (uint32_t)k : 0u)];
    pos[15 + k] = (lmk_live && 15u + (uint32_t)k < deg) ? p2 : 0u;
  }

  // ---- prologue: the beliefs this launch starts from, published as "iteration -1" (half 1, tag0) ----
  if (cam_wave) {
    const float* rec = b.camb + (size_t)v * kCamRec;
    if (lane < kFlowCam4) S_camb.st4((nC + v) * kFlowCam4 + lane, flow_rec(rec[cb_s0], rec[cb_s1], rec[cb_s2], F.tag0));
    if (lane == 0) {
      S_cmu.st4((nC + v) * 2u, flow_rec(cam_cur0.x, cam_cur0.y, cam_cur0.z, F.tag0));
      S_cmu.st4((nC + v) * 2u + 1u, flow_rec(cam_cur0.w, cam_cur1.x, cam_cur1.y, F.tag0));
      const float* cl = reinterpret_cast<const float*>(a.cam_lin + (size_t)v * kCamLin4);
      GBP_UNROLL
      for (int g = 0; g < (int)kFlowClin4; ++g)
        S_clin.st4((nC + v) * kFlowClin4 + (uint32_t)g, flow_rec(cl[3 * g], cl[3 * g + 1], g < 6 ? cl[3 * g + 2] : 0.f, F.tag0));
    }
  } else if (lmk_live) {
    const float* rec = reinterpret_cast<const float*>(a.lmkb) + (size_t)l * 16;
    S_lmkb.st4((nL + l) * kFlowLmk4 + q4, flow_rec(rec[l_e0], rec[l_e0 + 1u], rec[l_e0 + 2u], F.tag0));
    if (q4 == 0) {
      S_lmkb.st4((nL + l) * kFlowLmk4 + 4u, flow_rec(rec[3], rec[13], rec[14], F.tag0));
      S_lmu.st4(nL + l, flow_rec(lmk_cur.x, lmk_cur.y, lmk_cur.z, F.tag0));
    }
  }

  // ---- the metric (EV): per-iteration health words in device memory (zero on entry and on exit), the tile waves' partial sums in the
  // host's slots exactly as k_persist<true> leaves them ----
  auto health_of = [&](uint32_t kk) -> unsigned long long* { return A.ev.each ? F.health_iter + 2u * kk : A.ev.health; };
  // (the rotation of the camera's metric mean — eigenso3exp, a function of the camera alone — comes with the mean's record: computed once
  // by the mean's owner instead of once per factor, the same operations on the same operands, as in the two-kernel path's EvalRide)
  auto metric = [&](uint32_t kk, int packed, const float (&R)[9], const float (&t)[3], const float (&lmu)[3]) {
    double s_norm = 0, s_half = 0;
    const uint32_t flags = (uint32_t)packed & 7u;
    if (!(flags & kFlagPad) && (flags & kFlagActive)) eval_residual(R, t, lmu, fac[54], fac[55], a.K, s_norm, s_half);
    eval_wave_record(A.ev.slots + (size_t)(A.ev.each ? kk : 0u) * A.ev.stride + 1 + w, lane, packed, A.ev.num_undamped, s_norm, s_half);
  };
  // the tile wave's share of metric kk (means of iteration kk: half kk & 1, tag0 + kk + 1): c0 / c1 / l0 were loaded early, re-loaded here
  // only if they had not arrived then
  auto metric_of = [&](uint32_t kk, int packed, float4 (&c)[4], float4 l0) -> bool {
    const unsigned tg = F.tag0 + kk + 1u;
    const uint32_t ec = ((kk & 1u) * nC + cam_i) * 4u, el = (kk & 1u) * nL + lmk_i;
    if (!__all(pad_lane || (flow_is(c[0], tg) && flow_is(c[1], tg) && flow_is(c[2], tg) && flow_is(c[3], tg) && flow_is(l0, tg)))) {
      if (!flow_wait([&]() {
            GBP_UNROLL
            for (int g = 0; g < 4; ++g) c[g] = S_emc.ld4(ec + (uint32_t)g);
            l0 = S_eml.ld4(el);
            return pad_lane || (flow_is(c[0], tg) && flow_is(c[1], tg) && flow_is(c[2], tg) && flow_is(c[3], tg) && flow_is(l0, tg));
          }, A.sync, A.status, A.seq)) return false;
    }
    const float R[9] = {c[0].x, c[0].y, c[0].z, c[1].x, c[1].y, c[1].z, c[2].x, c[2].y, c[2].z};
    const float t[3] = {c[3].x, c[3].y, c[3].z}, lmu[3] = {l0.x, l0.y, l0.z};
    metric(kk, packed, R, t, lmu);
    return true;
  };
  auto publish_metric_mean = [&](uint32_t half, uint32_t cam, const float (&xm)[6], unsigned tag) {
    float R[9];
    eval_cam_rot(xm, R);
    GBP_UNROLL
    for (int g = 0; g < 3; ++g) S_emc.st4((half * nC + cam) * 4u + (uint32_t)g, flow_rec(R[3 * g], R[3 * g + 1], R[3 * g + 2], tag));
    S_emc.st4((half * nC + cam) * 4u + 3u, flow_rec(xm[0], xm[1], xm[2], tag));
  };

  for (int it = 0; it < A.n_iters; ++it) {
    const bool ev_means = ev_on && (A.ev.each || it + 1 == A.n_iters);     // this iteration's beliefs are evaluated
    const bool ev_prev = ev_on && A.ev.each && it > 0 && has_tile;          // this tile wave owes the residuals of iteration it - 1
    const int ev_packed = __float_as_int(lm[13]);      // the factor's state word as the sweep of iteration it - 1 left it
    const uint32_t h_in = ((uint32_t)it + 1u) & 1u, h_out = (uint32_t)it & 1u;
    const unsigned t_in = F.tag0 + (unsigned)it, t_out = F.tag0 + (unsigned)it + 1u;
    const bool last = it + 1 == A.n_iters;
    // WeakenPriorVertex in front of the NEXT iteration: the owners then publish the beliefs of the weakened priors (what WEAKEN_PRIORS'
    // belief refresh leaves: same messages, same order, the means against the one the last sweep used), the metric keeps this iteration's
    const bool weak_next = weakens && !last && (((A.w_first + (uint32_t)it) & 1u) == 0u) && (A.w_first + (uint32_t)it + 1u < A.w_steps2);
    // ================= phase A: the sweep of this wave's tile =================
    if (has_tile) {
      float4 c4[kFlowCam4], m4[2], q7[kFlowClin4], l5[kFlowLmk4], u4;
      const uint32_t cb0 = (h_in * nC + cam_i), lb0 = (h_in * nL + lmk_i);
      // probe: the records the two owners store last (the camera's belief behind its mean and CAM_LIN, the landmark's squared mean changes)
      if (!flow_wait([&]() { return pad_lane || (flow_is(S_camb.ld4(cb0 * kFlowCam4), t_in) && flow_is(S_lmkb.ld4(lb0 * kFlowLmk4 + 4u), t_in)); },
                     A.sync, A.status, A.seq)) return;
      if (!flow_wait([&]() {
            bool ok = true;
            GBP_UNROLL
            for (int g = 0; g < (int)kFlowCam4; ++g) c4[g] = S_camb.ld4(cb0 * kFlowCam4 + (uint32_t)g);
            m4[0] = S_cmu.ld4(cb0 * 2u); m4[1] = S_cmu.ld4(cb0 * 2u + 1u);
            GBP_UNROLL
            for (int g = 0; g < (int)kFlowClin4; ++g) q7[g] = S_clin.ld4(cb0 * kFlowClin4 + (uint32_t)g);
            GBP_UNROLL
            for (int g = 0; g < (int)kFlowLmk4; ++g) l5[g] = S_lmkb.ld4(lb0 * kFlowLmk4 + (uint32_t)g);
            u4 = S_lmu.ld4(lb0);
            GBP_UNROLL
            for (int g = 0; g < (int)kFlowCam4; ++g) ok = ok && flow_is(c4[g], t_in);
            ok = ok && flow_is(m4[0], t_in) && flow_is(m4[1], t_in);
            GBP_UNROLL
            for (int g = 0; g < (int)kFlowClin4; ++g) ok = ok && flow_is(q7[g], t_in);
            GBP_UNROLL
            for (int g = 0; g < (int)kFlowLmk4; ++g) ok = ok && flow_is(l5[g], t_in);
            return pad_lane || (ok && flow_is(u4, t_in));
          }, A.sync, A.status, A.seq)) return;
      float cb[44], lb[16], mu[12];
      {
        float pl[30];
        GBP_UNROLL
        for (int g = 0; g < (int)kFlowCam4; ++g) { pl[3 * g] = c4[g].x; pl[3 * g + 1] = c4[g].y; pl[3 * g + 2] = c4[g].z; }
        GBP_UNROLL
        for (int i = 0; i < 44; ++i) cb[i] = 0.f;
        GBP_UNROLL
        for (int i = 0; i < 7; ++i) cb[i] = pl[i];
        GBP_UNROLL
        for (int i = 0; i < 6; ++i) {
          GBP_UNROLL
          for (int j = 0; j <= i; ++j) cb[8 + i * 6 + j] = pl[7 + tri(i, j)];
        }
      }
      lb[0] = l5[0].x; lb[1] = l5[0].y; lb[2] = l5[0].z;
      GBP_UNROLL
      for (int g = 0; g < 3; ++g) { lb[4 + 3 * g] = l5[1 + g].x; lb[5 + 3 * g] = l5[1 + g].y; lb[6 + 3 * g] = l5[1 + g].z; }
      lb[3] = l5[4].x; lb[13] = l5[4].y; lb[14] = l5[4].z; lb[15] = 0.f;
      float damping = lm[3];
      const int packed = __float_as_int(lm[13]);
      int count = packed >> 3;
      uint32_t flags = (uint32_t)packed & 7u;
      const float var = lm[14];
      const bool active = (flags & kFlagActive) != 0;
      float oc_eta[6], oc_lam[36], bi[9], ol[16];
      bool relin;
      factor_update<true>(fac, cm, mu, lm, cb, lb, K, a.hp, damping, count, flags, var, active, oc_eta, oc_lam, bi, ol, relin,
                             [&](float (&x0c)[6], float (&x0l)[3], CamLin& cl, float&) {
                               x0c[0] = m4[0].x; x0c[1] = m4[0].y; x0c[2] = m4[0].z; x0c[3] = m4[1].x; x0c[4] = m4[1].y; x0c[5] = m4[1].z;
                               x0l[0] = u4.x; x0l[1] = u4.y; x0l[2] = u4.z;
                               float f[21];
                               GBP_UNROLL
                               for (int g = 0; g < (int)kFlowClin4; ++g) { f[3 * g] = q7[g].x; f[3 * g + 1] = q7[g].y; f[3 * g + 2] = q7[g].z; }
                               float4 clq[kCamLin4];
                               GBP_UNROLL
                               for (int g = 0; g < kCamLin4; ++g) clq[g] = make_float4(f[4 * g], f[4 * g + 1], f[4 * g + 2], f[4 * g + 3]);
                               cam_lin_unpack(clq, cl);
                             });
      fac_dirty = fac_dirty || (active && relin);
      tile_regs_refresh(ol, oc_eta, oc_lam, damping, count, flags, var, lm, cm);
      if (last) tile_cmsg_store(a, tile, lane, oc_eta, bi, active);
      // the tagged landmark messages: eta | Lambda row 0 | row 1 | row 2, through the LDS transpose of k_sweep (coalesced stores)
      lm_tile_out(stage, lane,
                  [&](uint32_t q) { return q == 0u ? flow_rec(ol[0], ol[1], ol[2], t_out) : flow_rec(ol[1 + 3 * q], ol[2 + 3 * q], ol[3 + 3 * q], t_out); },
                  [&](uint32_t k, float4 v) { S_lmsg.st4(h_out * Ep * 4u + lm_tile4 + k * 64u + lane, v); });
      {  // camera half of the belief reduction: per-row tree sums (row16_sums_store), the holder's twelve floats as four tagged records
        float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0, g2 = g0;
        row16_sums_store(oc_eta, oc_lam, lane, [&](uint32_t g, float4 x) {
          const uint32_t j = g >> 2;
          if (j == 0u) g0 = x; else if (j == 1u) g1 = x; else g2 = x;
          if (last) a.rowp[(size_t)(p >> 4) * kCamRec4 + g] = x;
        });
        if ((lane & 12u) == 12u) {
          const uint32_t q = lane & 3u, rp = (h_out * n_rows + (p >> 4)) * kFlowRow4 + 4u * q;
          S_rowp.st4(rp, flow_rec(g0.x, g0.y, g0.z, t_out));
          S_rowp.st4(rp + 1u, flow_rec(g0.w, g1.x, g1.y, t_out));
          S_rowp.st4(rp + 2u, flow_rec(g1.z, g1.w, g2.x, t_out));
          if (q < 3u) S_rowp.st4(rp + 3u, flow_rec(g2.y, g2.z, g2.w, t_out));
        }
      }
      if (last)   // the ordinary LMSG tile, as k_sweep leaves it (the state planes: tile_regs_store)
        lmsg_tile_out(stage, lane, ol, [&](uint32_t k, float4 v) { a.lmsg[tile * (uint32_t)(64 * kLmsgG) + k * 64u + lane] = v; });
    }

    // ================= phase B: the belief update (arithmetic of k_beliefs, roll = 1) =================
    float4 ev_c[4], ev_l0 = make_float4(0.f, 0.f, 0.f, 0.f);
    GBP_UNROLL
    for (int g = 0; g < 4; ++g) ev_c[g] = ev_l0;
    if (EV && ev_prev) {      // in flight with the role's own loads (measured: the residuals at the end of the phase, not behind the sweep)
      const uint32_t kk = (uint32_t)it - 1u;
      GBP_UNROLL
      for (int g = 0; g < 4; ++g) ev_c[g] = S_emc.ld4(((kk & 1u) * nC + cam_i) * 4u + (uint32_t)g);
      ev_l0 = S_eml.ld4((kk & 1u) * nL + lmk_i);
    }
    unsigned long long* const hw = EV ? health_of((uint32_t)it) : nullptr;
    if (cam_wave || (EV && met_wave && ev_means)) {
      float acc = 0.f;
      if (r1 > r0) {
        const uint32_t row4 = (h_out * n_rows + r0) * kFlowRow4 + row_f4;          // float4 index of this lane's element in row r0
        const uint32_t n = r1 - r0;
        // rows per round; rows of the first round.  (measured on the three sequences, round 5: 1 + 16 is as fast as or faster than 2 + 16,
        // 17 + 16, 9 + 8, 1 + 32 and everything in one round — k_persist's shape, for the same reason: registers)
        // (... and once the cameras had waves of their own, measured again: the instantiation with the metric is faster with two rounds for
        // up to 28 rows, 12 + 16 — fr1xyz 12.28 -> 11.94 us per iteration, fr1desk 12.47 -> 12.29, fr2robot2 11.45 -> 11.3; 4 + 24, 8 + 20,
        // 14 + 14 about the same — the plain one stays fastest with 1 + 16: 11.52 against 11.8 - 12.0)
        constexpr int RB = 16, RF = EV ? 12 : 1;
        uint32_t r = 0;
        {  // first round: rows 0 .. RF - 1 (unconditional; rows the camera does not have: out of range, no access)
          float4 x[RF];
          if (!flow_wait([&]() {
                bool ok = true;
                GBP_UNROLL
                for (int k = 0; k < RF; ++k) x[k] = S_rowp.ld4((uint32_t)k < n ? row4 + (uint32_t)k * kFlowRow4 : XwBuf::kNone4);
                GBP_UNROLL
                for (int k = 0; k < RF; ++k) ok = ok && ((uint32_t)k >= n || flow_is(x[k], t_out));
                return !cam_live || ok;
              }, A.sync, A.status, A.seq)) return;
          acc = flow_pick(x[0], row_c);
          GBP_UNROLL
          for (int k = 1; k < RF; ++k)
            if ((uint32_t)k < n) acc = acc + flow_pick(x[k], row_c);
          r = n < (uint32_t)RF ? n : (uint32_t)RF;
        }
        for (; r + RB <= n; r += RB) {
          float4 x[RB];
          if (!flow_wait([&]() {
                bool ok = true;
                GBP_UNROLL
                for (int k = 0; k < RB; ++k) x[k] = S_rowp.ld4(row4 + (r + (uint32_t)k) * kFlowRow4);
                GBP_UNROLL
                for (int k = 0; k < RB; ++k) ok = ok && flow_is(x[k], t_out);
                return !cam_live || ok;
              }, A.sync, A.status, A.seq)) return;
          GBP_UNROLL
          for (int k = 0; k < RB; ++k) acc = acc + flow_pick(x[k], row_c);
        }
        if (r < n) {  // tail (< RB rows): unconditional loads, the rows beyond the camera's out of range
          float4 x[RB];
          const uint32_t m = n - r;
          if (!flow_wait([&]() {
                bool ok = true;
                GBP_UNROLL
                for (int k = 0; k < RB; ++k) x[k] = S_rowp.ld4((uint32_t)k < m ? row4 + (r + (uint32_t)k) * kFlowRow4 : XwBuf::kNone4);
                GBP_UNROLL
                for (int k = 0; k < RB; ++k) ok = ok && ((uint32_t)k >= m || flow_is(x[k], t_out));
                return !cam_live || ok;
              }, A.sync, A.status, A.seq)) return;
          GBP_UNROLL
          for (int k = 0; k < RB; ++k)
            if ((uint32_t)k < m) acc = acc + flow_pick(x[k], row_c);
        }
      }
      if (cam_live) {
        if (last && cam_wave) b.cam_local[(size_t)v * kCamRec + cj] = acc;
        sh[wib][cj] = cam_prior_j + acc;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (EV && lane == 0 && !cam_wave) {   // metric role: what k_means computes for this camera, from the belief in LDS; then — published
        float xm[6];                        // first — the health check the camera wave would otherwise run on its critical lane
        solve_pivot<6>(sh[wib] + 8, 6, sh[wib], xm);
        publish_metric_mean(h_out, camv, xm, t_out);
        bool finite = true;
        GBP_UNROLL
        for (int i = 0; i < 6; ++i) finite &= (xm[i] - xm[i] == 0.f);
        if (!finite) atomicAdd(&hw[0], 1ull);
        if (!ldl_pivots_positive<6>(sh[wib] + 8, 6)) atomicAdd(&hw[1], 1ull);
      }
      float xm[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      bool pd = true;
      const bool ev_here = EV && ev_means && cam_wave && !cam_has_met_wave;     // no wave to spare for this camera's metric mean: solved here
      if (lane == 0 && ev_here) {      // ... from this iteration's belief, before a weakening replaces it below
        solve_pivot<6>(sh[wib] + 8, 6, sh[wib], xm);
        pd = ldl_pivots_positive<6>(sh[wib] + 8, 6);
      }
      if (weak_next) {      // WeakenPriorVertex on this camera's prior (every wave that holds a copy, the metric waves too)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (wf >= 1u && wf <= 5u) {
          if (cam_live) cam_prior_j *= wscale;
          wf -= 1u;
          weakened = true;
        }
        if (cam_live && cam_wave) sh[wib][cj] = cam_prior_j + acc;      // the belief the next sweep consumes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
      if (lane == 0 && cam_wave) {
        float cb[44], x0c[6];
        GBP_UNROLL
        for (int i = 0; i < 44; ++i) cb[i] = sh[wib][i];
        cam_mean(cb, x0c);
        const float used[6] = {cam_cur0.x, cam_cur0.y, cam_cur0.z, cam_cur0.w, cam_cur1.x, cam_cur1.y};
        const float S = cam_dmu2(used, x0c);
        if (last) { b.cam_mu[(size_t)v * 4 + 2] = cam_cur0; b.cam_mu[(size_t)v * 4 + 3] = cam_cur1; }
        cam_cur0 = make_float4(x0c[0], x0c[1], x0c[2], x0c[3]);
        cam_cur1 = make_float4(x0c[4], x0c[5], 0.f, 0.f);
        S_cmu.st4((h_out * nC + v) * 2u, flow_rec(x0c[0], x0c[1], x0c[2], t_out));
        S_cmu.st4((h_out * nC + v) * 2u + 1u, flow_rec(x0c[3], x0c[4], x0c[5], t_out));
        if (last) { b.cam_mu[(size_t)v * 4] = cam_cur0; b.cam_mu[(size_t)v * 4 + 1] = cam_cur1; }
        {
          CamLin cl;
          const float wv[3] = {x0c[3], x0c[4], x0c[5]};
          cam_lin(wv, cl);
          float4 q[kCamLin4];
          cam_lin_pack(cl, q);
          float f[21];
          GBP_UNROLL
          for (int g = 0; g < kCamLin4; ++g) { f[4 * g] = q[g].x; f[4 * g + 1] = q[g].y; f[4 * g + 2] = q[g].z; f[4 * g + 3] = q[g].w; }
          f[20] = 0.f;
          GBP_UNROLL
          for (int g = 0; g < (int)kFlowClin4; ++g)
            S_clin.st4((h_out * nC + v) * kFlowClin4 + (uint32_t)g, flow_rec(f[3 * g], f[3 * g + 1], f[3 * g + 2], t_out));
          if (last) {
            GBP_UNROLL
            for (int g = 0; g < kCamLin4; ++g) b.cam_lin[(size_t)v * kCamLin4 + g] = q[g];
          }
        }
        if (ev_here) {
          publish_metric_mean(h_out, v, xm, t_out);
          bool finite = true;
          GBP_UNROLL
          for (int i = 0; i < 6; ++i) finite &= (xm[i] - xm[i] == 0.f);
          if (!finite) atomicAdd(&hw[0], 1ull);
          if (!pd) atomicAdd(&hw[1], 1ull);
        }
        sh[wib][6] = S;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (cam_wave && lane < kFlowCam4) S_camb.st4((h_out * nC + v) * kFlowCam4 + lane, flow_rec(sh[wib][cb_s0], sh[wib][cb_s1], sh[wib][cb_s2], t_out));
      if (last && cam_live && cam_wave) b.camb[(size_t)v * kCamRec + cj] = sh[wib][cj];
      if (last && weakened && cam_wave) {
        if (cam_live) b.cam_prior_rw[(size_t)v * kCamRec + cj] = cam_prior_j;
        if (lane == 0) b.cam_wflag[v] = wf;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // sh[] is rewritten by the next iteration
      __builtin_amdgcn_wave_barrier();
    } else if (lmk_wave) {
      float a3[3] = {pr3[0], pr3[1], pr3[2]};
      const bool lw = weak_next && wf >= 1u && wf <= 5u;      // this landmark's prior is weakened in front of the next iteration
      if (lw) { pr3[0] *= wscale; pr3[1] *= wscale; pr3[2] *= wscale; }
      if (weak_next && wf >= 1u && wf <= 5u) { wf -= 1u; weakened = true; }
      float a3w[3] = {pr3[0], pr3[1], pr3[2]};                 // the same sums from the weakened prior (== a3 without a weakening)
      {
        float4 m[15], m2[15];
        const bool second = __any(deg > 15u);
        const uint32_t base = h_out * Ep;
        if (!flow_wait([&]() {
              bool ok = true;
              GBP_UNROLL
              for (int k = 0; k < 15; ++k) m[k] = S_lmsg.ld4((uint32_t)k < deg ? (base + pos[k]) * 4u + q4 : XwBuf::kNone4);
              if (second) {
                GBP_UNROLL
                for (int k = 0; k < 15; ++k) m2[k] = S_lmsg.ld4(15u + (uint32_t)k < deg ? (base + pos[15 + k]) * 4u + q4 : XwBuf::kNone4);
              }
              GBP_UNROLL
              for (int k = 0; k < 15; ++k) ok = ok && ((uint32_t)k >= deg || flow_is(m[k], t_out));
              if (second) {
                GBP_UNROLL
                for (int k = 0; k < 15; ++k) ok = ok && (15u + (uint32_t)k >= deg || flow_is(m2[k], t_out));
              }
              return !lmk_live || ok;
            }, A.sync, A.status, A.seq)) return;
        GBP_UNROLL
        for (int k = 0; k < 15; ++k)     // adds in slot order
          if ((uint32_t)k < deg) { a3[0] = a3[0] + m[k].x; a3[1] = a3[1] + m[k].y; a3[2] = a3[2] + m[k].z; }
        if (second) {
          GBP_UNROLL
          for (int k = 0; k < 15; ++k)
            if (15u + (uint32_t)k < deg) { a3[0] = a3[0] + m2[k].x; a3[1] = a3[1] + m2[k].y; a3[2] = a3[2] + m2[k].z; }
        }
        if (weak_next) {      // (wave-uniform)
          GBP_UNROLL
          for (int k = 0; k < 15; ++k)
            if ((uint32_t)k < deg) { a3w[0] = a3w[0] + m[k].x; a3w[1] = a3w[1] + m[k].y; a3w[2] = a3w[2] + m[k].z; }
          if (second) {
            GBP_UNROLL
            for (int k = 0; k < 15; ++k)
              if (15u + (uint32_t)k < deg) { a3w[0] = a3w[0] + m2[k].x; a3w[1] = a3w[1] + m2[k].y; a3w[2] = a3w[2] + m2[k].z; }
          }
        }
      }
      if (deg > 30u) {
        for (uint32_t s = lp0 + 30u; s < lp1; s += 8) {
          uint32_t ps[8];
          float4 m[8];
          const uint32_t nleft = lp1 - s;
          GBP_UNROLL
          for (int k = 0; k < 8; ++k) ps[k] = b.lmk_fpos[(uint32_t)k < nleft ? s + k : lp1 - 1u];     // clamped, unconditional
          if (!flow_wait([&]() {
                bool ok = true;
                GBP_UNROLL
                for (int k = 0; k < 8; ++k) m[k] = S_lmsg.ld4((h_out * Ep + ps[k]) * 4u + q4);
                GBP_UNROLL
                for (int k = 0; k < 8; ++k) ok = ok && flow_is(m[k], t_out);
                return ok;
              }, A.sync, A.status, A.seq)) return;
          GBP_UNROLL
          for (int k = 0; k < 8; ++k)
            if ((uint32_t)k < nleft) {
              a3[0] = a3[0] + m[k].x; a3[1] = a3[1] + m[k].y; a3[2] = a3[2] + m[k].z;
              a3w[0] = a3w[0] + m[k].x; a3w[1] = a3w[1] + m[k].y; a3w[2] = a3w[2] + m[k].z;
            }
        }
      }
      if (!weak_next) { a3w[0] = a3[0]; a3w[1] = a3[1]; a3w[2] = a3[2]; }      // (the tail loop above adds to both)
      // a3: this iteration's belief (the metric's); a3w: what the next sweep consumes
      if (lmk_live) S_lmkb.st4((h_out * nL + l) * kFlowLmk4 + q4, flow_rec(a3w[0], a3w[1], a3w[2], t_out));
      float rec[16];
      rec[0] = __shfl(a3w[0], 0, 4); rec[1] = __shfl(a3w[1], 0, 4); rec[2] = __shfl(a3w[2], 0, 4);
      GBP_UNROLL
      for (int g = 0; g < 3; ++g) {
        rec[4 + 3 * g] = __shfl(a3w[0], 1 + g, 4); rec[5 + 3 * g] = __shfl(a3w[1], 1 + g, 4); rec[6 + 3 * g] = __shfl(a3w[2], 1 + g, 4);
      }
      float recm[16];      // the record the metric mean is solved from
      GBP_UNROLL
      for (int g = 0; g < 16; ++g) recm[g] = rec[g];
      if (EV && weak_next) {
        recm[0] = __shfl(a3[0], 0, 4); recm[1] = __shfl(a3[1], 0, 4); recm[2] = __shfl(a3[2], 0, 4);
        GBP_UNROLL
        for (int g = 0; g < 3; ++g) {
          recm[4 + 3 * g] = __shfl(a3[0], 1 + g, 4); recm[5 + 3 * g] = __shfl(a3[1], 1 + g, 4); recm[6 + 3 * g] = __shfl(a3[2], 1 + g, 4);
        }
      }
      float u[3] = {0.f, 0.f, 0.f};
      if (lmk_live && q4 == 0) {
        float x0l[3];
        lmk_mean(rec, x0l);
        const float4 used = lmk_cur;
        lmk_dmu2(used, x0l, u);
        lmk_cur = make_float4(x0l[0], x0l[1], x0l[2], 0.f);
        S_lmu.st4(h_out * nL + l, flow_rec(x0l[0], x0l[1], x0l[2], t_out));
        S_lmkb.st4((h_out * nL + l) * kFlowLmk4 + 4u, flow_rec(u[0], u[1], u[2], t_out));
        if (last) { b.lmk_mu[(size_t)l * 2 + 1] = used; b.lmk_mu[(size_t)l * 2] = lmk_cur; }
        if (EV && ev_means) {   // metric mean of this landmark (k_means), from the belief record in registers
          float x[3];
          solve_pivot<3>(recm + 4, 3, recm, x);
          S_eml.st4(h_out * nL + l, flow_rec(x[0], x[1], x[2], t_out));
          bool finite = true;
          GBP_UNROLL
          for (int i = 0; i < 3; ++i) finite &= (x[i] - x[i] == 0.f);
          if (!finite) atomicAdd(&hw[0], 1ull);
          if (!ldl_pivots_positive<3>(recm + 4, 3)) atomicAdd(&hw[1], 1ull);
        }
      }
      if (last) {   // the ordinary LMKB record: float4 #q4 of [eta, u0 | Lambda 0..3 | 4..7 | 8, u1, u2, 0]
        rec[3] = __shfl(u[0], 0, 4); rec[13] = __shfl(u[1], 0, 4); rec[14] = __shfl(u[2], 0, 4); rec[15] = 0.f;
        float4 o;
        o.x = q4 == 0u ? rec[0] : q4 == 1u ? rec[4] : q4 == 2u ? rec[8] : rec[12];
        o.y = q4 == 0u ? rec[1] : q4 == 1u ? rec[5] : q4 == 2u ? rec[9] : rec[13];
        o.z = q4 == 0u ? rec[2] : q4 == 1u ? rec[6] : q4 == 2u ? rec[10] : rec[14];
        o.w = q4 == 0u ? rec[3] : q4 == 1u ? rec[7] : q4 == 2u ? rec[11] : rec[15];
        if (lmk_live) b.lmkb[(size_t)l * 4 + q4] = o;
        if (lmk_live && weakened) {
          float* pw = reinterpret_cast<float*>(b.lmk_prior_rw) + (size_t)l * 16 + l_e0;
          pw[0] = pr3[0]; pw[1] = pr3[1]; pw[2] = pr3[2];
          if (q4 == 0) b.lmk_wflag[l] = wf;
        }
      }
    }
    // the residuals of the PREVIOUS iteration, behind this wave's role (they delay nobody but this wave's next sweep)
    if (EV && ev_prev)
      if (!metric_of((uint32_t)it - 1u, ev_packed, ev_c, ev_l0)) return;
  }

  if (has_tile) tile_regs_store(a, tile, lane, fac, fac_dirty, lm);

  // ---- the metric of the last iteration; then the launch's ONE barrier: behind it every owner has counted and block 0 hands the
  // health words of every metric of the launch to the host's slots (and leaves them zero) ----
  if (EV && ev_on) {
    if (has_tile) {
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);      // (tag 0 is nobody's: the records are loaded in metric_of)
      float4 zc[4] = {z, z, z, z};
      if (!metric_of((uint32_t)A.n_iters - 1u, __float_as_int(lm[13]), zc, z)) return;
    }
    grid_sync(A.sync, A.epoch_base + nblk, A.status, A.seq);
    if (bid == 0 && (threadIdx.x == 0 || A.ev.each)) {
      if (A.ev.each) {
        for (int kk = (int)threadIdx.x; kk < A.n_iters; kk += 256) health_handoff(A.ev.slots + (size_t)kk * A.ev.stride, F.health_iter + 2 * kk);
      } else {
        health_handoff(A.ev.slots, A.ev.health);      // (both areas zero behind every metric: see k_eval)
        A.ev.health_next[0] = 0ull; A.ev.health_next[1] = 0ull;
      }
    }
  }
}

// The placement of k_persist without its work: the same grid, the same filler rule, three barriers.  gbp_create runs it
// once: if the working workgroups of this graph are NOT all resident at once on this device (another partition mode, another
// dispatch order than workgroup b -> XCD b mod 8) the barrier gives up, *status is raised and the ctx stays on the
// two-kernel path — found at creation, in milliseconds, not in the middle of a run.
__global__ __launch_bounds__(256) void k_persist_probe(unsigned* sync, unsigned* status, uint32_t spread, uint32_t n_work_blocks) {
  // same register footprint class as k_persist is not needed for the residency question that matters here (which CUs the
  // working workgroups may use); one workgroup per CU is enforced by asking for the LDS a CU can give only once
  extern __shared__ float probe_lds[];
  if (threadIdx.x == 0) probe_lds[0] = 0.f;
  if ((int)spread > 1 && blockIdx.x % spread) return;
  const uint32_t nblk = (int)spread > 1 ? gridDim.x / spread : gridDim.x;
  (void)n_work_blocks;
  for (unsigned e = 1; e <= 3; ++e) grid_sync(sync, e * nblk, status, 1u);
}

static int persist_spread(uint32_t nb) { return nb <= 64 ? 4 : nb <= 128 ? 2 : 1; }
#ifdef GBP_BUILD_EXPERIMENTS
int lab_persist_spread(int spread);
#endif

bool persist_probe(uint32_t n_tiles, uint32_t n_cams, uint32_t n_lmks, unsigned* sync, unsigned* status_dev, volatile unsigned* status_host,
                   bool cooperative, hipStream_t s) {
  const uint32_t nb = persist_grid(n_tiles, n_cams, n_lmks, true).nb;     // the larger of the two grids this graph is launched with
  const int spread = persist_spread(nb);
  if (hipMemsetAsync(sync, 0, kPersistSyncWords * sizeof(unsigned), s) != hipSuccess) return false;
  // 96 KiB of dynamic LDS per workgroup: at most ONE workgroup per CU (160 KiB), like k_persist's ~450 registers per lane
  // (profiles/r04_resources.md)
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_persist_probe), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess) return false;
  if (cooperative) {
    uint32_t sp = (uint32_t)spread, nwb = nb;
    void* args[] = {&sync, &status_dev, &sp, &nwb};
    if (hipLaunchCooperativeKernel(reinterpret_cast<const void*>(k_persist_probe), dim3(nb * (uint32_t)spread), dim3(256), args, 96 * 1024, s) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
  } else {
    hipLaunchKernelGGL(k_persist_probe, dim3(nb * (uint32_t)spread), dim3(256), 96 * 1024, s, sync, status_dev, (uint32_t)spread, nb);
  }
  if (hipStreamSynchronize(s) != hipSuccess) return false;
  const bool ok = *status_host == 0u;
  *status_host = 0u;
  return ok;
}

// Workgroups of a launch.  Role separation of k_persist_flow (PersistArgs.separate): the grid has a tile-less wave for every camera (and
// metric mean) as long as that still is at most one workgroup per CU (else roles and tiles share waves as in k_persist).  Measured
// (profiles/r05_persist_flow.md): with the metric after every iteration fr1xyz 13.1 -> 12.3 us per iteration, fr2robot2 12.3 -> 11.4,
// fr1desk unchanged; plain bursts 0.1 - 0.2 us faster.
PersistGrid persist_grid(uint32_t n_tiles, uint32_t n_cams, uint32_t n_lmks, bool with_metric) {
  const uint64_t cx = (uint64_t)n_cams * (with_metric ? 2u : 1u), g = ((uint64_t)n_lmks + 15) / 16;
  const uint32_t n_met = with_metric ? n_cams : 0u;
  // with the metric after every iteration the landmark owners move off the tile waves too where that fits (their fp64 metric solves,
  // and on graphs with landmarks of > 30 factors their extra rounds of loads, then delay no sweep: fr1desk 13.6 -> 12.5 us per
  // iteration, fr1xyz 12.3 -> 12.2, fr2robot2 11.4 -> 11.5; plain bursts do not gain from it)
  const uint64_t nb_full = ((uint64_t)n_tiles + cx + g + 3) / 4;
  const uint64_t nb_sep = with_metric && nb_full <= 256u ? nb_full : ((n_tiles + cx > cx + g ? n_tiles + cx : cx + g) + 3) / 4;
  if (nb_sep != 0u && nb_sep <= 256u) return PersistGrid{(uint32_t)nb_sep, 1u, n_met};
  // roles and tiles share waves
  const uint64_t waves_b = (uint64_t)n_cams + g;
  const uint64_t waves = waves_b > n_tiles ? waves_b : n_tiles;
  const uint32_t nb = (uint32_t)((waves + 3) / 4);
  if (!with_metric) return PersistGrid{nb, 0u, 0u};
  // a launch that carries the metric after EVERY iteration gets one more wave per camera for the metric roles: fr1xyz 52 -> 56
  // workgroups, fr2robot2 19 -> 24, fr1desk 61 -> 77 (every 2nd dispatch slot instead of every 4th; without barriers more workgroups cost
  // nothing: 16.3 -> 13.9 us per iteration with the metric, round 5) — as long as the larger grid still is one workgroup per CU.
  // Launches without the metric keep the smaller grid.
  const uint64_t waves_m = waves_b + n_cams > n_tiles ? waves_b + n_cams : n_tiles;
  const uint32_t nb_m = (uint32_t)((waves_m + 3) / 4);
  return PersistGrid{nb_m <= 256u ? nb_m : nb, 0u, 0u};
}
int persist_max_resident_blocks() {
  int dev = 0, per_cu = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (k_persist_flow<true>), 256, 0) != hipSuccess) return 0;
  return per_cu * prop.multiProcessorCount;
}
hipError_t launch_persist(PersistArgs A, bool cooperative, hipStream_t s) {
  A.n_lmk_groups = (A.b.n_lmks + 15) / 16;
  const PersistGrid pg = persist_grid(A.n_tiles, A.b.n_cams, A.b.n_lmks, A.ev.on != 0 && A.ev.each != 0);   // (one final metric: not worth 4 more workgroups in every barrier)
  const uint32_t nb = pg.nb;
  // Placement: the grid is 4x the work and only every 4th workgroup works (the fillers leave at once).  Measured
  // (profiles/persist_placement.py, profiles/r03_small_graphs.md): with the working workgroups in consecutive dispatch slots a
  // few of them — always all four waves of a workgroup, on a CU next to another working CU — run their fp64-heavy sections
  // 2-2.7x slower and set the barrier-to-barrier time; every 2nd or 4th slot removes those outliers (fr1xyz 22.0 -> 19.3 us
  // per iteration in the traced build), every 3rd does not.
  // Workgroup b runs on XCD b % 8 (round-robin dispatch), so every spread-th workgroup lands on 8 / spread XCDs of 32 CUs:
  // the working workgroups stay co-resident (one per CU: 256 VGPRs + 160-215 AGPRs per lane, profiles/r04_resources.md) only while nb <= 32 * 8 / spread.
  int spread = persist_spread(nb);
#ifdef GBP_BUILD_EXPERIMENTS
  spread = lab_persist_spread(spread);      // placement studies / the forced time-out of tests/test_gpu_experiments.py (GBP_PERSIST_SPREAD)
#endif
  A.n_work_blocks = nb;
  A.spread = (uint32_t)spread;
  A.separate = pg.separate;
  A.n_met = pg.n_met;
  const uint32_t grid = spread > 1 ? nb * (uint32_t)spread : spread < -1 ? ((nb + 7) / 8) * (uint32_t)(-spread) * 8 : nb;
  const bool flow = A.f.lmsg != nullptr;      // hand-offs through tagged records (PersistFlow); without: the barrier kernel of the test-hooks build
  const void* f = A.ev.on ? reinterpret_cast<const void*>(k_persist_flow<true>) : reinterpret_cast<const void*>(k_persist_flow<false>);
#ifdef GBP_BUILD_TEST_HOOKS
  if (!flow) f = A.ev.on ? reinterpret_cast<const void*>(k_persist<true>) : reinterpret_cast<const void*>(k_persist<false>);
  else if (A.f.mirror4 != 0u)      // gbp_debug_persist_verify: every record published twice and compared by its consumers
    f = A.ev.on ? reinterpret_cast<const void*>(k_persist_flow<true, true>) : reinterpret_cast<const void*>(k_persist_flow<false, true>);
#else
  if (!flow) return hipErrorInvalidValue;
#endif
  void* args[] = {&A};
  if (cooperative) return hipLaunchCooperativeKernel(f, dim3(grid), dim3(256), args, 0, s);
  (void)hipLaunchKernel(f, dim3(grid), dim3(256), args, 0, s);
  return hipGetLastError();
}

}  // namespace gbp
