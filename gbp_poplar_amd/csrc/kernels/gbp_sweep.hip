// kernels/gbp_sweep.hip — k_sweep and k_linearise with their launchers: the per-factor half of an iteration.
#pragma once
#include "gbp_tile.hpp"
#include "gbp_vertex.hpp"
#include "gbp_metric_math.hpp"      // ride_metric (k_sweep<EV>)

namespace gbp {
using namespace gbpdev;

// =================================================================================================
// k_sweep: one lane = one factor.
// =================================================================================================
// HOIST = true: the belief means are per-VARIABLE quantities (inf2mean of the camera / landmark belief,
// gbp_codelets.cpp:264-265) that the reference recomputes in every incident factor.  The belief kernels
// compute them once per variable; dmu^2 = ((((((0+t0)+..+t5) + u0) + u1) + u2) splits into a per-camera
// prefix S_c (CAMB slot 6) and three per-landmark terms u (LMKB slots 3,13,14), evaluated with the same
// fp32 operations in the same order, so the result is bit-identical while the per-factor MU stream and
// two of the five small inverses disappear from the sweep.  HOIST = false keeps the literal per-factor
// mu/oldmu tensors (needed only if a caller uploads non-zero oldmu).
constexpr int kWpb = 4;      // wavefronts per workgroup of the sweep (the waves of a workgroup share nothing)
// POL: cache policy of the two message streams (SweepArgs.policy, chosen per graph shape by gbp_api_ctx.cpp; a template parameter,
// not a branch on the flag: with both load sequences behind a branch the non-temporal path lost 1.2 %)
// EV: the metric of the PREVIOUS iteration rides in this sweep (EvalRide in gbp_kernels.h)
// SEG: the tile's all-pad segments (four lanes) are neither loaded nor stored (SweepArgs.seg_live, load_tile_seg above); the state
// planes — 4 or 8 bytes per position — are moved whole
// ISSUE: kIssue* bits (gbp_kernels.h) — WHEN the loads of the relinearising path are requested.  The same bytes and the same
// arithmetic either way; the product runs kSweepIssue, the test-hooks build can be told to run the other (gbp_debug_force_sweep_policy).
constexpr int kRelinSlots = 8;      // 1 KiB LDS-DMA slots of a wave's relinearisation operands: FST_VAR (256 B of it), CAM_MU 0..1, CAM_LIN 0..4
template <bool HOIST, uint32_t POL = 0, bool EV = false, bool SEG = false, uint32_t ISSUE = kSweepIssue>
GBP_DEV void sweep_tile(const SweepArgs& a, const uint32_t wslot) {
  constexpr bool EARLY = HOIST && (ISSUE & kIssueEarlyRelin) != 0;      // (the literal-mu sweep keeps its path: it fetches the variance only)
  // (the slot is wave-uniform: as an SGPR it turns the permutation look-up into one scalar load)
  const uint32_t ws = (uint32_t)__builtin_amdgcn_readfirstlane((int)wslot);
  const uint32_t tile = a.tile_perm ? a.tile_perm[ws] : ws;
  const uint32_t lane = threadIdx.x & 63, p = tile * 64 + lane;
  const uint32_t ev_done = EV ? (uint32_t)__builtin_amdgcn_readfirstlane((int)*a.ev.counter) : 0u;     // (a scalar load, up here)

  const uint32_t cam_i = a.row_cam[p >> 4];
  const uint32_t lmk_i = __builtin_nontemporal_load(a.lmk_idx + p);
  // EARLY: the packed word goes out in FRONT of the streams — its count decides, behind cmsg_expand and while the gathers are still in
  // flight, whether the wave requests its relinearisation operands (the vm counter retires in order: requested behind the gathers,
  // as below, the word would be the last thing to land)
  const int packed_first = EARLY ? a.fst_packed[p] : 0;

  // SEG: bit s of the tile's mask = the 64-byte segment of lanes 4s .. 4s + 3 holds at least one factor (one scalar load)
  const uint32_t segm = SEG ? a.seg_live[tile] : 0xffffu;
  const bool live8 = !SEG || ((segm >> (lane >> 2)) & 1u) != 0u;
  float fac[56], cmr[16], mu[12], lm[16], cb[44], lb[16];
  if (SEG) load_tile_seg<kFacG>(a.fac, tile, lane, live8, fac);
  else load_tile<kFacG>(a.fac, tile, lane, fac);
  // The camera messages: non-temporal like the potentials, or — SweepArgs.cmsg_cached, graphs with few cameras — with the
  // default policy like the landmark messages below (both are rewritten in place by this tile).  The potentials, which an
  // ordinary sweep only reads, keep the hint on every graph: with default-policy loads they cost 3 %.
  if (SEG) load_tile_seg<kCmsgG, !(POL & kPolCmsgLoadCached)>(a.cmsg, tile, lane, live8, cmr);
  else load_tile<kCmsgG, !(POL & kPolCmsgLoadCached)>(a.cmsg, tile, lane, cmr);
  if (!HOIST) load_tile<kMuG>(a.mu, tile, lane, mu);
  // Landmark messages: the wave's 3 KiB block of LMSG through the wave-private LDS stage (lmsg_tile_in above), the two state planes
  // the sweep reads every time with it.  SEG: a float4 of an all-pad segment (lmsg_seg_live) is given an offset beyond the tile's
  // descriptor — zeros for the load, nothing for the store, no memory access.
  __shared__ float4 lm_stage[kWpb][64 * kLmsgG];
  float4* stage = lm_stage[threadIdx.x >> 6];
  float4* lm_tile = a.lmsg + (size_t)tile * (64 * kLmsgG);
  const __amdgpu_buffer_rsrc_t lm_rsrc = tile_rsrc<kLmsgG>(a.lmsg, SEG ? tile : 0u);
  // (DEFAULT policy for this one stream unless the shape says otherwise: the tile is rewritten in place ten microseconds later
  // and gathered by k_beliefs right after the sweep — measured +1.5 % iterations/s on the 1M-factor graph against the
  // non-temporal hint, with either store policy; the potentials keep the hint on every graph)
  lmsg_tile_in(stage, lane, [&](uint32_t k) {
    if (SEG) {
      typedef unsigned v4u __attribute__((ext_vector_type(4)));
      const bool live_k = lmsg_seg_live(segm, k * 64u + lane);
      const v4u v = __builtin_amdgcn_raw_buffer_load_b128(lm_rsrc, (live_k ? (int)(lane * 16u) : kBufOob) + (int)k * 1024, 0, (POL & kPolLmsgLoadNt) ? 2 : 0);
      return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
    }
    const v4f* src = reinterpret_cast<const v4f*>(lm_tile) + k * 64u + lane;
    const v4f v = (POL & kPolLmsgLoadNt) ? __builtin_nontemporal_load(src) : *src;
    return make_float4(v.x, v.y, v.z, v.w);
  }, lm);
  load_rec<kCamRec4>(a.camb + (size_t)cam_i * kCamRec4, cb);
  load_rec<kLmkRec4>(a.lmkb + (size_t)lmk_i * kLmkRec4, lb);
  const int packed = EARLY ? packed_first : a.fst_packed[p];      // (behind the gathers: nothing needs them before the gathers have landed)
  float damping = a.fst_damp[p];
  // EV: the camera's metric record (one address per 16-lane row) and the landmark's metric mean (a 16-byte gather from a table
  // 1/4 the size of the beliefs') go out WITH the belief gathers — unconditionally: pads index 0 — and wait in a wave-private
  // LDS area for the end of the tile, where the registers are free: 16 more live registers in this prologue (50 loads in
  // flight, 236 of 256 VGPRs) made the compiler issue the belief gathers BEHIND the metric — two dependent round trips per
  // wave, +8 us per sweep (the ISA showed it, profiles/r05_default_loop.md).
  __shared__ float4 ev_stage[EV ? kWpb : 1][EV ? 64 * 4 : 1];
  float4 evq0, evq1, evq2, evq3;
  if (EV) {
    evq0 = a.ev.cam_rec[(size_t)cam_i * 3]; evq1 = a.ev.cam_rec[(size_t)cam_i * 3 + 1]; evq2 = a.ev.cam_rec[(size_t)cam_i * 3 + 2];
    evq3 = a.ev.lmk_mean[lmk_i];
    // (a compiler barrier: without it the belief gathers above — used only by active lanes — are sunk into that branch, behind
    // the wait for the metric records)
    asm volatile("" ::: "memory");
  }
  // per-factor scalar state: the packed word and the damping from their planes (above); the measurement variance is read by
  // relin_core only, so the sweep fetches it where a lane relinearises (beside the means below) and never writes it
  int count = packed >> 3;
  uint32_t flags = (uint32_t)packed & 7u;
  const float var = 0.f;
  const bool active = (flags & kFlagActive) != 0;
  const bool count_was_0 = count == 0;      // (factor_update then sets the damping: see the store of FST_DAMP below)

  float K[9];
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) K[i] = a.K[i];

  const int ev_packed = packed;      // EV: the factor's state word as the sweep of the evaluated iteration left it
  const float ev_z0 = fac[54], ev_z1 = fac[55];
  if (EV) {
    float4* park = ev_stage[threadIdx.x >> 6];
    park[lane] = evq0; park[64 + lane] = evq1; park[128 + lane] = evq2; park[192 + lane] = evq3;
  }

  // the message the record stands for, from the potential as loaded (it needs the two tile streams only: it runs under the gathers)
  float cm[28];
  cmsg_expand(fac, cmr, a.cmsg_lit, tile, lane, cm);

  // EARLY: relin = dmu < threshold && count + 1 > min_linear_iters - num_undamped_iters (factor_update), and the second condition is
  // known as soon as the packed word has landed.  Where it holds for a lane of the wave, the operands only a relinearising lane reads —
  // its variance, its camera's hoisted mean and CAM_LIN record: L2-resident tables — are requested HERE, eight LDS-DMA transfers into
  // a wave-private area (no register: the kernel stands at the limit of two waves per SIMD), so that they travel with the belief
  // gathers factor_update is about to wait for — instead of inside factor_update behind the dmu test, where both waves of a SIMD sat
  // out a round trip of their own in the middle of the arithmetic.  A lane whose dmu then fails the test leaves its 128 bytes
  // unread.  On S1 no lane passes in 10 sweeps of 11, and the wave executes one compare and one branch more.
  //  * HERE, not in the load prologue: a branch in the prologue ends the block in which the compiler interleaves cmsg_expand with the
  //    loads, and the wave then waited for every gather before its first multiplication — in every sweep (profiles/sweep_issue_order.md).
  //  * The test is ONE compare into a scalar pair, on the count alone (count + 1 > bound <=> packed >= 8 x bound: an arithmetic
  //    shift rounds down): an inactive or pad lane beyond the bound makes its wave request operands nobody reads, which is correct.
  //    The active bit would need a vector register, and so would address arithmetic: the free ones are dead slots of belief
  //    records still in flight, and writing one waits for that gather.  So the wave's number is taken as a scalar and the camera
  //    records are addressed by INDEX through descriptors that carry their stride.
  __shared__ float4 rl_stage[EARLY ? kWpb : 1][EARLY ? 64 * kRelinSlots : 1];
  static_assert(3 + kCamLin4 == kRelinSlots, "one slot per transfer");
  if (EARLY) {
    const int bound8 = (a.hp.min_linear_iters - a.hp.num_undamped_iters) * 8;
    unsigned long long may_relin;      // the lanes with count + 1 > min_linear_iters - num_undamped_iters
    asm volatile("v_cmp_le_i32 %0, %2, %1" : "=s"(may_relin) : "v"(packed_first), "s"(bound8));
    if (may_relin != 0ull) {      // (every lane asks, pads too: row_cam and the planes cover all positions)
      float4* rl = rl_stage[(uint32_t)__builtin_amdgcn_readfirstlane((int)threadIdx.x) >> 6];
      const __amdgpu_buffer_rsrc_t mu_t = rec_rsrc(a.cam_mu, 4 * 16), lin_t = rec_rsrc(a.cam_lin, kCamLin4 * 16);
      lds_dma<4>(a.fst_var + p, rl);
      lds_dma_rec16(mu_t, cam_i, 0, rl + 64);
      lds_dma_rec16(mu_t, cam_i, 16, rl + 128);
      GBP_UNROLL
      for (int g = 0; g < kCamLin4; ++g) lds_dma_rec16(lin_t, cam_i, g * 16, rl + (3 + g) * 64);
    }
  }

  float oc_eta[6], oc_lam[36], bi[9], ol[16];
  bool relin;
  factor_update<HOIST>(fac, cm, mu, lm, cb, lb, K, a.hp, damping, count, flags, var, active, oc_eta, oc_lam, bi, ol, relin,
                            [&](float (&x0c)[6], float (&x0l)[3], CamLin& cl, float& var_r) {   // rare path: loaded only by relinearising lanes
                              float4 m0, m1, q[kCamLin4];
                              if (EARLY) {      // requested above (a lane that gets here passed the count test there)
                                lds_dma_wait();
                                const float4* rl = rl_stage[threadIdx.x >> 6];
                                var_r = reinterpret_cast<const float*>(rl)[lane];
                                m0 = rl[64 + lane]; m1 = rl[128 + lane];
                                GBP_UNROLL
                                for (int g = 0; g < kCamLin4; ++g) q[g] = rl[(3 + g) * 64 + lane];
                              } else {
                                var_r = a.fst_var[p];
                                if (!HOIST) return;      // (the literal mu tensors: the means are the lane's own)
                                // camera side: the hoisted mean and its CAM_LIN record — per-camera tables (C x 144 B) that live in L2
                                m0 = a.cam_mu[(size_t)cam_i * 4]; m1 = a.cam_mu[(size_t)cam_i * 4 + 1];
                                GBP_UNROLL
                                for (int g = 0; g < kCamLin4; ++g) q[g] = a.cam_lin[(size_t)cam_i * kCamLin4 + g];
                              }
                              x0c[0] = m0.x; x0c[1] = m0.y; x0c[2] = m0.z; x0c[3] = m0.w; x0c[4] = m1.x; x0c[5] = m1.y;
                              cam_lin_unpack(q, cl);
                              // landmark side: the mean is RECOMPUTED from the belief record the lane holds anyway — inf2mean3x3
                              // (bafuncs.cpp:11-15) by lmk_mean, as k_beliefs computes LMK_MU, so the same bits — instead of
                              // gathered: a second random gather (a 128-B line fill per factor for 12 useful bytes) made the
                              // lock-step relinearising sweep move 104 MB more than it has to
                              lmk_mean(lb, x0l);
                            });

  // ---- outputs --------------------------------------------------------------------------------
  lmsg_tile_out(stage, lane, ol, [&](uint32_t k, float4 f) {
    if (SEG) {
      typedef unsigned v4u __attribute__((ext_vector_type(4)));
      const bool live_k = lmsg_seg_live(segm, k * 64u + lane);
      const v4u v = {__float_as_uint(f.x), __float_as_uint(f.y), __float_as_uint(f.z), __float_as_uint(f.w)};
      __builtin_amdgcn_raw_buffer_store_b128(v, lm_rsrc, (live_k ? (int)(lane * 16u) : kBufOob) + (int)k * 1024, 0, (POL & kPolLmsgStoreNt) ? 2 : 0);
    } else if (POL & kPolLmsgStoreNt) {
      const v4f v = {f.x, f.y, f.z, f.w};
      __builtin_nontemporal_store(v, reinterpret_cast<v4f*>(lm_tile) + k * 64u + lane);
    } else {
      lm_tile[k * 64u + lane] = f;
    }
  });
  // the state planes: the packed word every sweep (the count of an active factor moves every sweep); the damping only when a lane
  // of the wave has written it — factor_update does at a relinearisation and when the count stands at 0, nowhere else — and then from
  // all 64 lanes (whole lines).  No branch: the store goes through a descriptor of the tile's 256 bytes of the plane, and a wave
  // that has nothing to say gives every lane an offset beyond it — the hardware drops the store without a memory access, as for an
  // all-pad segment (load_tile_seg).  (A branch round a plain store cost 10 to 14 VGPRs and the second wave per SIMD of two instantiations.)
  a.fst_packed[p] = (int)(((uint32_t)count << 3) | flags);
  {
    // (the literal-mu instantiation stores every time: with the test it needs 259 registers, one wave per SIMD)
    const bool wave_wrote = !HOIST || __builtin_amdgcn_ballot_w64(active && (count_was_0 || relin)) != 0ull;
    const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc(a.fst_damp + (size_t)tile * 64, 0, 256, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(damping), dr, wave_wrote ? (int)(lane * 4u) : kBufOob, 0, 0);
  }
  {
    float cmo[16];
    cmsg_pack(oc_eta, bi, active, cmo);
    if (SEG) store_tile_seg<kCmsgG>(a.cmsg, tile, lane, live8, cmo);
    else store_tile<kCmsgG>(a.cmsg, tile, lane, cmo);
  }
  // camera half of the belief reduction: per-row (16 factors of one camera) tree sums
  {
    float4* rp = a.rowp + (size_t)(p >> 4) * kCamRec4;
    row16_sums_store(oc_eta, oc_lam, lane, [&](uint32_t g, float4 v) { rp[g] = v; });
  }
  if (active) {
    if (!HOIST) store_tile<kMuG>(a.mu, tile, lane, mu);
    if (relin) store_tile<kFacG>(a.fac, tile, lane, fac);
  }
  if (EV) {
    // The metric of the iteration that has just ended (EvalRide in gbp_kernels.h), behind this tile's own work: the factor's
    // state word as ITS sweep left it, the measurement, the metric records parked above.
    const float4* park = ev_stage[threadIdx.x >> 6];
    ride_metric(a.ev, ev_done, ws, tile, lane, ev_packed, ev_z0, ev_z1, park[lane], park[64 + lane], park[128 + lane], park[192 + lane], K);
  }
}

template <bool HOIST, uint32_t POL = 0, bool EV = false, bool SEG = false, uint32_t ISSUE = kSweepIssue>
__global__ __launch_bounds__(64 * kWpb) void k_sweep(const SweepArgs a) {
  sweep_tile<HOIST, POL, EV, SEG, ISSUE>(a, blockIdx.x * kWpb + (threadIdx.x >> 6));
}

// =================================================================================================
// k_linearise: RelineariseFactorVertex on every factor (no active_flag test in the reference).
// =================================================================================================
__global__ __launch_bounds__(256) void k_linearise(const SweepArgs a) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  const uint32_t tile = p >> 6, lane = p & 63;
  const uint32_t cam_i = a.row_cam[p >> 4], lmk_i = a.lmk_idx[p];
  const int packed = a.fst_packed[p];
  uint32_t flags = (uint32_t)packed & 7u;
  if (flags & kFlagPad) return;
  float fac[56], cb[44], lb[16], K[9], x0c[6], x0l[3];
  load_tile<kFacG>(a.fac, tile, lane, fac);
  load_rec<kCamRec4>(a.camb + (size_t)cam_i * kCamRec4, cb);
  load_rec<kLmkRec4>(a.lmkb + (size_t)lmk_i * kLmkRec4, lb);
  // The potential is about to change under the factor's camera message, which a kCmsgDerived record derives from it: such a record
  // is first made literal — its Lambda, from the potential it still holds here, into CMSG_LIT.  (a.cmsg_lit == NULL: no sweep has run
  // since the upload's zero fill — the shipped flows, LINEARISE right behind WRITE — so no record is derived)
  if (a.cmsg_lit) {
    float4* last = a.cmsg + ((size_t)tile * kCmsgG + (kCmsgG - 1)) * 64 + lane;      // Bi[6..8], format word
    const float4 w3 = *last;
    if (w3.w == kCmsgDerived) {
      float rec[16], cm[28], l[kCmsgLitG * 4];
      load_tile<kCmsgG, false>(a.cmsg, tile, lane, rec);
      cmsg_expand(fac, rec, nullptr, tile, lane, cm);
      GBP_UNROLL
      for (int i = 0; i < kCmsgLitG * 4; ++i) l[i] = i < 21 ? cm[6 + i] : 0.f;
      store_tile<kCmsgLitG, false>(a.cmsg_lit, tile, lane, l);
      *last = make_float4(w3.x, w3.y, w3.z, kCmsgLiteral);
    }
  }
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) K[i] = a.K[i];
  GBP_UNROLL
  for (int i = 0; i < 54; ++i) fac[i] = 0.f;
  belief_means(cb, lb, x0c, x0l);
  CamLin cl;
  const float wv[3] = {x0c[3], x0c[4], x0c[5]};
  cam_lin(wv, cl);
  const bool robust = relin_core(fac, x0c, x0l, K, a.fst_var[p], a.hp.nstds, cl);
  flags = robust ? (flags | kFlagRobust) : (flags & ~kFlagRobust);
  a.fst_packed[p] = (packed & ~7) | (int)flags;
  store_tile<kFacG>(a.fac, tile, lane, fac);
}

#ifdef GBP_BUILD_EXPERIMENTS
bool lab_launch_sweep(const SweepArgs& a, uint32_t n_tiles, bool hoist, hipStream_t s);   // experiments/gbp_lab_kernels.hip
#endif
void launch_sweep(const SweepArgs& a, uint32_t n_tiles, bool hoist, hipStream_t s, bool ev) {
  const dim3 g(n_tiles / kWpb), b(64 * kWpb);
  const bool seg = a.seg_live && hoist && a.policy == 0u;      // a graph of many small cameras (gbp_api_ctx.cpp decides): the all-pad segments are skipped
  if (ev && hoist) {        // the metric rides along (gbp_iterate_eval_each beyond k_persist): the policies sweep_policy_for() chooses
    if (seg) hipLaunchKernelGGL((k_sweep<true, 0, true, true>), g, b, 0, s, a);
    else if (a.policy == kPolCmsgLoadCached) hipLaunchKernelGGL((k_sweep<true, kPolCmsgLoadCached, true>), g, b, 0, s, a);
    else hipLaunchKernelGGL((k_sweep<true, 0, true>), g, b, 0, s, a);
    return;
  }
#ifdef GBP_BUILD_EXPERIMENTS
  if (lab_launch_sweep(a, n_tiles, hoist, s)) return;     // a mapping experiment / an ablated sweep was asked for (SweepArgs.variant)
#endif
  if (!hoist) { hipLaunchKernelGGL(k_sweep<false>, g, b, 0, s, a); return; }
#ifdef GBP_BUILD_TEST_HOOKS      // the other issue order of the plain hoisted sweep (gbp_debug_force_sweep_policy + kPolForceLateRelin: A/B measurements, tests)
  if (a.issue != kSweepIssue && (seg || a.policy <= kPolCmsgLoadCached)) {
    constexpr uint32_t kOther = kSweepIssue ^ kIssueEarlyRelin;
    if (seg) hipLaunchKernelGGL((k_sweep<true, 0, false, true, kOther>), g, b, 0, s, a);
    else if (a.policy == kPolCmsgLoadCached) hipLaunchKernelGGL((k_sweep<true, kPolCmsgLoadCached, false, false, kOther>), g, b, 0, s, a);
    else hipLaunchKernelGGL((k_sweep<true, 0, false, false, kOther>), g, b, 0, s, a);
    return;
  }
#endif
  if (seg) { hipLaunchKernelGGL((k_sweep<true, 0, false, true>), g, b, 0, s, a); return; }
  switch (a.policy) {      // the instantiations sweep_policy_for() (gbp_api_ctx.cpp) can choose
    case kPolCmsgLoadCached: hipLaunchKernelGGL((k_sweep<true, kPolCmsgLoadCached>), g, b, 0, s, a); break;
    case kPolLmsgLoadNt | kPolLmsgStoreNt: hipLaunchKernelGGL((k_sweep<true, kPolLmsgLoadNt | kPolLmsgStoreNt>), g, b, 0, s, a); break;
#ifdef GBP_BUILD_TEST_HOOKS      // the other combinations, for measurements (gbp_debug_force_sweep_policy)
    case 2: hipLaunchKernelGGL((k_sweep<true, 2>), g, b, 0, s, a); break;
    case 3: hipLaunchKernelGGL((k_sweep<true, 3>), g, b, 0, s, a); break;
    case 4: hipLaunchKernelGGL((k_sweep<true, 4>), g, b, 0, s, a); break;
    case 5: hipLaunchKernelGGL((k_sweep<true, 5>), g, b, 0, s, a); break;
    case 7: hipLaunchKernelGGL((k_sweep<true, 7>), g, b, 0, s, a); break;
#endif
    default: hipLaunchKernelGGL((k_sweep<true, 0>), g, b, 0, s, a); break;
  }
}
void launch_linearise(const SweepArgs& a, uint32_t n_tiles, hipStream_t s) {
  hipLaunchKernelGGL(k_linearise, dim3(n_tiles / 4), dim3(256), 0, s, a);
}

}  // namespace gbp
