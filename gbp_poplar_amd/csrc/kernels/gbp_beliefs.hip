// kernels/gbp_beliefs.hip — the belief owners (beliefs_body and its seven k_beliefs* kernels), the two gather kernels of the
// peer-memory exchanges, and their launchers: the per-variable half of an iteration.
#pragma once
#include "gbp_tile.hpp"
#include "gbp_vertex.hpp"
#include "gbp_metric_math.hpp"      // solve_pivot, ldl_pivots_positive, eval_cam_rot (the EV instantiations)

namespace gbp {
using namespace gbpdev;

// =================================================================================================
// k_beliefs: buildUpdateBeliefsProg (ba.cpp:104-139) in ONE launch.
//   blocks [0, cam_blocks): camera part, one wavefront per camera (lanes 0..43 = the 44-float record);
//   remaining blocks:       landmark part, four lanes per landmark (lane q = float4 #q of the record).
// Camera beliefs: local = rows of this camera left to right (rows were tree-summed by k_sweep), then
// belief = prior + local (single GPU) or prior + sum_r gathered[r] (after the all-gather, rank order).
// Landmark beliefs: prior + messages in slot order.  With `hoist` the belief means (inf2mean, bafuncs.cpp:2-15)
// and the dmu^2 pieces of the next sweep are computed here once per variable (see k_sweep<HOIST>).
// =================================================================================================
// EV: the belief owners also leave the METRIC RECORDS of the new beliefs (EvalRide in gbp_kernels.h): what k_means computes.
// CAM_ONLY: a launch without landmark blocks (the camera combine behind the exchange of a sharded iteration, prior-only refreshes of the
// split-phase path): the landmark half is compiled out, so the kernel needs the camera half's registers only — 8 waves per SIMD instead of
// 7, i.e. the 2 000 workgroups of an 8 000-camera graph resident in ONE generation (256 CUs x 8) instead of one and a bit
// PEERS (with CAM_ONLY): the combine behind the direct peer-memory exchange — partial r straight from peers[r] (rank r's exchange
// buffer, slot r) instead of b.gathered[r]; the same additions in the same order, so the same bits
// SLICE (with PEERS): the reduce of the sliced peer-memory exchange — the launch covers the cameras [sl.lo, sl.hi) only (block 0 starts at
// camera sl.lo) and, next to this rank's own tables, leaves every finished camera as one result record (CamSlice in gbp_kernels.h) for
// the other ranks to gather
template <bool EV, bool CAM_ONLY = false, bool PEERS = false, bool SLICE = false>
GBP_DEV void beliefs_body(const BeliefArgs& b, const float* const* __restrict__ peers = nullptr, const CamSlice sl = CamSlice{}) {
  __shared__ float sh[4][48];
  __shared__ float lrec[EV ? 64 : 1][13];      // EV: the beliefs of the workgroup's 64 landmarks (eta 3, Lambda 9; 13: bank spread)
  // one more iteration of the burst done (read by the NEXT sweep) — counted by the LAST belief launch of the iteration: where the update is
  // two launches round an exchange (a sharded ctx), the first carries kEvNotLast and the camera combine behind the exchange counts
  if (EV && !(b.ev_split & kEvNotLast) && blockIdx.x == 0 && threadIdx.x == 0) *b.ev.counter = *b.ev.counter + 1u;
  // Which blocks are the cameras'?  The FIRST cam_blocks of the grid where a camera block ends in the serial chain of its means (long
  // latency: started first, hidden under the landmark blocks) — the LAST ones where it only adds up rows (partial_only, before the
  // exchange of a sharded iteration): short work that fills the slots the landmark blocks free as they drain, instead of holding the
  // first generation of the grid (config-5 shard shape: profiles/r06_sharded_timeline.md)
  const bool cams_last = !CAM_ONLY && b.partial_only != 0 && b.lmk_blocks != 0u;
  const bool cam_block = cams_last ? blockIdx.x >= b.lmk_blocks : blockIdx.x < b.cam_blocks;
  if (cam_block) {
    const uint32_t w = threadIdx.x >> 6, j = threadIdx.x & 63;
    const uint32_t cblk = cams_last ? blockIdx.x - b.lmk_blocks : blockIdx.x;
    const uint32_t cam0 = SLICE ? sl.lo : 0u, cam1 = SLICE ? sl.hi : b.n_cams;      // the cameras of this launch
    const uint32_t c = cam0 + cblk * 4 + w;
    const bool live = c < cam1 && j < (uint32_t)kCamRec;
    float bel = 0.f;
    if (live) {
      // WeakenPriorVertex (gbp_codelets.cpp:176-197) rides in the belief refresh WEAKEN_PRIORS ends with (ba.cpp:863-865): the
      // owner of a prior element scales it on its way into the sum and writes it back; lane 0 then counts the flag down (every
      // lane of the record sits in this wave and has read the flag by then)
      float prior = b.cam_prior[(size_t)c * kCamRec + j];
      const uint32_t wf = b.weaken ? b.cam_wflag[c] : 0u;
      if (wf >= 1u && wf <= 5u) {
        prior *= b.cam_scale[c];
        b.cam_prior_rw[(size_t)c * kCamRec + j] = prior;
      }
      if (PEERS) {
        const size_t off = (size_t)c * kCamRec + j;
        float acc = prior;
        for (int r0 = 0; r0 < b.world; r0 += 8) {      // as below: eight ranks' loads in flight (clamped, unconditional), rank order
          float v[8];
          GBP_UNROLL
          for (int k = 0; k < 8; ++k) v[k] = peers[r0 + k < b.world ? r0 + k : b.world - 1][off];      // wave-uniform table entry
          GBP_UNROLL
          for (int k = 0; k < 8; ++k)
            if (r0 + k < b.world) acc = acc + v[k];
        }
        bel = acc;
      } else if (b.gathered) {
        const float* g = b.gathered + (size_t)c * kCamRec + j;      // exchange layout: [world][C][44]
        float acc = prior;
        for (int r0 = 0; r0 < b.world; r0 += 8) {      // the partials of eight ranks in flight at once (clamped, unconditional), added in rank order
          float v[8];
          GBP_UNROLL
          for (int k = 0; k < 8; ++k) v[k] = g[(size_t)(r0 + k < b.world ? r0 + k : b.world - 1) * b.n_cams * kCamRec];
          GBP_UNROLL
          for (int k = 0; k < 8; ++k)
            if (r0 + k < b.world) acc = acc + v[k];
        }
        bel = acc;
      } else {
        const uint32_t r0 = b.cam_row_ptr[c], r1 = b.cam_row_ptr[c + 1];
        float acc = 0.f;
        if (r1 > r0 && !b.row_slot) {
          const float* row = b.rowp + (size_t)r0 * kCamRec + j;
          acc = row[0];
          uint32_t r = 1;
          const uint32_t n = r1 - r0;
          for (; r + 16 <= n; r += 16) {  // loads of 16 rows in flight, adds in row order
            float v[16];
            GBP_UNROLL
            for (int k = 0; k < 16; ++k) v[k] = row[(size_t)(r + k) * kCamRec];
            GBP_UNROLL
            for (int k = 0; k < 16; ++k) acc = acc + v[k];
          }
          {  // tail (< 16 rows) in one batch as well, the loads unconditional (row clamped, value dropped: a conditional load is a
             // branch with its own wait): this chain is pure load latency
            float v[16];
            const uint32_t m = n - r;
            GBP_UNROLL
            for (int k = 0; k < 16; ++k) v[k] = row[(size_t)((uint32_t)k < m ? r + k : n - 1u) * kCamRec];
            GBP_UNROLL
            for (int k = 0; k < 16; ++k)
              if ((uint32_t)k < m) acc = acc + v[k];
          }
        } else if (r1 > r0) {
          // the camera's rows sit where the row placement put them (gbp_layout.cpp): the same sums in the same order, each row
          // found through row_slot (wave-uniform indices: one round of scalar loads in front of the rows')
          const float* base = b.rowp + j;
          const uint32_t n = r1 - r0;
          acc = base[(size_t)b.row_slot[r0] * kCamRec];
          for (uint32_t r = 1; r < n; r += 16) {
            uint32_t sl[16];
            float v[16];
            const uint32_t m = n - r;
            GBP_UNROLL
            for (int k = 0; k < 16; ++k) sl[k] = b.row_slot[r0 + ((uint32_t)k < m ? r + k : n - 1u)];      // clamped, unconditional
            GBP_UNROLL
            for (int k = 0; k < 16; ++k) v[k] = base[(size_t)sl[k] * kCamRec];
            GBP_UNROLL
            for (int k = 0; k < 16; ++k)
              if ((uint32_t)k < m) acc = acc + v[k];
          }
        }
        b.cam_local[(size_t)c * kCamRec + j] = acc;
        bel = prior + acc;
      }
      sh[w][j] = bel;
      if (j == 0 && wf >= 1u && wf <= 5u) b.cam_wflag[c] = wf - 1u;
    }
    if (b.partial_only) return;      // (EV too: a partial sum is no belief — no camera metric record, no health word; the combine leaves them)
    __syncthreads();
    // The 6x6 mean of a camera is one serial instruction stream on ONE lane.  The four cameras of the workgroup share a
    // single stream (lanes 0..3 of wave 0) instead of issuing it from four wavefronts: with thousands of cameras the
    // camera part is bound by exactly these issue slots (8 000 cameras: 11 -> 4 us).
    if (b.hoist && w == 0 && j < 4) {
      const uint32_t cj = cam0 + cblk * 4 + j;
      if (cj < cam1) {
        float x0c[6];
        cam_mean(sh[j], x0c);                    // operands straight from LDS: the 44-float copy cost 14 VGPRs of occupancy
        float4* mu = b.cam_mu + (size_t)cj * 4;  // [0,1] = means of the current belief, [2,3] = means the last sweep used
        float4 u0 = mu[2], u1 = mu[3];
        if (b.roll) { u0 = mu[0]; u1 = mu[1]; mu[2] = u0; mu[3] = u1; }
        const float used[6] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y};
        const float S = cam_dmu2(used, x0c);
        mu[0] = make_float4(x0c[0], x0c[1], x0c[2], x0c[3]);
        mu[1] = make_float4(x0c[4], x0c[5], 0.f, 0.f);
        sh[j][6] = S;
        // camera-only Jacobian terms of this mean (gbp_device_math.hpp: cam_lin), once per camera instead of once per
        // relinearising factor
        CamLin cl;
        const float wv[3] = {x0c[3], x0c[4], x0c[5]};
        cam_lin(wv, cl);
        float4 q[kCamLin4];
        cam_lin_pack(cl, q);
        GBP_UNROLL
        for (int g = 0; g < kCamLin4; ++g) b.cam_lin[(size_t)cj * kCamLin4 + g] = q[g];
        if (SLICE) {      // the same registers into the camera's result record: float4 11, 12 = the mean, 13 .. 17 = CAM_LIN
          float4* res = sl.res + (size_t)(cj - cam0) * kCamRes4 + kCamRec4;
          res[0] = make_float4(x0c[0], x0c[1], x0c[2], x0c[3]);
          res[1] = make_float4(x0c[4], x0c[5], 0.f, 0.f);
          GBP_UNROLL
          for (int g = 0; g < kCamLin4; ++g) res[2 + g] = q[g];
        }
      }
    }
    if (EV && (w == 1 || w == 2) && j < 4) {
      // The metric's share of a camera, on the workgroup's OTHER waves (three long serial chains on one lane would set the
      // length of the whole kernel): wave 1 solves the fp64 pivoted means of the four cameras (util.cpp:103-105 stand-in, as
      // k_means) and leaves rotation + translation for the residuals, wave 2 checks the LDL^T pivots.  Both read the belief
      // (eta at sh[.][0..5], Lambda at sh[.][8..43]); wave 0 writes sh[.][6] only.  The 6 x 7 fp64 tableau takes the kernel from
      // 68 to 96 VGPRs = from 7 to 5 waves per SIMD, which costs the landmark part 1.5 us; measured and worse: the occupancy
      // pinned at 7 (the tableau spills: 20.1 us against 18.3), the tableau in LDS (21.4 - 25.1 us: the camera chain then sets the
      // kernel's length) — profiles/r05_default_loop.md.
      const uint32_t cj = cam0 + cblk * 4 + j;
      const bool count_cams = !(b.ev_split & kEvNoCamHealth);      // cameras are replicated over the ranks: rank 0 counts them (as k_means: count_cams)
      if (cj < cam1) {
        if (w == 1) {
          float xm[6], R[9];
          solve_pivot<6>(sh[j] + 8, 6, sh[j], xm);
          bool finite = true;
          GBP_UNROLL
          for (int i = 0; i < 6; ++i) finite &= (xm[i] - xm[i] == 0.f);
          if (!finite && count_cams) atomicAdd(&b.ev.health[0], 1ull);
          eval_cam_rot(xm, R);
          float4* rec = b.ev.cam_rec + (size_t)cj * 3;
          rec[0] = make_float4(R[0], R[1], R[2], xm[0]);
          rec[1] = make_float4(R[3], R[4], R[5], xm[1]);
          rec[2] = make_float4(R[6], R[7], R[8], xm[2]);
        } else if (count_cams && !ldl_pivots_positive<6>(sh[j] + 8, 6)) {
          atomicAdd(&b.ev.health[1], 1ull);
        }
      }
    }
    __syncthreads();
    if (live) b.camb[(size_t)c * kCamRec + j] = sh[w][j];
    if (SLICE && live) reinterpret_cast<float*>(sl.res + (size_t)(c - cam0) * kCamRes4)[j] = sh[w][j];      // float4 0 .. 10 = the belief record
    return;
  }
  if (CAM_ONLY) return;
  // ---- landmark part ----
  uint32_t lb = cams_last ? blockIdx.x : blockIdx.x - b.cam_blocks;
  if (b.lmk_xcd_order) {
    // XCD-aware order: the blocks that share an XCD (equal index mod 8 under round-robin placement) take one contiguous
    // run of landmarks.  The 64-B message records of two neighbouring factors share a 128-B line, and the partner's
    // landmark is a near neighbour (factors are sorted by landmark inside a camera): with both in one XCD's L2 about
    // half of the partner fetches disappear (k_beliefs: 25.6 -> 21.3 us on the 1M-factor graph).
    const uint32_t qn = b.lmk_blocks / 8, rn = b.lmk_blocks % 8, g = lb & 7u;
    lb = g * qn + (g < rn ? g : rn) + (lb >> 3);
  }
  const uint32_t t = lb * 256 + threadIdx.x;
  const uint32_t l = t >> 2, q = t & 3;
  const bool live = l < b.n_lmks;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  // LMK_IX[l] = {degree, position of slot 1 .. slot 15} (64 B): ONE load tells the quad where the landmark's records
  // are, so the whole sum is two dependent round trips (index record -> up to 15 message records in flight) instead
  // of four (lmk_ptr -> fpos -> 8 records -> tail).  Slots beyond 15 (rare) go through lmk_ptr / lmk_fpos.
  uint4 ix = make_uint4(0u, 0u, 0u, 0u);
  float4 used_mu = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    ix = reinterpret_cast<const uint4*>(b.lmk_ix)[(size_t)l * 4 + q];
    acc = b.lmk_prior[(size_t)l * 4 + q];
    if (b.weaken) {        // WeakenPriorVertex on the landmark's prior (see the camera part): the quad's four lanes share a wave
      const uint32_t wf = b.lmk_wflag[l];
      if (wf >= 1u && wf <= 5u) {
        const float sc = b.lmk_scale[l];
        acc.x *= sc; acc.y *= sc; acc.z *= sc; acc.w *= sc;
        b.lmk_prior_rw[(size_t)l * 4 + q] = acc;
        if (q == 0) b.lmk_wflag[l] = wf - 1u;
      }
    }
    // the mean the last sweep used (roll: the current one becomes it) goes out with the first round of loads: fetched where it
    // is consumed — behind the gathers — it was a third dependent round trip of every wave
    if (b.hoist && q == 0) used_mu = b.lmk_mu[(size_t)l * 2 + (b.roll ? 0 : 1)];
  }
  const uint32_t deg = (uint32_t)__shfl((int)ix.x, 0, 4);
  acc = lmk_quad_dense(acc, q);     // the sums run on the dense image of the messages (see lmsg_load)
  {
    // element k + 1 of the index record sits in lane (k + 1) / 4, component (k + 1) % 4 of the quad
    auto slot_pos = [&](int k) -> uint32_t {
      const uint32_t v = ((k + 1) & 3) == 0 ? ix.x : ((k + 1) & 3) == 1 ? ix.y : ((k + 1) & 3) == 2 ? ix.z : ix.w;
      return (uint32_t)__shfl((int)v, (k + 1) >> 2, 4);
    };
    // Ten gathers in flight, then (only where a landmark of the wave has more than ten factors) the other five: 40
    // instead of 60 staging registers (1M-factor graph: k_beliefs 20.4 -> 18.8 us).
    float4 m[10];
    GBP_UNROLL
    for (int k = 0; k < 10; ++k) m[k] = lmsg_load(b.lmsg, slot_pos(k), q);      // all ten in flight (see lmsg_load)
    GBP_UNROLL
    for (int k = 0; k < 10; ++k) {   // adds in slot order
      const float4 v = m[k];
      if ((uint32_t)k < deg) lmk_acc_add(acc, v);
    }
    if (__any(deg > 10u)) {
      GBP_UNROLL
      for (int k = 10; k < 15; ++k) m[k - 10] = lmsg_load(b.lmsg, slot_pos(k), q);
      GBP_UNROLL
      for (int k = 10; k < 15; ++k) {
        const float4 v = m[k - 10];
        if ((uint32_t)k < deg) lmk_acc_add(acc, v);
      }
    }
  }
  if (deg > 15u) {   // slots 16.. : positions from lmk_fpos, 8 record gathers in flight per round, adds in slot order
    const uint32_t s1 = b.lmk_ptr[l + 1];
    for (uint32_t s = b.lmk_ptr[l] + 15u; s < s1; s += 8) {
      uint32_t pos[8];
      float4 m[8];
      const uint32_t nleft = s1 - s;
      GBP_UNROLL
      for (int k = 0; k < 8; ++k) pos[k] = b.lmk_fpos[(uint32_t)k < nleft ? s + k : s1 - 1u];     // clamped, unconditional
      GBP_UNROLL
      for (int k = 0; k < 8; ++k) m[k] = lmsg_load(b.lmsg, pos[k], q);
      GBP_UNROLL
      for (int k = 0; k < 8; ++k) {
        const float4 v = m[k];
        if ((uint32_t)k < nleft) { acc.x = acc.x + v.x; acc.y = acc.y + v.y; acc.z = acc.z + v.z; acc.w = acc.w + v.w; }
      }
    }
  }
  acc = lmk_quad_record(acc, q);
  if (b.hoist) {
    // gather the 16-float record of the quad into its lane 0 (all lanes execute the shuffles)
    float rec[16];
    GBP_UNROLL
    for (int k = 0; k < 4; ++k) {
      rec[4 * k] = __shfl(acc.x, k, 4); rec[4 * k + 1] = __shfl(acc.y, k, 4);
      rec[4 * k + 2] = __shfl(acc.z, k, 4); rec[4 * k + 3] = __shfl(acc.w, k, 4);
    }
    float u[3] = {0.f, 0.f, 0.f};
    if (live && q == 0) {
      float x0l[3];
      lmk_mean(rec, x0l);
      float4* mu = b.lmk_mu + (size_t)l * 2;  // [0] = mean of the current belief, [1] = mean the last sweep used
      const float4 used = used_mu;
      if (b.roll) mu[1] = used;
      lmk_dmu2(used, x0l, u);
      mu[0] = make_float4(x0l[0], x0l[1], x0l[2], 0.f);
      if (EV) {   // the belief (eta 3, Lambda 9) for the metric below
        GBP_UNROLL
        for (int i = 0; i < 3; ++i) lrec[threadIdx.x >> 2][i] = rec[i];
        GBP_UNROLL
        for (int i = 0; i < 9; ++i) lrec[threadIdx.x >> 2][3 + i] = rec[4 + i];
      }
    }
    if (EV) {
      // The landmarks' metric means (what k_means computes: fp64 pivoted solve, LDL^T pivots) — long fp64 chains that one lane
      // in four would run at a quarter of the wave's width in each of the four waves: the 64 landmarks of the workgroup meet in
      // LDS and ONE wave solves them, all lanes busy (k_beliefs<EV> 18.6 -> measured in profiles/r05_default_loop.md).
      __syncthreads();
      if (threadIdx.x < 64) {
        const uint32_t le = lb * 64 + threadIdx.x;
        if (le < b.n_lmks) {
          float r12[12], x[3];
          GBP_UNROLL
          for (int i = 0; i < 12; ++i) r12[i] = lrec[threadIdx.x][i];
          solve_pivot<3>(r12 + 3, 3, r12, x);
          bool finite = true;
          GBP_UNROLL
          for (int i = 0; i < 3; ++i) finite &= (x[i] - x[i] == 0.f);
          b.ev.lmk_mean[le] = make_float4(x[0], x[1], x[2], 0.f);
          if (!finite) atomicAdd(&b.ev.health[0], 1ull);
          if (!ldl_pivots_positive<3>(r12 + 3, 3)) atomicAdd(&b.ev.health[1], 1ull);
        }
      }
    }
    const float u0 = __shfl(u[0], 0, 4), u1 = __shfl(u[1], 0, 4), u2 = __shfl(u[2], 0, 4);
    if (q == 0) acc.w = u0;                       // record slot 3
    if (q == 3) { acc.y = u1; acc.z = u2; }       // record slots 13, 14
  }
  if (live) b.lmkb[(size_t)l * 4 + q] = acc;
}
__global__ __launch_bounds__(256) void k_beliefs(const BeliefArgs b) { beliefs_body<false>(b); }      // (held at 8 waves per SIMD: S1 +0.1 %, config-5 shape +0.2 %: noise — profiles/HISTORY.md)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_beliefs_cam(const BeliefArgs b) { beliefs_body<false, true>(b); }
__global__ __launch_bounds__(256) void k_beliefs_ev(const BeliefArgs b) { beliefs_body<true>(b); }
// The camera combine of a sharded iteration that carries the metric (behind the exchange; BeliefArgs.ev_split): each camera's metric record
// from the finished belief.  Not pinned at 8 waves per SIMD like k_beliefs_cam: the fp64 tableau of the metric's solve would spill there
// (see the EV block of beliefs_body), so the compiler chooses — resources in profiles/sharded_metric.md.
__global__ __launch_bounds__(256) void k_beliefs_cam_ev(const BeliefArgs b) { beliefs_body<true, true>(b); }
// The direct peer-memory exchange.  The peers' partials were written by kernels of OTHER processes, whose completion the
// host has observed before the region barrier that let this launch be enqueued; the system-scope acquire in front of the first peer
// access drops whatever stale copy of those lines this agent's caches still hold (the read of two exchanges ago, same parity).
// No flags, no waits on another process inside a kernel.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_beliefs_cam_peers(const BeliefArgs b,
                                                                                                     const float* const* __restrict__ peers) {
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
  beliefs_body<false, true, true>(b, peers);
}
__global__ __launch_bounds__(256) void k_beliefs_cam_peers_ev(const BeliefArgs b, const float* const* __restrict__ peers) {
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
  beliefs_body<true, true, true>(b, peers);
}
// dst[r] = peers[r] for every rank r != self, 16 bytes per lane (a camera record is 11 float4); grid.y = rank
__global__ __launch_bounds__(256) void k_gather_peers(const float* const* __restrict__ peers, float* __restrict__ dst, uint32_t n4,
                                                      int self) {
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
  const uint32_t r = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if ((int)r == self || i >= n4) return;
  reinterpret_cast<float4*>(dst)[(size_t)r * n4 + i] = reinterpret_cast<const float4*>(peers[r])[i];
}
// The sliced peer-memory exchange (p2p-slices): the camera sums and the chain behind them run ONCE per camera, on the rank
// that owns the camera's slice (slice_bounds), and only the finished records travel.
//   k_beliefs_cam_slice   the reduce: k_beliefs_cam_peers over the cameras of this rank's slice — partial r of those cameras straight from
//                         peers[r], the same additions in rank order, the same means and CAM_LIN — into this rank's tables AND into its
//                         result buffer (record c - lo of the parity)
//   k_gather_slices       the gather: the records of every OTHER slice out of their owners' result buffers (results[s], IPC mappings) into
//                         this rank's CAMB, hoisted means and CAM_LIN: what the reduce left on the owner, so what k_beliefs_cam_peers would
//                         have computed here.  grid.y = owner rank, 16 bytes per lane.  "Means used by the last sweep" := this rank's own
//                         current means (roll), which equal the owner's: every rank held the same tables before the exchange.
// Both begin with the acquire of the peer readers above; neither waits on another process.
static_assert(kCamLin4 == 5 && kCamRes4 == kCamRec4 + 2 + kCamLin4, "result record: belief 11 + mean 2 + CAM_LIN 5 float4");
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_beliefs_cam_slice(const BeliefArgs b,
                                                                                                     const float* const* __restrict__ peers,
                                                                                                     const CamSlice sl) {
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
  beliefs_body<false, true, true, true>(b, peers, sl);
}
__global__ __launch_bounds__(256) void k_gather_slices(const float4* const* __restrict__ results, float4* __restrict__ camb,
                                                       float4* __restrict__ cam_mu, float4* __restrict__ cam_lin, uint32_t n_cams, int world,
                                                       int self, int hoist, int roll) {
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
  const int s = (int)blockIdx.y;
  if (s == self) return;
  uint32_t lo, hi;
  slice_bounds(n_cams, world, s, &lo, &hi);
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= (hi - lo) * (uint32_t)kCamRes4) return;
  const uint32_t c = lo + i / (uint32_t)kCamRes4, k = i % (uint32_t)kCamRes4;
  if (k >= (uint32_t)kCamRec4 && !hoist) return;      // no hoisted tables on this ctx: the owner wrote none
  const float4 v = results[s][i];
  if (k < (uint32_t)kCamRec4) {
    camb[(size_t)c * kCamRec4 + k] = v;
  } else if (k < (uint32_t)kCamRec4 + 2u) {
    float4* mu = cam_mu + (size_t)c * 4 + (k - kCamRec4);
    if (roll) mu[2] = mu[0];
    mu[0] = v;
  } else {
    cam_lin[(size_t)c * kCamLin4 + (k - kCamRec4 - 2u)] = v;
  }
}

void launch_beliefs(BeliefArgs b, bool do_cam, bool do_lmk, hipStream_t s, bool ev) {
  b.cam_blocks = do_cam ? (b.n_cams + 3) / 4 : 0;
  const uint32_t lmk_blocks = do_lmk ? blocks_for((uint64_t)b.n_lmks * 4) : 0;
  b.lmk_blocks = lmk_blocks;
  if (b.cam_blocks + lmk_blocks == 0) return;
  if (ev && lmk_blocks == 0) hipLaunchKernelGGL(k_beliefs_cam_ev, dim3(b.cam_blocks), dim3(256), 0, s, b);
  else if (ev) hipLaunchKernelGGL(k_beliefs_ev, dim3(b.cam_blocks + lmk_blocks), dim3(256), 0, s, b);
  else if (lmk_blocks == 0) hipLaunchKernelGGL(k_beliefs_cam, dim3(b.cam_blocks), dim3(256), 0, s, b);
  else hipLaunchKernelGGL(k_beliefs, dim3(b.cam_blocks + lmk_blocks), dim3(256), 0, s, b);
}
void launch_beliefs_cam_peers(BeliefArgs b, const float* const* peers, hipStream_t s, bool ev) {
  b.cam_blocks = (b.n_cams + 3) / 4;
  b.lmk_blocks = 0;
  b.gathered = nullptr;
  if (b.cam_blocks == 0) return;
  if (ev) hipLaunchKernelGGL(k_beliefs_cam_peers_ev, dim3(b.cam_blocks), dim3(256), 0, s, b, peers);
  else hipLaunchKernelGGL(k_beliefs_cam_peers, dim3(b.cam_blocks), dim3(256), 0, s, b, peers);
}
void launch_gather_peers(const float* const* peers, float* dst, uint32_t n4, int world, int self, hipStream_t s) {
  if (n4 == 0 || world < 2) return;
  hipLaunchKernelGGL(k_gather_peers, dim3((n4 + 255) / 256, (uint32_t)world), dim3(256), 0, s, peers, dst, n4, self);
}
void launch_beliefs_cam_slice(BeliefArgs b, const float* const* peers, const CamSlice& sl, hipStream_t s) {
  b.cam_blocks = (sl.hi - sl.lo + 3) / 4;
  b.lmk_blocks = 0;
  b.gathered = nullptr;
  if (sl.hi <= sl.lo) return;      // an empty slice (fewer cameras than ranks)
  hipLaunchKernelGGL(k_beliefs_cam_slice, dim3(b.cam_blocks), dim3(256), 0, s, b, peers, sl);
}
void launch_gather_slices(const float4* const* results, const BeliefArgs& b, int self, hipStream_t s) {
  if (b.n_cams == 0 || b.world < 2) return;
  const uint32_t widest = (b.n_cams + (uint32_t)b.world - 1) / (uint32_t)b.world;      // no slice holds more cameras (slice_bounds)
  hipLaunchKernelGGL(k_gather_slices, dim3((widest * kCamRes4 + 255) / 256, (uint32_t)b.world), dim3(256), 0, s, results,
                     reinterpret_cast<float4*>(b.camb), b.cam_mu, b.cam_lin, b.n_cams, b.world, self, b.hoist, b.roll);
}

}  // namespace gbp
