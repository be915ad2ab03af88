// kernels/gbp_persist_support.hpp — what the persistent kernels are made of: the sc1 buffer view of an array that crosses waves
// inside a launch, the counter barrier, the placement rule, a tile wave's register state and the bounded waits on tagged records.
// Device helpers only; used by k_persist_flow (gbp_persist.hip), by the barrier kernel k_persist of the test-hooks build
// (hooks/gbp_persist_barrier.hip) and by the flow-torture hook.
#pragma once
#include "gbp_tile.hpp"      // load_tile / store_tile, lmsg_tile_in, lmsg_quad_i4
#include "gbp_vertex.hpp"    // cmsg_expand, cmsg_pack

namespace gbp {
using namespace gbpdev;

// =================================================================================================
// k_persist: n iterations of {k_sweep; k_beliefs} in ONE launch, for graphs whose workgroups are all resident at once.
//
// A graph of a few thousand factors (BASELINE configs 1-3: fr1xyz = 204 wavefronts on 1 024 SIMDs) is bound by what
// happens BETWEEN its kernels: a dependent launch costs ~3.5 us on this stack and every kernel starts with cold L2s
// (profiles/r03_small_graphs.md), while the arithmetic of a whole iteration is ~10 us.  Here the iteration loop lives
// inside the kernel:
//   phase A  wave w sweeps tile w with factor_update() — the same per-lane arithmetic as k_sweep; the factor's
//            potential and both of its messages stay in REGISTERS across iterations (FAC / CMSG are written back once,
//            after the last iteration); the landmark-message tile and the row sums go to memory for phase B;
//   barrier  device-wide (grid_sync below);
//   phase B  wave w owns camera w, or 16 landmarks (4 lanes each) — the arithmetic of k_beliefs; row pointers, the
//            landmark index record and the priors stay in registers, so the phase is ONE round of loads;
//   barrier  (not after the last iteration).
// Results are bit-identical to the two-kernel path (same per-lane operations in the same order); every array the other
// kernels and the C-ABI read (FAC, CMSG, LMSG, ROWP, CAMB, LMKB, the hoisted means, cam_local) is left exactly as n
// launches of k_sweep + k_beliefs leave it.  Hoisted means only (gbp_params.per_factor_mu = 0), single-GPU ctx only.
// =================================================================================================
// Device-wide hand-off without cache maintenance.  The 8 XCDs have private, mutually incoherent L2s; the textbook grid
// barrier (release: write the L2 back, acquire: invalidate it) costs 5.5 us for 51 workgroups on this chip — more than
// the 3.7 us of a kernel boundary (profiles/r03_small_graphs.md).  Instead every access to the arrays that cross waves
// inside the launch (LMSG, ROWP, CAMB, LMKB, the hoisted means) is an agent-scope relaxed atomic: stores are written
// through to memory, loads are re-fetched (global_load/store_dwordx2 ... sc1), so the barrier itself only has to wait for
// this wave's stores (s_waitcnt vmcnt(0)), meet the workgroup, and count one arrival per workgroup: 1.4 us for 51
// workgroups.  The counter only grows (epoch e expects e * n arrivals); the host zeroes it before the launch.  The wait
// is bounded: if a workgroup were not resident (the launcher checks occupancy, so it is) the kernel raises *status and
// carries on instead of hanging the GPU.
// An array that crosses waves inside the launch ("xw"): every access is sc1 — through a buffer descriptor, because the
// buffer intrinsics give 16-byte sc1 accesses the compiler tracks (agent-scope atomics stop at 8 bytes, and 8-byte accesses
// move at 0.54-0.70x the 16-byte rate, MI355X_MICROARCH.md).  Offsets are 32-bit: arrays below 4 GiB, which the size limit of
// k_persist guarantees by a factor of a thousand.
// VER (test-hooks builds only, gbp_debug_persist_verify): every record is published TWICE — the record itself and, `mirror4` float4
// further on, a copy with the payload words complemented and the same tag — and a load hands a record to its consumer only once BOTH
// copies carry the same tag (until then the record reads as "not arrived": tag 0, the consumer keeps polling); the two payloads must
// then be bit-wise complements, or the load counts a mismatch in *verr.  A torn or stale 16-byte record, which the product's consumers
// could not tell from a good one, shows up as such a mismatch (tests/test_gpu_parity.py: test_persistent_kernel_redundant_records).
template <bool VER>
struct XwBufT {
  __amdgpu_buffer_rsrc_t r;
  uint32_t mirror4 = 0;
  unsigned long long* verr = nullptr;
  // soff: byte offset of this array inside the allocation the descriptor covers — the scalar offset operand of the buffer instructions,
  // an add the address unit does for nothing (and which its range check ignores: kNone4 stays out of range).  k_persist_flow describes
  // its nine shadows, which live in ONE allocation, with one descriptor + nine such offsets instead of nine descriptors: 23 fewer
  // live SGPRs in a kernel that spills them (profiles/r06_resources.md)
  uint32_t soff = 0;
  GBP_DEV explicit XwBufT(const void* base, uint32_t mirror4_ = 0, unsigned long long* verr_ = nullptr, uint32_t soff_ = 0)
      : r(__builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000)), mirror4(mirror4_), verr(verr_), soff(soff_) {}
  static constexpr int kSc1 = 16;        // cache-policy bit of the gfx94x / gfx950 buffer instructions
  typedef unsigned v4u __attribute__((ext_vector_type(4)));
  GBP_DEV float4 ld4(uint32_t i4) const {   // float4 #i4 of the array
    const v4u v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)(i4 * 16u), (int)soff, kSc1);
    if (VER) {
      if (mirror4 != 0u && i4 < kNone4) {
        const v4u m = __builtin_amdgcn_raw_buffer_load_b128(r, (int)((i4 + mirror4) * 16u), (int)soff, kSc1);
        if (m.w != v.w) return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), 0.f);      // one copy has not arrived yet
        if ((m.x != ~v.x || m.y != ~v.y || m.z != ~v.z) && v.w != 0u) atomicAdd(verr, 1ull);
      }
    }
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
  }
  // float4 #kNone4 lies beyond the descriptor's range (0x7fffffff bytes): the hardware returns zeros WITHOUT a memory access — what a
  // slot that is not needed loads (a clamped duplicate would be one more trip through the fabric; a conditional load a branch)
  static constexpr uint32_t kNone4 = 0x0fffffffu;
  GBP_DEV void st4(uint32_t i4, const float4 v) const {
    const v4u x = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
    __builtin_amdgcn_raw_buffer_store_b128(x, r, (int)(i4 * 16u), (int)soff, kSc1);
    if (VER) {
      if (mirror4 != 0u) {
        const v4u y = {~x.x, ~x.y, ~x.z, x.w};
        __builtin_amdgcn_raw_buffer_store_b128(y, r, (int)((i4 + mirror4) * 16u), (int)soff, kSc1);
      }
    }
  }
  // (the b32 intrinsics are typed unsigned: bit casts, not value conversions)
  GBP_DEV float ld1(uint32_t i) const { return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)(i * 4u), (int)soff, kSc1)); }
  GBP_DEV void st1(uint32_t i, const float v) const { __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, (int)(i * 4u), (int)soff, kSc1); }
};
using XwBuf = XwBufT<false>;
template <int G>
GBP_DEV void load_rec_xw(const XwBuf& buf, uint32_t i4, float (&out)[G * 4]) {
  GBP_UNROLL
  for (int g = 0; g < G; ++g) {
    const float4 v = buf.ld4(i4 + (uint32_t)g);
    out[4 * g] = v.x; out[4 * g + 1] = v.y; out[4 * g + 2] = v.z; out[4 * g + 3] = v.w;
  }
}
GBP_DEV float4 lmsg_piece_xw(const XwBuf& lmsg, uint32_t pos, uint32_t q) { return lmsg.ld4(lmsg_quad_i4(pos, q)); }      // (see lmsg_load)

constexpr unsigned long long kBarrierTimeoutTicks = 150000000ull;   // 1.5 s of the 100 MHz wall clock
// The hand-off in two halves, so that work which needs nothing from the other workgroups can run between the arrival and the
// wait (the metric's residuals of the previous iteration: they then cost nothing while the arrivals are in flight).
GBP_DEV void grid_arrive(unsigned* sync) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's write-through stores have been acknowledged
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_fetch_add(sync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
GBP_DEV void grid_wait(unsigned* sync, unsigned target /* arrivals to wait for */, unsigned* status, unsigned seq /* what a time-out writes to *status */) {
  if (threadIdx.x == 0) {
    unsigned spin = 0;
    unsigned long long t0 = 0;
    while ((int)(__hip_atomic_load(sync, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0) {   // wrap-safe
      // bounded wait (1.5 s by the wall clock), and once ONE workgroup has given up every other one leaves its barriers at once
      // (sync[32] is the abort word): a launch that can never complete ends in seconds with *status raised, it does not hang
      // the GPU.  The abort word stays set: later launches of the ctx return at once (k_persist prologue) until the host has
      // restored the state the failed launch started from (gbp_api_persist.cpp: persist_recover).
      if ((++spin & 255u) == 0u) {
        const unsigned long long now = wall_clock64();
        if (t0 == 0) t0 = now;
        if (now - t0 > kBarrierTimeoutTicks || __hip_atomic_load(sync + 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
          if (__hip_atomic_exchange(sync + 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) *status = seq;   // the first to give up names the launch
          break;
        }
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  __syncthreads();
}
GBP_DEV void grid_sync(unsigned* sync, unsigned target, unsigned* status, unsigned seq) {
  grid_arrive(sync);
  grid_wait(sync, target, status, seq);
}

// ---- what the two persistent kernels (k_persist, k_persist_flow) share ----
// placement (profiles/r03_small_graphs.md): the grid is `spread` times larger than the work; filler workgroups leave at once.
// spread > 0: workgroup b works iff b % spread == 0;  spread < 0 (s = -spread): iff (b / 8) % s == 0 (every XCD keeps working,
// every s-th dispatch slot inside an XCD).  false: a filler; true: workgroup bid of the nblk working ones
GBP_DEV bool persist_place(const PersistArgs& A, uint32_t& bid, uint32_t& nblk) {
  bid = blockIdx.x; nblk = gridDim.x;
  if ((int)A.spread > 1) {
    if (blockIdx.x % A.spread) return false;
    bid = blockIdx.x / A.spread; nblk = gridDim.x / A.spread;
  } else if ((int)A.spread < -1) {
    const uint32_t sp = (uint32_t)(-(int)A.spread), slot = blockIdx.x >> 3;
    if (slot % sp) return false;
    bid = (slot / sp) * 8 + (blockIdx.x & 7u); nblk = A.n_work_blocks;
    if (bid >= nblk) return false;
  }
  return true;
}
// The tagged landmark messages of k_persist_flow (PersistFlow.lmsg: four 16-byte records per factor) through the wave's LDS stage:
// piece q of record r sits at float4 slot r*4 + (q ^ swz(r)), swz(r) = ((r>>2)&3) ^ (r&2) — a permutation inside each 64-B record,
// so the tile-order accesses (whole records) and the record-order accesses (one piece per lane) are both bank-conflict-free for
// ds_read_b128 (16-lane groups, 64 banks) and ds_write_b128 (8-lane groups, 32 banks).
// Out: `piece(q)` is float4 #q of the lane's record; `st(k, v)` stores the lane's float4 of the k-th coalesced access.
template <class Piece, class St>
GBP_DEV void lm_tile_out(float4* stage, uint32_t lane, Piece&& piece, St&& st) {
  const uint32_t rec_t = lane >> 2, swz_own = ((lane >> 2) & 3u) ^ (lane & 2u);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  GBP_UNROLL
  for (int q = 0; q < 4; ++q) stage[lane * 4 + ((uint32_t)q ^ swz_own)] = piece((uint32_t)q);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  GBP_UNROLL
  for (int k = 0; k < 4; ++k) {
    const uint32_t r = k * 16 + rec_t;
    st((uint32_t)k, stage[r * 4 + ((lane & 3u) ^ (((r >> 2) & 3u) ^ (r & 2u)))]);
  }
}
// A tile wave's registers for the whole launch: the potential, the camera messages and — `ld_lm(i4)` = float4 #i4 of LMSG — the
// landmark messages of tile `tile` with the factor's scalars in the pad slots of their register image (gbp_kernels.h).  The camera message stays LITERAL in registers across the iterations: cmsg_expand of the CMSG
// record once, then each iteration's output; its record is written by the launch's last iteration (tile_cmsg_store)
template <class LdLm>
GBP_DEV void tile_regs_load(const SweepArgs& a, uint32_t tile, uint32_t lane, float4* stage, LdLm&& ld_lm, float (&fac)[56], float (&cm)[28],
                            float (&lm)[16]) {
  load_tile<kFacG, false>(a.fac, tile, lane, fac);
  float rec[16];
  load_tile<kCmsgG, false>(a.cmsg, tile, lane, rec);
  cmsg_expand(fac, rec, a.cmsg_lit, tile, lane, cm);
  const uint32_t p = tile * 64u + lane;
  lm[3] = a.fst_damp[p]; lm[13] = __int_as_float(a.fst_packed[p]); lm[14] = a.fst_var[p]; lm[15] = 0.f;
  lmsg_tile_in(stage, lane, [&](uint32_t k) { return ld_lm(tile * (uint32_t)(64 * kLmsgG) + k * 64u + lane); }, lm);
}
// behind factor_update: the factor's scalar state into the pad slots of its new landmark message ol; both new messages become the
// registers the next iteration starts from
GBP_DEV void tile_regs_refresh(float (&ol)[16], const float (&oc_eta)[6], const float (&oc_lam)[36], float damping, int count, uint32_t flags,
                               float var, float (&lm)[16], float (&cm)[28]) {
  ol[3] = damping;
  ol[13] = __int_as_float((int)(((uint32_t)count << 3) | flags));
  ol[14] = var;
  GBP_UNROLL
  for (int i = 0; i < 16; ++i) lm[i] = ol[i];
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) cm[i] = oc_eta[i];
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) {
    GBP_UNROLL
    for (int j = 0; j <= i; ++j) cm[6 + tri(i, j)] = oc_lam[i * 6 + j];
  }
  cm[27] = 0.f;
}
// behind the factor_update of the launch's LAST iteration, where the 3x3 inverse of the new camera message is at hand: the CMSG record
// the launch leaves (nobody reads the records of the iterations before it: their messages live in cm)
GBP_DEV void tile_cmsg_store(const SweepArgs& a, uint32_t tile, uint32_t lane, const float (&oc_eta)[6], const float (&bi)[9], bool active) {
  float rec[16];
  cmsg_pack(oc_eta, bi, active, rec);
  store_tile<kCmsgG, false>(a.cmsg, tile, lane, rec);
}
// what stayed in registers goes back to its arrays: the potential where a lane relinearised, the two mutable state planes (lm: the
// register image the last iteration left)
GBP_DEV void tile_regs_store(const SweepArgs& a, uint32_t tile, uint32_t lane, const float (&fac)[56], bool fac_dirty, const float (&lm)[16]) {
  if (fac_dirty) store_tile<kFacG, false>(a.fac, tile, lane, fac);
  const uint32_t p = tile * 64u + lane;
  a.fst_packed[p] = __float_as_int(lm[13]);
  a.fst_damp[p] = lm[3];
}

GBP_DEV bool flow_give_up(unsigned spin, unsigned long long& t0, unsigned* sync, unsigned* status, unsigned seq) {
  if ((spin & 255u) != 255u) return false;
  const unsigned long long now = wall_clock64();
  if (t0 == 0) t0 = now;
  if (now - t0 > kBarrierTimeoutTicks || __hip_atomic_load(sync + 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
    if (__hip_atomic_exchange(sync + 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) *status = seq;
    return true;
  }
  return false;
}
// `attempt()` issues a round of loads and says per lane whether everything it needs has arrived; true once every lane says so
// (a waiting wave re-loads through the fabric — sc1 loads miss the L2 by design: between two rounds it sleeps, and where a round is
// many records per lane it first polls ONE of them, `probe`, the one its producer writes last; 200 waves re-loading 30 records per
// lane flat out were 5 TB/s of polling and made fr1xyz 2 us per iteration SLOWER than the barriers)
template <class Attempt>
GBP_DEV bool flow_wait(Attempt&& attempt, unsigned* sync, unsigned* status, unsigned seq) {
  unsigned long long t0 = 0;
  for (unsigned spin = 0;; ++spin) {
    asm volatile("" ::: "memory");      // the loads are re-issued every time round
    if (__all(attempt())) return true;
    if (flow_give_up(spin, t0, sync, status, seq)) return false;
    __builtin_amdgcn_s_sleep(2);
  }
}
GBP_DEV float4 flow_rec(float x, float y, float z, unsigned tag) { return make_float4(x, y, z, __uint_as_float(tag)); }
GBP_DEV bool flow_is(const float4 v, unsigned tag) { return __float_as_uint(v.w) == tag; }
GBP_DEV float flow_pick(const float4 v, uint32_t c) { return c == 0u ? v.x : c == 1u ? v.y : v.z; }
// payload slot k (0 .. 29) of the tagged camera belief -> float of the 44-float CAMB record (eta 0..5, S, lower triangle row-wise)
GBP_DEV uint32_t flow_camb_src(uint32_t k) {
  if (k < 7u) return k;
  if (k >= 28u) return 0u;
  const uint32_t t = k - 7u;
  uint32_t i = 0;
  while ((i + 1u) * (i + 2u) / 2u <= t) ++i;
  return 8u + i * 6u + (t - i * (i + 1u) / 2u);
}

}  // namespace gbp
