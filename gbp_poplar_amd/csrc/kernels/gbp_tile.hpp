// kernels/gbp_tile.hpp — tile and record access: how a wave moves a tile of per-factor records, a variable's record, the 16-lane
// row sums of the camera messages and a wave's landmark messages between memory, LDS and registers.  Device helpers (all GBP_DEV,
// no kernel) and, at the end, blocks_for: the one host helper the launchers of several units share.  Every kernel unit and the
// vertex / persistent-kernel helpers build on this header.
#pragma once
#include "../gbp_kernels.h"
#include "../gbp_device_math.hpp"

namespace gbp {
using namespace gbpdev;

// The per-factor tiles are touched exactly once per sweep: stream them with the non-temporal hint so that
// they do not displace the gathered tables (landmark messages / beliefs, camera beliefs: ~70 MB for S1)
// from L2 and the 256 MiB Infinity Cache.
typedef float v4f __attribute__((ext_vector_type(4)));
template <int G, bool NT = true>
GBP_DEV void load_tile(const float4* base, uint32_t tile, uint32_t lane, float (&out)[G * 4]) {
  const v4f* p = reinterpret_cast<const v4f*>(base) + (size_t)tile * G * 64 + lane;
  GBP_UNROLL
  for (int g = 0; g < G; ++g) {
    const v4f v = NT ? __builtin_nontemporal_load(p + g * 64) : p[g * 64];
    out[4 * g] = v.x; out[4 * g + 1] = v.y; out[4 * g + 2] = v.z; out[4 * g + 3] = v.w;
  }
}
template <int G, bool NT = true>
GBP_DEV void store_tile(float4* base, uint32_t tile, uint32_t lane, const float (&in)[G * 4]) {
  v4f* p = reinterpret_cast<v4f*>(base) + (size_t)tile * G * 64 + lane;
  GBP_UNROLL
  for (int g = 0; g < G; ++g) {
    const v4f v = {in[4 * g], in[4 * g + 1], in[4 * g + 2], in[4 * g + 3]};
    if (NT) __builtin_nontemporal_store(v, p + g * 64); else p[g * 64] = v;
  }
}
// SEG (k_sweep<..., SEG = true>): the same tile accesses through a buffer descriptor that covers exactly this tile's G KiB, so that
// a lane whose 64-byte segment (four lanes) holds PAD positions only can be given an offset beyond the descriptor's range: the
// hardware then returns zeros for a load and drops a store WITHOUT a memory access — no branch, no divergence, and the all-pad
// segments (the unused tail of a camera's last row: 3.7 % of the positions on the config-5 shard shape) are never streamed in or
// out.  Measured on that shape: 839 -> 813 MB per ordinary sweep (reads only drop where BOTH halves of a 128-byte line are empty,
// writes per 64 bytes), 0.1551 -> 0.1532 ms per iteration (profiles/r06_configs.md).  aux: 2 = the non-temporal hint of the gfx94x / gfx950 buffer instructions.
constexpr int kBufOob = 0x40000000;      // beyond every tile descriptor (<= 14 KiB), and + g KiB does not wrap
template <int G>
GBP_DEV __amdgpu_buffer_rsrc_t tile_rsrc(const float4* base, uint32_t tile) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float4*>(base) + (size_t)tile * G * 64, 0, G * 1024, 0x00020000);
}
template <int G, bool NT = true>
GBP_DEV void load_tile_seg(const float4* base, uint32_t tile, uint32_t lane, bool live, float (&out)[G * 4]) {
  typedef unsigned v4u __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t r = tile_rsrc<G>(base, tile);
  const int off = live ? (int)(lane * 16u) : kBufOob;
  GBP_UNROLL
  for (int g = 0; g < G; ++g) {
    const v4u v = __builtin_amdgcn_raw_buffer_load_b128(r, off + g * 1024, 0, NT ? 2 : 0);
    out[4 * g] = __uint_as_float(v.x); out[4 * g + 1] = __uint_as_float(v.y); out[4 * g + 2] = __uint_as_float(v.z); out[4 * g + 3] = __uint_as_float(v.w);
  }
}
template <int G, bool NT = true>
GBP_DEV void store_tile_seg(float4* base, uint32_t tile, uint32_t lane, bool live, const float (&in)[G * 4]) {
  typedef unsigned v4u __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t r = tile_rsrc<G>(base, tile);
  const int off = live ? (int)(lane * 16u) : kBufOob;
  GBP_UNROLL
  for (int g = 0; g < G; ++g) {
    const v4u v = {__float_as_uint(in[4 * g]), __float_as_uint(in[4 * g + 1]), __float_as_uint(in[4 * g + 2]), __float_as_uint(in[4 * g + 3])};
    __builtin_amdgcn_raw_buffer_store_b128(v, r, off + g * 1024, 0, NT ? 2 : 0);
  }
}
template <int G>
GBP_DEV void load_rec(const float4* rec, float (&out)[G * 4]) {
  GBP_UNROLL
  for (int g = 0; g < G; ++g) {
    const float4 v = rec[g];
    out[4 * g] = v.x; out[4 * g + 1] = v.y; out[4 * g + 2] = v.z; out[4 * g + 3] = v.w;
  }
}

// LDS-DMA (global_load_lds_dword / _dwordx4, the gfx950 b128 form): every lane names its own SOURCE address, the data lands at
// dst + lane * BYTES — dst is wave-uniform — without passing through a register, so a request costs the prologue no live VGPR
// beyond its address.  Nothing orders a later ds_read behind the transfer but the issuing wave's own vmcnt: lds_dma_wait() goes
// in front of the first read.
template <int BYTES>
GBP_DEV void lds_dma(const void* src, void* dst) {
  static_assert(BYTES == 4 || BYTES == 16, "global_load_lds: dword or dwordx4");
  const auto* g = (const __attribute__((address_space(1))) void*)src;
  auto* l = (__attribute__((address_space(3))) void*)dst;
  if (BYTES == 16) __builtin_amdgcn_global_load_lds(g, l, 16, 0, 0);      // (the size is a literal: the builtin takes no dependent value)
  else __builtin_amdgcn_global_load_lds(g, l, 4, 0, 0);
}
// ... the same from a table of records: lane's source = record `index` of the table + `byte` (a multiple of 16 below the stride).  The
// hardware scales the index by the stride of the descriptor, so the request needs no address arithmetic in vector registers.
GBP_DEV __amdgpu_buffer_rsrc_t rec_rsrc(const float4* table, int stride_bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float4*>(table), (short)stride_bytes, 0x7fffffff, 0x00020000);
}
GBP_DEV void lds_dma_rec16(__amdgpu_buffer_rsrc_t table, uint32_t index, int byte, void* dst) {
  __builtin_amdgcn_struct_ptr_buffer_load_lds(table, (__attribute__((address_space(3))) void*)dst, 16, (int)index, 0, byte, 0, 0);
}
GBP_DEV void lds_dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// The 44-float ROWP record of every 16-lane row of a tile: the sums of the camera messages (6 eta + 36 Lambda entries, two
// pad slots) over the row's 16 factors, each the balanced binary tree in lane order of row16_sum, handed to `st(g, float4)`
// (float4 group g of the row's record) by the lanes that end up holding them.
//
// A butterfly that leaves all 42 sums in all 16 lanes costs 4 x 42 tree nodes, each evaluated by sixteen lanes, as v_mov_b32_dpp +
// (packed) v_add: 252 instructions.  Here a node is ONE v_add_f32 with a DPP operand, and the two intra-quad steps HALVE the
// set a lane carries (lane%4 = q ends up with the float4 groups g = q, q+4, q+8 of the record): the partners of a step keep
// different halves, each sends the half the other keeps (two selects per pair of values), so the steps cost 60 + 36 + 12 +
// 12 = 120 instructions and the record leaves in three stores of 64 contiguous bytes per row (lanes 12..15) instead of
// eleven 16-byte ones (lane 0).  Every node adds the same two operands as the butterfly's ((x0+x1)+(x2+x3)) + ..., own +
// partner, commutative: the same bits.
//   step 1 (lane ^ 1): even lanes keep groups {0,2} mod 4, odd lanes groups {1,3} mod 4      -> t[2k], t[2k+1]
//   step 2 (lane ^ 2): lane%4 in {0,1} keep t[2k] (groups 4j, 4j+1), {2,3} keep t[2k+1]      -> u[k], k = 4j + component
//   steps 3, 4: row_shr:4 then row_shr:8 — quad 1 = Q0+Q1 and quad 3 = Q2+Q3, then quad 3 = (Q0+Q1)+(Q2+Q3)
// A DPP operand must have been written >= 2 instructions earlier and inline asm is invisible to the hazard recogniser:
// the DPP adds go in blocks of <= 6 behind one s_nop, reading only registers produced before their block (a copy or
// AGPR read-back the register allocator might place in front of a block is covered by the nop as well).  Call with every
// lane of the wave active.
#define GBP_DPP6(ctrl, o, s0, s1)                                                                                         \
  asm volatile("s_nop 1\n\t"                                                                                              \
               "v_add_f32_dpp %0, %6, %12 " ctrl "\n\tv_add_f32_dpp %1, %7, %13 " ctrl "\n\tv_add_f32_dpp %2, %8, %14 " ctrl "\n\t" \
               "v_add_f32_dpp %3, %9, %15 " ctrl "\n\tv_add_f32_dpp %4, %10, %16 " ctrl "\n\tv_add_f32_dpp %5, %11, %17 " ctrl      \
               : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5])                              \
               : "v"(s0[0]), "v"(s0[1]), "v"(s0[2]), "v"(s0[3]), "v"(s0[4]), "v"(s0[5]),                                   \
                 "v"(s1[0]), "v"(s1[1]), "v"(s1[2]), "v"(s1[3]), "v"(s1[4]), "v"(s1[5]))
#define GBP_DPP_QP1 "quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1"
#define GBP_DPP_QP2 "quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1"
#define GBP_DPP_SHR4 "row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1"
#define GBP_DPP_SHR8 "row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1"
template <class Store>
GBP_DEV void row16_sums_store(const float (&oc_eta)[6], const float (&oc_lam)[36], const uint32_t lane, Store&& st) {
  float x[48];      // the record's slots as this lane's terms (6, 7: pads; 44..47: the group that does not exist)
  GBP_UNROLL
  for (int i = 0; i < 6; ++i) x[i] = oc_eta[i];
  GBP_UNROLL
  for (int i = 0; i < 36; ++i) x[8 + i] = oc_lam[i];
  x[6] = x[2]; x[7] = x[3];                      // (any defined value: what the pad / missing slots sum to is never stored)
  GBP_UNROLL
  for (int c = 0; c < 4; ++c) x[44 + c] = x[40 + c];
  const bool odd = (lane & 1u) != 0, hi = (lane & 2u) != 0;
  float t[24], u[12], w[12], r[12];
  {  // step 1: t[m], m = 2k + h, pairs the groups 4j + 2h (kept by even lanes) and 4j + 2h + 1 (kept by odd lanes)
    float keep[24], send[24];
    GBP_UNROLL
    for (int m = 0; m < 24; ++m) {
      const int k = m / 2, h = m % 2, j = k / 4, c = k % 4;
      const float a = x[4 * (4 * j + 2 * h) + c], b = x[4 * (4 * j + 2 * h + 1) + c];
      keep[m] = odd ? b : a;
      send[m] = odd ? a : b;
    }
    GBP_UNROLL
    for (int m = 0; m < 24; m += 6) {
      float o[6], s0[6], s1[6];
      GBP_UNROLL
      for (int i = 0; i < 6; ++i) { s0[i] = send[m + i]; s1[i] = keep[m + i]; }
      GBP_DPP6(GBP_DPP_QP1, o, s0, s1);
      GBP_UNROLL
      for (int i = 0; i < 6; ++i) t[m + i] = o[i];
    }
  }
  {  // step 2
    float keep[12], send[12];
    GBP_UNROLL
    for (int k = 0; k < 12; ++k) {
      keep[k] = hi ? t[2 * k + 1] : t[2 * k];
      send[k] = hi ? t[2 * k] : t[2 * k + 1];
    }
    GBP_UNROLL
    for (int k = 0; k < 12; k += 6) {
      float o[6], s0[6], s1[6];
      GBP_UNROLL
      for (int i = 0; i < 6; ++i) { s0[i] = send[k + i]; s1[i] = keep[k + i]; }
      GBP_DPP6(GBP_DPP_QP2, o, s0, s1);
      GBP_UNROLL
      for (int i = 0; i < 6; ++i) u[k + i] = o[i];
    }
  }
  GBP_UNROLL
  for (int k = 0; k < 12; k += 6) {   // step 3: lanes 4..7 <- 0..3, 12..15 <- 8..11
    float o[6], s0[6];
    GBP_UNROLL
    for (int i = 0; i < 6; ++i) s0[i] = u[k + i];
    GBP_DPP6(GBP_DPP_SHR4, o, s0, s0);
    GBP_UNROLL
    for (int i = 0; i < 6; ++i) w[k + i] = o[i];
  }
  GBP_UNROLL
  for (int k = 0; k < 12; k += 6) {   // step 4: lanes 12..15 <- 4..7
    float o[6], s0[6];
    GBP_UNROLL
    for (int i = 0; i < 6; ++i) s0[i] = w[k + i];
    GBP_DPP6(GBP_DPP_SHR8, o, s0, s0);
    GBP_UNROLL
    for (int i = 0; i < 6; ++i) r[k + i] = o[i];
  }
  if ((lane & 12u) == 12u) {
    const uint32_t q = lane & 3u;
    if (q == 1u) { r[2] = 0.f; r[3] = 0.f; }      // the pad slots of group 1
    GBP_UNROLL
    for (int j = 0; j < 3; ++j)
      if (j < 2 || q < 3u) st(q + 4u * (uint32_t)j, make_float4(r[4 * j], r[4 * j + 1], r[4 * j + 2], r[4 * j + 3]));
  }
}

// A wave's 64 landmark messages between LMSG and the lanes' registers.  In memory they are one contiguous 3 KiB block in record
// order (gbp_kernels.h), moved with kLmsgG coalesced 1 KiB accesses — `ld(k)` / `st(k, v)`: the lane's float4 of access k, float4
// 64 k + lane of the tile — and transposed through a wave-private LDS stage (>= 192 float4) in the plain record order of
// lmsg_lds_slot: the tile-order side touches consecutive float4, the record-order side (lane r: piece q of record r) is free of
// bank conflicts without a swizzle (the maps' comment in gbp_kernels.h).  In registers a message keeps the 16-float shape of a
// landmark record (eta 0..2, Lambda 4..12); the scalar slots 3, 13, 14, 15 are the caller's.
// k_beliefs gathers the messages of a landmark by position (random READS are ~2.3x cheaper than random writes of the same size:
// measured, profiles/HISTORY.md).
template <class Ld>
GBP_DEV void lmsg_tile_in(float4* stage, uint32_t lane, Ld&& ld, float (&lm)[16]) {
  GBP_UNROLL
  for (int k = 0; k < kLmsgG; ++k) {
    const uint32_t i4 = (uint32_t)k * 64u + lane;
    stage[lmsg_lds_slot(lmsg_tile_rec(i4), lmsg_tile_piece(i4))] = ld((uint32_t)k);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float d[4 * kLmsgG];
  GBP_UNROLL
  for (int q = 0; q < kLmsgG; ++q) {
    // (each piece is ONE ds_read_b128: the empty asm keeps the 16 bytes one value.  Without it the compiler re-cuts the 48 bytes
    // along the eta | Lambda boundary of the register image — b96, 2 x b32, b32, b64, b128 — and the narrow reads, whose bank rule
    // is another, conflict at this 48-byte stride: 0.3 M conflict cycles per sweep of the 1M-factor graph)
    v4f v = *reinterpret_cast<const v4f*>(&stage[lmsg_lds_slot(lane, (uint32_t)q)]);
    asm volatile("" : "+v"(v));
    d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w;
  }
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) lm[i] = d[i];
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) lm[4 + i] = d[3 + i];
}
template <class St>
GBP_DEV void lmsg_tile_out(float4* stage, uint32_t lane, const float (&ol)[16], St&& st) {
  float d[4 * kLmsgG];
  GBP_UNROLL
  for (int i = 0; i < 3; ++i) d[i] = ol[i];
  GBP_UNROLL
  for (int i = 0; i < 9; ++i) d[3 + i] = ol[4 + i];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  GBP_UNROLL
  for (int q = 0; q < kLmsgG; ++q) stage[lmsg_lds_slot(lane, (uint32_t)q)] = make_float4(d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  GBP_UNROLL
  for (int k = 0; k < kLmsgG; ++k) {
    const uint32_t i4 = (uint32_t)k * 64u + lane;
    st((uint32_t)k, stage[lmsg_lds_slot(lmsg_tile_rec(i4), lmsg_tile_piece(i4))]);
  }
}

// The landmark sums.  A quad of lanes owns a landmark, lane q its float4 #q of the 16-float record (prior, belief); a message is 12
// dense floats (LMSG in gbp_kernels.h), so lane q < 3 gathers float4 #q of every message (lane 3 repeats lane 2's address: no further
// bytes, no branch) and the sums run on the DENSE image: lmk_quad_dense deals the record's twelve payload slots to the lanes 0..2 as
// the messages hold them, lmk_quad_record deals the sums back (pad slots: zero — a prior's pads are zero, and nothing reads a belief's pad
// slots but the hoisted dmu^2 pieces the owner writes into them afterwards).  Slot for slot the same additions in the same order.
// The loads of a batch are issued UNCONDITIONALLY (unused slots hold position 0: a valid message) before anything looks at a loaded
// value: written as `k < deg ? load : 0` every gather became a branch with its own `s_waitcnt vmcnt(0)` at the join — ten dependent
// round trips per wave instead of ten loads in flight (the ISA showed it; `k_persist` had hit the same thing with its sc1 loads).
GBP_DEV uint32_t lmsg_quad_i4(uint32_t pos, uint32_t q) { return pos * (uint32_t)kLmsgG + (q < 2u ? q : 2u); }
// acc += v, four scalar adds: paired into v_pk_add_f32 the (y, z) halves of messages that arrive in odd-aligned registers are first
// copied into aligned pairs — 8 registers more at the peak of k_beliefs, its seventh wave per SIMD
GBP_DEV void lmk_acc_add(float4& acc, const float4 v) {
  acc.x = acc.x + v.x;
  acc.y = acc.y + v.y; GBP_SLP_FENCE(acc.y);
  acc.z = acc.z + v.z; GBP_SLP_FENCE(acc.z);
  acc.w = acc.w + v.w; GBP_SLP_FENCE(acc.w);
}
GBP_DEV float4 lmsg_load(const float4* lmsg, uint32_t pos, uint32_t q) {
  return lmsg[lmsg_quad_i4(pos, q)];   // default cache policy: a non-temporal hint here costs 4 us (the line's other part is a neighbour's message)
}
// (both are called by whole waves: the DPP moves read the quad's other lanes)
GBP_DEV float4 lmk_quad_dense(const float4 r, uint32_t q) {      // record float4 r of lane q -> dense float4 q (lanes 0..2; lane 3: unused)
  // dense 0 = (r0.x r0.y r0.z r1.x)   dense 1 = (r1.y r1.z r1.w r2.x)   dense 2 = (r2.y r2.z r2.w r3.x)
  // the next lane's .x (lane 3: lane 0's, unused) — a DPP quad permutation [1,2,3,0]: no index register, no trip through the LDS crossbar
  const float nx = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(r.x), 0x39, 0xF, 0xF, false));
  return q == 0u ? make_float4(r.x, r.y, r.z, nx) : make_float4(r.y, r.z, r.w, nx);
}
GBP_DEV float4 lmk_quad_record(const float4 d, uint32_t q) {      // ... and back; all four lanes call it
  // r0 = (d0.x d0.y d0.z 0)   r1 = (d0.w d1.x d1.y d1.z)   r2 = (d1.w d2.x d2.y d2.z)   r3 = (d2.w 0 0 0)
  const float pw = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(d.w), 0x93, 0xF, 0xF, false));      // the previous lane's .w: quad permutation [3,0,1,2] (lane 0: unused)
  if (q == 0u) return make_float4(d.x, d.y, d.z, 0.f);
  if (q == 3u) return make_float4(pw, 0.f, 0.f, 0.f);
  return make_float4(pw, d.x, d.y, d.z);
}

// (host) workgroups of a launch with one thread per item, 256 threads per workgroup: the launchers of the kernel units
static inline uint32_t blocks_for(uint64_t threads) { return (uint32_t)((threads + 255) / 256); }

}  // namespace gbp
