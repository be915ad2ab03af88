// gbp_comm.hpp — the one exchange step of a landmark-sharded GBP iteration, from the C++ host.
//
// Replaces what Poplar compiles for `--ipus N` (reference ba/ba.cpp:414-417,617-649: one graph over N x 1216 tiles,
// inter-IPU exchange generated from the static graph).  Here every rank (one process per GPU) holds a [C x 44] fp32
// buffer of camera partial sums; one ALL-GATHER per iteration gives every rank all of them, and each rank adds
// prior + partials in rank order (k_beliefs) — deterministic, bit-identical camera beliefs on all ranks.
//
// Four transports (Transport, gbp_transport.hpp; a fifth value, Measured, is a way to choose among them: gbp_api_comm.cpp).  Comm::kind() says which one a communicator is; its name, whether it is
// stream-ordered and whether it exchanges through buffers of its own follow from that:
//   * Rccl (xGMI): ncclAllGather on a HIP stream — stream-ordered, capturable into the iteration's hipGraph.  librccl
//     is dlopen'ed on first use (no link-time dependency: a single-GPU user never loads it, and inside a PyTorch
//     process the already-loaded librccl is reused instead of a second copy).
//   * HostStaged: ranks that SHARE a GPU (fewer GPUs than ranks: test rigs, `--ipus 2` on a one-GPU box) cannot form
//     an RCCL communicator ("duplicate GPU"); their partials travel through a MAP_SHARED region (D2H, barrier, H2D).
//     It moves the same bytes in the same layout, only slower; nothing is computed on the host.
//   * P2p (direct peer memory, asked for explicitly): every rank owns an exchange buffer X (ExchangeLayout) in its own device
//     memory, the ranks map each other's through HIP IPC (the same GPU, or peer-accessible GPUs), and a kernel reads every
//     peer's slot in place after ONE host barrier per exchange.  Not stream-ordered.
//   * P2pSlices (asked for explicitly): p2p's buffers and rules, but in the iteration every camera is summed ONCE, by the rank that
//     owns its slice of the cameras, out of the peers' partials; the owner runs the camera chain behind the sum and leaves the
//     finished record in a second IPC-mapped buffer of its own, R (ResultLayout), from where the other ranks gather it — two host
//     barriers per exchange.  Everything outside the iteration (LINEARISE's exchange, NEW_KEYFRAME's and the
//     prior-only refreshes, gbp_comm_probe) is p2p's.
// P2p and P2pSlices are PeerComm: callers ask it for the slot to write and the table to read; only the two layouts know where they lie.
// The shared region also carries the rendezvous of a forked launcher (RCCL unique id, per-rank GPU identity, barrier).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>

#include "gbp_kernels.h"      // kCamRec, kCamRes4: the records the buffers hold
#include "gbp_transport.hpp"

namespace gbp {

constexpr int kCommIdBytes = 128;      // NCCL_UNIQUE_ID_BYTES
// (kCommMaxWorld: gbp_transport.hpp)

// X = [2 parities][world][C][kCamRec] fp32: rank r's partials of an exchange go into slot r of the exchange's parity
struct ExchangeLayout {
  int world = 1; uint32_t n_cams = 0;
  size_t slot_floats() const { return (size_t)n_cams * kCamRec; }
  size_t slot(int p, int r) const { return ((size_t)(p & 1) * (size_t)world + (size_t)r) * slot_floats(); }      // float offset
  size_t bytes() const { return std::max<size_t>(16, 2 * (size_t)world * slot_floats() * sizeof(float)); }      // what a rank allocates (never nothing)
};

// R = [2 parities][widest slice][kCamRes4] float4: one record per camera of the owner's slice (slice_bounds, gbp_kernels.h)
struct ResultLayout {
  int world = 1; uint32_t n_cams = 0;
  size_t res4() const { return ((size_t)n_cams + (size_t)world - 1) / (size_t)world * kCamRes4; }      // float4 of one parity
  size_t parity_offset(int p) const { return (size_t)(p & 1) * res4(); }                                // float4 offset
  size_t bytes() const { return std::max<size_t>(16, 2 * res4() * sizeof(float4)); }
};

class Comm {
 public:
  virtual ~Comm() {}
  virtual Transport kind() const = 0;      // never Auto
  const char* name() const { return transport_name(kind()); }
  // stream-ordered: all_gather only enqueues on its stream (the others synchronise it, exchange and return with recv complete)
  bool stream_ordered() const { return kind() == Transport::Rccl; }
  // recv[r][0..n) = send of rank r, for all r
  virtual int all_gather(const float* send_dev, float* recv_dev, size_t n, hipStream_t s, std::string& err) = 0;
  // small host-side gather (metric sums): all[r*n + i] = mine[i] of rank r
  virtual int all_gather_host(const double* mine, double* all, int n, std::string& err) = 0;
  virtual int barrier(std::string& err) = 0;
  // where the collective library was loaded from and its version ("" / 0 without one): what a first multi-GPU run wants on
  // record next to its numbers
  virtual std::string library_path() const { return ""; }
  virtual int library_version() const { return 0; }
  int rank = 0, world = 1;
};

// The peer-memory transports.  The parity advances once per exchange, whatever made it (all_gather or advance).
class PeerComm : public Comm {
 public:
  // this rank's slot / the whole [world][n] block of the NEXT exchange: what all_gather takes as send / recv
  float* send_slot() const { return X + xl.slot(parity, rank); }
  float* next_block() const { return X + xl.slot(parity, 0); }
  // this rank's own slot of the LAST exchange
  const float* last_own_slot() const { return X + xl.slot(parity ^ 1, rank); }
  // device table of `world` pointers: slot r of parity p in rank r's buffer (its own for r == rank); of the last exchange
  const float* const* peer_table(int p) const { return x_tab + (size_t)(p & 1) * (size_t)world; }
  const float* const* last_table() const { return peer_table(parity ^ 1); }
  // P2pSlices: this rank's result buffer, parity p (written by its reduce only); the device table of every rank's, parity p
  float4* result_buffer(int p) const { return R + rl.parity_offset(p); }
  const float4* const* result_table(int p) const { return r_tab + (size_t)(p & 1) * (size_t)world; }
  // the exchange without a copy: synchronise `s`, one region barrier, advance the parity; *closed = the parity of this exchange.
  // Until this rank's next exchange a kernel on `s` may read peer_table(*closed) in place.
  int advance(hipStream_t s, int* closed, std::string& err);
  // both parities of X cleared (a new problem)
  hipError_t zero(hipStream_t s) const { return hipMemsetAsync(X, 0, xl.bytes(), s); }

 protected:
  ExchangeLayout xl;
  ResultLayout rl;
  float* X = nullptr;
  const float* const* x_tab = nullptr;      // [2][world]
  float4* R = nullptr;
  const float4* const* r_tab = nullptr;     // [2][world]
  int parity = 0;                           // of the NEXT exchange
};

// c as PeerComm if it exchanges through buffers of its own, not through the ctx's / the caller's; nullptr otherwise (and for no communicator)
inline PeerComm* peers(Comm* c) {
  return c && (c->kind() == Transport::P2p || c->kind() == Transport::P2pSlices) ? static_cast<PeerComm*>(c) : nullptr;
}

// RCCL
int comm_unique_id(void* id128, std::string& err);
Comm* comm_create_rccl(const void* id128, int rank, int world, std::string& err);

// shared rendezvous / staging region (created by the launcher before the ranks start, e.g. mmap MAP_SHARED|MAP_ANONYMOUS)
size_t comm_region_bytes(uint32_t n_cams, int world);
int comm_region_init(void* region, size_t bytes, uint32_t n_cams, int world);
void comm_region_abort(void* region);      // a supervisor saw a rank die: wake every rank waiting in the region with an error
int comm_region_selftest(void* region, int rank, int world, int rounds, std::string& err);   // protocol check, no device
// n_cams: the ctx's cameras, the size of a rank's slot in X
Comm* comm_create_from_region(void* region, int rank, int world, Transport transport, uint32_t n_cams, std::string& err);

// The measured transport (Transport::Measured, gbp_api_comm.cpp: comm_init_measured) takes the two steps of comm_create_from_region apart.
// 1. Collective: every rank publishes its facts in the region — its GPU; then, knowing every rank's GPU, peer access towards each and
//    (only where no two ranks share a GPU: RCCL is out otherwise, and the library is not loaded to learn nothing) whether librccl
//    resolves — and leaves with the same table[world] as every other rank.  No communicator exists yet, nothing can have failed in one.
int comm_region_facts(void* region, int rank, int world, RankFacts* table, std::string& err);
// 2. Collective: a communicator of ONE given transport (Rccl, HostStaged, P2p, P2pSlices) that eligible_candidates(table) allows.
//    Rccl at most once per region (its unique id is handed over once): the measured transport keeps that communicator between its
//    two measurements.  A failure raises the region's abort flag, as in comm_create_from_region.
Comm* comm_create_in_region(void* region, int rank, int world, Transport transport, uint32_t n_cams, std::string& err);

}  // namespace gbp
