// gbp_comm.hpp — the one exchange step of a landmark-sharded GBP iteration, from the C++ host.
//
// Replaces what Poplar compiles for `--ipus N` (reference ba/ba.cpp:414-417,617-649: one graph over N x 1216 tiles,
// inter-IPU exchange generated from the static graph).  Here every rank (one process per GPU) holds a [C x 44] fp32
// buffer of camera partial sums; one ALL-GATHER per iteration gives every rank all of them, and each rank adds
// prior + partials in rank order (k_beliefs) — deterministic, bit-identical camera beliefs on all ranks.
//
// Four transports behind one interface:
//   * RCCL (xGMI): ncclAllGather on a HIP stream — stream-ordered, capturable into the iteration's hipGraph.  librccl
//     is dlopen'ed on first use (no link-time dependency: a single-GPU user never loads it, and inside a PyTorch
//     process the already-loaded librccl is reused instead of a second copy).
//   * host-staged: ranks that SHARE a GPU (fewer GPUs than ranks: test rigs, `--ipus 2` on a one-GPU box) cannot form
//     an RCCL communicator ("duplicate GPU"); their partials travel through a MAP_SHARED region (D2H, barrier, H2D).
//     It moves the same bytes in the same layout, only slower; nothing is computed on the host.
//   * p2p (direct peer memory, asked for explicitly): every rank owns an exchange buffer [2 parities][world][C][44] in its
//     own device memory, the ranks map each other's through HIP IPC (the same GPU, or peer-accessible GPUs), and a kernel
//     reads every peer's slot in place after ONE host barrier per exchange.  Not stream-ordered.
//   * p2p-slices (asked for explicitly): p2p's buffers and rules, but in the iteration every camera is summed ONCE, by the rank that owns
//     its slice of the cameras, out of the peers' partials; the owner runs the camera chain behind the sum and leaves the finished record
//     in a second IPC-mapped buffer of its own, from where the other ranks gather it — two host barriers per exchange.
//     Everything outside the iteration (LINEARISE's exchange, NEW_KEYFRAME's and the prior-only refreshes, gbp_comm_probe) is p2p's.
// The shared region also carries the rendezvous of a forked launcher (RCCL unique id, per-rank GPU identity, barrier).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

namespace gbp {

constexpr int kCommIdBytes = 128;      // NCCL_UNIQUE_ID_BYTES
constexpr int kCommMaxWorld = 64;

class Comm {
 public:
  virtual ~Comm() {}
  // recv[r][0..n) = send of rank r, for all r.  Stream-ordered transports enqueue on `s`; the host-staged one
  // synchronises `s`, exchanges and returns with recv complete.
  virtual int all_gather(const float* send_dev, float* recv_dev, size_t n, hipStream_t s, std::string& err) = 0;
  virtual bool stream_ordered() const = 0;
  // small host-side gather (metric sums): all[r*n + i] = mine[i] of rank r
  virtual int all_gather_host(const double* mine, double* all, int n, std::string& err) = 0;
  virtual int barrier(std::string& err) = 0;
  virtual const char* name() const = 0;
  // where the collective library was loaded from and its version ("" / 0 for the host-staged transport): what a first
  // multi-GPU run wants on record next to its numbers
  virtual std::string library_path() const { return ""; }
  virtual int library_version() const { return 0; }
  // ---- the direct peer-memory transport only (nullptr / an error for the others) ----
  // its exchange buffer [2 parities][world][n] fp32 (parity 1 at + world * n); rank r's partials go into slot r
  virtual float* exchange_buffer() const { return nullptr; }
  // device table of `world` pointers: slot r of parity p in rank r's buffer (its own for r == rank)
  virtual const float* const* peer_table(int p) const { (void)p; return nullptr; }
  // parity of the NEXT exchange: advances once per exchange, whatever made it
  virtual int next_parity() const { return 0; }
  // the exchange without a copy: synchronise `s`, one region barrier, advance the parity.  Until this rank's next exchange a
  // kernel on `s` may read peer_table(parity of this exchange) in place.
  virtual int exchange_in_place(hipStream_t s, std::string& err) { (void)s; err = "not a peer-memory transport"; return -1; }
  // ---- the sliced peer-memory transport only ----
  // true: the iteration reduces every camera once, on the rank that owns its slice (slice_bounds, gbp_kernels.h), and gathers the results
  virtual bool sliced() const { return false; }
  // this rank's result buffer, parity p: one record of kCamRes4 float4 per camera of its slice (written by its reduce only)
  virtual float4* result_buffer(int p) const { (void)p; return nullptr; }
  // device table of `world` pointers: the result buffer of rank r, parity p (its own for r == rank)
  virtual const float4* const* result_table(int p) const { (void)p; return nullptr; }
  int rank = 0, world = 1;
};

// RCCL
int comm_unique_id(void* id128, std::string& err);
Comm* comm_create_rccl(const void* id128, int rank, int world, std::string& err);

// shared rendezvous / staging region (created by the launcher before the ranks start, e.g. mmap MAP_SHARED|MAP_ANONYMOUS)
size_t comm_region_bytes(uint32_t n_cams, int world);
int comm_region_init(void* region, size_t bytes, uint32_t n_cams, int world);
void comm_region_abort(void* region);
int comm_region_selftest(void* region, int rank, int world, int rounds, std::string& err);   // protocol check, no device   // a supervisor saw a rank die: wake every rank waiting in the region with an error
// transport: 0 = auto (RCCL when every rank sits on its own GPU, host-staged otherwise), 1 = RCCL, 2 = host-staged,
// 3 = p2p, 4 = p2p-slices (neither ever chosen by auto; n_cams: the ctx's cameras, the size of a rank's slot in the p2p exchange buffer)
Comm* comm_create_from_region(void* region, int rank, int world, int transport, uint32_t n_cams, std::string& err);

}  // namespace gbp
