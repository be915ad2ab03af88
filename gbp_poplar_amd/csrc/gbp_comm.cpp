// gbp_comm.cpp — transports of the per-iteration camera-partial all-gather (see gbp_comm.hpp).
#include "gbp_comm.hpp"
#include "gbp_kernels.h"

#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: the library is dlopen'ed, nothing links against it
#include <sched.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

namespace gbp {
namespace {

// ---- RCCL through dlopen ------------------------------------------------------------------------------------
struct RcclApi {
  void* handle = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclGetVersion) GetVersion = nullptr;     // optional
  std::string path;                                    // resolved file the symbols come from (dladdr)
  std::string error;
};

RcclApi& rccl() {
  static RcclApi api;
  static bool tried = false;
  if (tried) return api;
  tried = true;
  // Inside a PyTorch process torch's own librccl (loaded as "librccl.so") is already there: reuse it, two RCCL
  // runtimes in one process would each bring their own bootstrap and HIP state.
  // GBP_RCCL_LIB names the library explicitly: then ONLY that path is tried (no silent substitute).
  const char* env = std::getenv("GBP_RCCL_LIB");
  void* h = nullptr;
  std::string tried_names;
  auto open = [&](const char* name, int flags) {
    if (h) return;
    (void)dlerror();
    h = dlopen(name, flags);
    if (!h && !(flags & RTLD_NOLOAD)) {
      const char* de = dlerror();     // read ONCE: the call clears the message
      tried_names += std::string(tried_names.empty() ? "" : "; ") + name + ": " + (de ? de : "?");
    }
  };
  if (env && *env) {
    open(env, RTLD_NOW | RTLD_LOCAL);
  } else {
    open("librccl.so", RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
    open("librccl.so.1", RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
    for (const char* name : {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"}) open(name, RTLD_NOW | RTLD_LOCAL);
  }
  if (!h) {
    api.error = "librccl not found (dlopen: " + tried_names + ")";
    return api;
  }
  api.handle = h;
  api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
  api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
  api.AllGather = reinterpret_cast<decltype(api.AllGather)>(dlsym(h, "ncclAllGather"));
  api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
  api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
  api.GetVersion = reinterpret_cast<decltype(api.GetVersion)>(dlsym(h, "ncclGetVersion"));
  Dl_info info;
  if (api.AllGather && dladdr(reinterpret_cast<void*>(api.AllGather), &info) && info.dli_fname) api.path = info.dli_fname;
  if (!api.GetUniqueId || !api.CommInitRank || !api.AllGather || !api.CommDestroy || !api.GetErrorString) {
    api.error = "librccl lacks an expected symbol";
    api.handle = nullptr;
  }
  return api;
}

std::string nccl_err(const char* what, ncclResult_t r) {
  return std::string(what) + ": " + (rccl().GetErrorString ? rccl().GetErrorString(r) : "RCCL error");
}

// ---- shared region ----------------------------------------------------------------------------------------------
constexpr uint32_t kMagic = 0x47425043u;   // "GBPC"
constexpr double kTimeoutS = 300.0;

struct RegionHeader {
  uint32_t magic, world, n_cams, pad;
  std::atomic<uint32_t> bar_count, bar_sense, abort_flag, id_ready;
  char id[kCommIdBytes];
  RankFacts facts[kCommMaxWorld];                    // every rank's GPU (all transports); peer access and librccl (the measured transport)
  double scratch[kCommMaxWorld][16];
  char ipc[kCommMaxWorld][HIP_IPC_HANDLE_SIZE];     // p2p: every rank's IPC handle of its exchange buffer (fixed size: the region's
                                                     // size stays linear in world x cams)
};
static_assert(std::atomic<uint32_t>::is_always_lock_free, "cross-process barrier needs lock-free atomics");
static_assert(sizeof(RegionHeader) == 32 + kCommIdBytes + kCommMaxWorld * (64 + 16 * sizeof(double) + HIP_IPC_HANDLE_SIZE),
              "the header's size is part of gbp_comm_region_bytes");

inline size_t header_bytes() { return (sizeof(RegionHeader) + 255) / 256 * 256; }
inline float* region_data(void* region) { return reinterpret_cast<float*>(static_cast<char*>(region) + header_bytes()); }

struct RegionPeer {   // one rank's view of the region: sense-reversing barrier, abortable and bounded in time
  RegionHeader* h = nullptr;
  uint32_t sense = 0;
  int world = 1;
  bool wait_until(const std::atomic<uint32_t>& a, uint32_t want, std::string& err, const char* what) {
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while (a.load(std::memory_order_acquire) != want) {
      if (h->abort_flag.load(std::memory_order_acquire)) { err = std::string(what) + ": another rank aborted"; return false; }
      if (++spins > 2000) {
        usleep(50);
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > kTimeoutS) {
          h->abort_flag.store(1, std::memory_order_release);
          err = std::string(what) + ": timed out waiting for the other ranks";
          return false;
        }
      } else {
        sched_yield();
      }
    }
    return true;
  }
  // The sense of a barrier is the opposite of the last one's, which the region still shows when a rank arrives: it changes only once
  // every rank has arrived at the NEXT barrier, this one included.  So any copy of a RegionPeer may take the next barrier, whichever
  // copy took the last (the measured transport makes and drops communicators on one region).
  bool barrier(std::string& err) {
    sense = h->bar_sense.load(std::memory_order_acquire) ^ 1u;
    if (h->bar_count.fetch_add(1, std::memory_order_acq_rel) + 1 == (uint32_t)world) {
      h->bar_count.store(0, std::memory_order_relaxed);
      h->bar_sense.store(sense, std::memory_order_release);
      return true;
    }
    return wait_until(h->bar_sense, sense, err, "barrier");
  }
  bool gather_host(int rank, const double* mine, double* all, int n, std::string& err) {
    if (n > 16) { err = "all_gather_host: at most 16 values"; return false; }
    std::memcpy(h->scratch[rank], mine, sizeof(double) * n);
    if (!barrier(err)) return false;
    for (int r = 0; r < world; ++r) std::memcpy(all + (size_t)r * n, h->scratch[r], sizeof(double) * n);
    return barrier(err);    // nobody overwrites the scratch before everyone has read it
  }
};

// ---- RCCL transport ---------------------------------------------------------------------------------------------
class RcclComm : public Comm {
 public:
  ncclComm_t comm = nullptr;
  RegionPeer peer;                 // launcher-made groups: host-side gather / barrier through the region
  double* d_scratch = nullptr;     // id-made groups (no region): small gathers through RCCL itself
  ~RcclComm() override {
    if (d_scratch) (void)hipFree(d_scratch);
    if (comm && rccl().CommDestroy) (void)rccl().CommDestroy(comm);
  }
  int all_gather(const float* send, float* recv, size_t n, hipStream_t s, std::string& err) override {
    const ncclResult_t r = rccl().AllGather(send, recv, n, ncclFloat, comm, s);
    if (r != ncclSuccess) { err = nccl_err("ncclAllGather", r); return -1; }
    return 0;
  }
  int all_gather_host(const double* mine, double* all, int n, std::string& err) override {
    if (peer.h) return peer.gather_host(rank, mine, all, n, err) ? 0 : -1;
    if (n > 16) { err = "all_gather_host: at most 16 values"; return -1; }
    if (!d_scratch && hipMalloc(&d_scratch, sizeof(double) * 16 * (size_t)(world + 1)) != hipSuccess) { err = "hipMalloc"; return -1; }
    if (hipMemcpy(d_scratch, mine, sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess) { err = "hipMemcpy"; return -1; }
    const ncclResult_t r = rccl().AllGather(d_scratch, d_scratch + 16, (size_t)n, ncclDouble, comm, nullptr);
    if (r != ncclSuccess) { err = nccl_err("ncclAllGather", r); return -1; }
    if (hipStreamSynchronize(nullptr) != hipSuccess ||
        hipMemcpy(all, d_scratch + 16, sizeof(double) * n * (size_t)world, hipMemcpyDeviceToHost) != hipSuccess) { err = "hip sync/copy"; return -1; }
    return 0;
  }
  int barrier(std::string& err) override {
    if (peer.h) return peer.barrier(err) ? 0 : -1;
    double x = 0, all[kCommMaxWorld];
    return all_gather_host(&x, all, 1, err);
  }
  Transport kind() const override { return Transport::Rccl; }
  std::string library_path() const override { return rccl().path; }
  int library_version() const override {
    int v = 0;
    if (rccl().GetVersion && rccl().GetVersion(&v) == ncclSuccess) return v;
    return 0;
  }
};

// ---- host-staged transport (ranks sharing a GPU) -----------------------------------------------------------------------
class StagedComm : public Comm {
 public:
  RegionPeer peer;
  float* data = nullptr;        // the region's staging slots, laid out as X
  ExchangeLayout l;
  int parity = 0;
  std::vector<float> stage;
  int all_gather(const float* send, float* recv, size_t n, hipStream_t s, std::string& err) override {
    if (n > l.slot_floats()) { err = "all_gather: message larger than the staging region"; return -1; }
    float* slot = data + l.slot(parity, rank);
    if (hipMemcpyAsync(slot, send, n * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
      err = "all_gather: device -> region copy failed";
      return -1;
    }
    if (!peer.barrier(err)) return -1;
    // a rank can be at most one exchange ahead of the slowest one (the next barrier needs everybody), so the
    // two parities never collide
    stage.resize((size_t)world * n);
    for (int r = 0; r < world; ++r) std::memcpy(&stage[(size_t)r * n], data + l.slot(parity, r), n * 4);
    if (hipMemcpyAsync(recv, stage.data(), stage.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
      err = "all_gather: region -> device copy failed";
      return -1;
    }
    parity ^= 1;
    return 0;
  }
  int all_gather_host(const double* mine, double* all, int n, std::string& err) override {
    return peer.gather_host(rank, mine, all, n, err) ? 0 : -1;
  }
  int barrier(std::string& err) override { return peer.barrier(err) ? 0 : -1; }
  Transport kind() const override { return Transport::HostStaged; }
  bool setup(RegionHeader* h, int, uint32_t, std::string& err) {      // (the staging slots are the region's, sized by its cameras)
    data = region_data(h);
    l = ExchangeLayout{world, h->n_cams};
    return peer.barrier(err);
  }
};

// ---- one IPC-shared device buffer --------------------------------------------------------------------------------------------
// A rank's hipMalloc'ed buffer that every peer maps through HIP IPC, and the device table of pointers into the ranks' buffers.
// who / what name the transport and the buffer in the error texts ("p2p" / "exchange buffer").
struct IpcBuffer {
  void* own = nullptr;
  std::vector<void*> mapped;       // [world] IPC mappings of the peers' buffers (nullptr: this rank)
  void** d_tab = nullptr;          // [2][world] device pointer table
  IpcBuffer() = default;
  IpcBuffer(const IpcBuffer&) = delete;
  IpcBuffer& operator=(const IpcBuffer&) = delete;
  // (the owner has quiesced: no peer reads this rank's buffer any more) the mappings closed first, this rank's memory freed last
  ~IpcBuffer() {
    for (void* p : mapped)
      if (p) (void)hipIpcCloseMemHandle(p);
    if (d_tab) (void)hipFree(d_tab);
    if (own) (void)hipFree(own);
  }
  // Collective over the ranks, four region barriers; on failure the caller raises the region's abort flag.  The handle goes into the
  // region's handle slot of this rank (idle: a barrier lies behind every rank's reads of what it held before).  off(p, r): byte
  // offset in rank r's buffer of what entry r of parity p's table points to.
  template <class Off>
  bool setup(RegionHeader* h, RegionPeer& peer, int rank, const char* who, const char* what, uint32_t tag, uint32_t n_cams, size_t bytes,
             Off off, std::string& err) {
    const int world = peer.world;
    const std::string pre = std::string(who) + ": ";
    // 1. the buffer, its handle published in the region
    if (hipMalloc(&own, bytes) != hipSuccess) { own = nullptr; err = pre + "hipMalloc of the " + what + " failed"; return false; }
    hipIpcMemHandle_t handle;
    if (hipIpcGetMemHandle(&handle, own) != hipSuccess) { err = pre + "hipIpcGetMemHandle failed"; return false; }
    std::memcpy(h->ipc[rank], &handle, HIP_IPC_HANDLE_SIZE);
    if (!peer.barrier(err)) return false;
    // 2. every peer's buffer mapped (never this rank's own handle)
    mapped.assign(world, nullptr);
    for (int r = 0; r < world; ++r) {
      if (r == rank) continue;
      std::memcpy(&handle, h->ipc[r], HIP_IPC_HANDLE_SIZE);
      if (hipIpcOpenMemHandle(&mapped[r], handle, hipIpcMemLazyEnablePeerAccess) != hipSuccess || !mapped[r]) {
        mapped[r] = nullptr;
        err = pre + "hipIpcOpenMemHandle of rank " + std::to_string(r) + "'s " + what + " failed";
        return false;
      }
    }
    auto at = [&](int p, int r) { return static_cast<char*>(r == rank ? own : mapped[r]) + off(p, r); };
    // 3. every mapping checked with runtime copies before any kernel reads through it: (tag, rank, C, world) where entry (0, r) points
    const uint32_t pat[4] = {tag, (uint32_t)rank, n_cams, (uint32_t)world};
    if (hipMemcpy(at(0, rank), pat, sizeof(pat), hipMemcpyHostToDevice) != hipSuccess) { err = pre + "pattern copy failed"; return false; }
    if (!peer.barrier(err)) return false;
    for (int r = 0; r < world; ++r) {
      if (r == rank) continue;
      uint32_t got[4] = {0, 0, 0, 0};
      const uint32_t want[4] = {tag, (uint32_t)r, n_cams, (uint32_t)world};
      if (hipMemcpy(got, at(0, r), sizeof(got), hipMemcpyDeviceToHost) != hipSuccess || std::memcmp(got, want, sizeof(got)) != 0) {
        err = pre + "the mapping of rank " + std::to_string(r) + "'s " + what + " does not hold its pattern";
        return false;
      }
    }
    if (!peer.barrier(err)) return false;
    if (hipMemset(own, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { err = pre + "zero-fill failed"; return false; }
    // 4. the pointer tables
    std::vector<void*> tab(2 * (size_t)world);
    for (int p = 0; p < 2; ++p)
      for (int r = 0; r < world; ++r) tab[(size_t)p * world + r] = at(p, r);
    if (hipMalloc(&d_tab, tab.size() * sizeof(void*)) != hipSuccess) { d_tab = nullptr; err = pre + "hipMalloc failed"; return false; }
    if (hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(void*), hipMemcpyHostToDevice) != hipSuccess) { err = pre + "table upload failed"; return false; }
    return peer.barrier(err);
  }
};

// ---- direct peer-memory transport (p2p) ---------------------------------------------------------------------------------
// Every rank owns X (ExchangeLayout; its own hipMalloc).  Rank r's partials always go into slot r of the parity of the
// exchange; peers read only that slot, through an IPC mapping of X; a rank's gather writes only the other slots of its own X.
// Exchange k: partials into parity k & 1 (stream-ordered), stream synchronised, ONE region barrier, then the readers
// (k_gather_peers / k_beliefs_cam_peers) on the stream.  A rank reaches barrier k + 1 only after its stream has finished everything
// it enqueued before it — its reads of exchange k included — so by the time any rank writes parity k & 1 again (exchange k + 2, after
// barrier k + 1) every peer is done reading it.
class P2pComm : public PeerComm {
 public:
  RegionPeer peer;
  IpcBuffer x;
  bool armed = false;              // every rank has set up: teardown meets the others at a barrier
  bool quiet = false;              // quiesce() has run
  // first step of every teardown, once: this rank's work done, then (armed) every rank's — no peer reads this rank's buffers any more
  void quiesce() {
    if (quiet) return;
    quiet = true;
    (void)hipDeviceSynchronize();
    std::string err;
    if (armed) (void)peer.barrier(err);
  }
  ~P2pComm() override { quiesce(); }      // (then the members: mappings closed, memory freed)
  Transport kind() const override { return Transport::P2p; }
  int all_gather(const float* send, float* recv, size_t n, hipStream_t s, std::string& err) override {
    if (n != xl.slot_floats() || send != send_slot() || recv != next_block()) {
      err = "all_gather: the p2p transport exchanges through its own buffer (send / recv of the current parity)";
      return -1;
    }
    int p = 0;
    if (advance(s, &p, err) != 0) return -1;
    launch_gather_peers(peer_table(p), recv, (uint32_t)(n / 4), world, rank, s);
    if (hipGetLastError() != hipSuccess) { err = "all_gather: k_gather_peers did not launch"; return -1; }
    return 0;
  }
  int all_gather_host(const double* mine, double* all, int n, std::string& err) override {
    return peer.gather_host(rank, mine, all, n, err) ? 0 : -1;
  }
  int barrier(std::string& err) override { return peer.barrier(err) ? 0 : -1; }

  virtual bool setup(RegionHeader* h, int dev, uint32_t n_cams, std::string& err) {
    // ranks on different GPUs must reach each other's memory
    for (int r = 0; r < world; ++r) {
      if (r == rank || same_gpu(h->facts[r], h->facts[rank])) continue;
      int pdev = -1, can = 0;
      if (hipDeviceGetByPCIBusId(&pdev, h->facts[r].bus) != hipSuccess || hipDeviceCanAccessPeer(&can, dev, pdev) != hipSuccess || !can) {
        err = std::string("p2p: the GPU of rank ") + std::to_string(rank) + " (" + h->facts[rank].bus + ") cannot access the GPU of rank " +
              std::to_string(r) + " (" + h->facts[r].bus + ")";
        return false;
      }
    }
    xl = ExchangeLayout{world, n_cams};
    armed = x.setup(h, peer, rank, "p2p", "exchange buffer", kMagic, n_cams, xl.bytes(), [this](int p, int r) { return xl.slot(p, r) * sizeof(float); }, err);
    X = static_cast<float*>(x.own);
    x_tab = reinterpret_cast<const float* const*>(x.d_tab);
    return armed;
  }
};

// ---- sliced peer-memory transport (p2p-slices) ---------------------------------------------------------------------------------------
// P2pComm (its exchange buffer X, its tables, its all_gather for everything outside the iteration) plus a second IPC-mapped buffer per
// rank, the RESULT buffer R (ResultLayout), written only by its owner.  The cameras are cut into `world` slices (slice_bounds,
// gbp_kernels.h), rank s owns slice s.  Exchange k of the iteration, parity p = k & 1:
//   partials into X[p][rank]; stream sync; barrier A (advance)
//   reduce: the owner sums its slice out of every peer's X[p] and writes the finished records into its own R[p]; stream sync; barrier B
//   gather: every rank copies the other slices out of their owners' R[p]
// A rank reaches the next barrier, whichever it is, only after its stream has finished everything enqueued before it.  So X[p] is written
// again (exchange k + 2, behind a barrier of exchange k + 1) only after every rank's reduce k has ended, and R[p] is written again (reduce
// k + 2, behind barrier A of k + 2) only after every rank's gather k has ended.
class P2pSlicesComm : public P2pComm {
 public:
  IpcBuffer r;                     // (destroyed before P2pComm's x: R's mappings and memory go first)
  ~P2pSlicesComm() override { quiesce(); }      // no peer reads R (or X) any more
  Transport kind() const override { return Transport::P2pSlices; }
  // X as in p2p; then the same steps for R — its handle goes into the region's handle slots only behind the barrier that ended X's
  // setup, when every rank has opened the handles of X
  bool setup(RegionHeader* h, int dev, uint32_t n_cams, std::string& err) override {
    if (!P2pComm::setup(h, dev, n_cams, err)) return false;
    armed = false;                 // (a failure below is met by the region's abort flag, not by a teardown barrier)
    rl = ResultLayout{world, n_cams};
    armed = r.setup(h, peer, rank, "p2p-slices", "result buffer", ~kMagic, n_cams, rl.bytes(), [this](int p, int) { return rl.parity_offset(p) * sizeof(float4); }, err);
    R = static_cast<float4*>(r.own);
    r_tab = reinterpret_cast<const float4* const*>(r.d_tab);
    return armed;
  }
};

// a communicator of a launcher-made group: constructed, given its place in the group, set up — or the region's abort flag raised
template <class T>
Comm* create_in_region(RegionHeader* h, const RegionPeer& peer, int rank, int world, int dev, uint32_t n_cams, std::string& err) {
  T* c = new (std::nothrow) T();
  if (c) { c->rank = rank; c->world = world; c->peer = peer; }
  else err = "out of memory";
  if (c && c->setup(h, dev, n_cams, err)) return c;
  h->abort_flag.store(1);
  delete c;
  return nullptr;
}

}  // namespace

int PeerComm::advance(hipStream_t s, int* closed, std::string& err) {
  if (hipStreamSynchronize(s) != hipSuccess) { err = "p2p exchange: stream synchronisation failed"; return -1; }
  if (barrier(err) != 0) return -1;
  *closed = parity;
  parity ^= 1;
  return 0;
}

int comm_unique_id(void* id128, std::string& err) {
  RcclApi& api = rccl();
  if (!api.handle) { err = api.error; return -1; }
  ncclUniqueId id;
  const ncclResult_t r = api.GetUniqueId(&id);
  if (r != ncclSuccess) { err = nccl_err("ncclGetUniqueId", r); return -1; }
  std::memcpy(id128, id.internal, kCommIdBytes);
  return 0;
}

Comm* comm_create_rccl(const void* id128, int rank, int world, std::string& err) {
  RcclApi& api = rccl();
  if (!api.handle) { err = api.error; return nullptr; }
  if (world < 1 || world > kCommMaxWorld || rank < 0 || rank >= world) { err = "bad rank / world"; return nullptr; }
  ncclUniqueId id;
  std::memcpy(id.internal, id128, kCommIdBytes);
  RcclComm* c = new (std::nothrow) RcclComm();
  if (!c) { err = "out of memory"; return nullptr; }
  c->rank = rank; c->world = world;
  const ncclResult_t r = api.CommInitRank(&c->comm, world, id, rank);
  if (r != ncclSuccess) {
    err = nccl_err("ncclCommInitRank", r);
    c->comm = nullptr;
    delete c;
    return nullptr;
  }
  return c;
}

size_t comm_region_bytes(uint32_t n_cams, int world) {
  if (world < 1) world = 1;
  return header_bytes() + (size_t)2 * world * n_cams * 44 * sizeof(float);
}

int comm_region_init(void* region, size_t bytes, uint32_t n_cams, int world) {
  if (!region || world < 1 || world > kCommMaxWorld || bytes < comm_region_bytes(n_cams, world)) return -1;
  RegionHeader* h = new (region) RegionHeader();
  h->magic = kMagic; h->world = (uint32_t)world; h->n_cams = n_cams; h->pad = 0;
  h->bar_count.store(0); h->bar_sense.store(0); h->abort_flag.store(0); h->id_ready.store(0);
  std::memset(h->id, 0, sizeof(h->id));
  std::memset(h->facts, 0, sizeof(h->facts));
  std::memset(h->ipc, 0, sizeof(h->ipc));
  return 0;
}

void comm_region_abort(void* region) {
  RegionHeader* h = static_cast<RegionHeader*>(region);
  if (h && h->magic == kMagic) h->abort_flag.store(1, std::memory_order_release);
}

// The cross-process protocol of the region on its own (no device): `rounds` x {gather of two doubles per rank, barrier},
// every rank checks what it received.  Lets the rendezvous / staging logic be tested on a CPU-only box.
int comm_region_selftest(void* region, int rank, int world, int rounds, std::string& err) {
  RegionHeader* h = static_cast<RegionHeader*>(region);
  if (!h || h->magic != kMagic || (int)h->world != world || rank < 0 || rank >= world) { err = "bad communication region"; return -1; }
  RegionPeer peer;
  peer.h = h; peer.world = world;
  std::vector<double> all((size_t)world * 2);
  for (int r = 0; r < rounds; ++r) {
    const double mine[2] = {(double)(rank * 1000 + r), (double)(r - rank)};
    if (!peer.gather_host(rank, mine, all.data(), 2, err)) return -1;
    for (int k = 0; k < world; ++k)
      if (all[(size_t)k * 2] != (double)(k * 1000 + r) || all[(size_t)k * 2 + 1] != (double)(r - k)) { err = "selftest: wrong data from a rank"; return -2; }
    if (!peer.barrier(err)) return -1;
  }
  return 0;
}

namespace {

RegionHeader* checked_region(void* region, int rank, int world, std::string& err) {
  RegionHeader* h = static_cast<RegionHeader*>(region);
  if (!h || h->magic != kMagic || (int)h->world != world || rank < 0 || rank >= world) { err = "bad communication region"; return nullptr; }
  return h;
}

// this rank's GPU into its slot of the region's table (the rest of the slot cleared)
bool publish_gpu(RegionHeader* h, int rank, int* dev, std::string& err) {
  RankFacts mine;
  std::memset(&mine, 0, sizeof(mine));
  if (hipGetDevice(dev) != hipSuccess || hipDeviceGetPCIBusId(mine.bus, sizeof(mine.bus), *dev) != hipSuccess) { err = "hipDeviceGetPCIBusId failed"; return false; }
  mine.bus[sizeof(mine.bus) - 1] = 0;
  std::memcpy(&h->facts[rank], &mine, sizeof(mine));
  return true;
}

// every rank knows every rank's GPU: the communicator of one transport (any number but Rccl, P2p, P2pSlices: host-staged)
Comm* create_transport(RegionHeader* h, const RegionPeer& peer, int rank, int world, int dev, Transport transport, uint32_t n_cams,
                       std::string& err) {
  switch (transport) {
    case Transport::P2p: return create_in_region<P2pComm>(h, peer, rank, world, dev, n_cams, err);
    case Transport::P2pSlices: return create_in_region<P2pSlicesComm>(h, peer, rank, world, dev, n_cams, err);
    case Transport::Rccl: break;
    default: return create_in_region<StagedComm>(h, peer, rank, world, dev, n_cams, err);      // (any other number: as before, host-staged)
  }
  if (any_shared_gpu(h->facts, world)) { err = "RCCL needs one GPU per rank, but two ranks share a GPU"; h->abort_flag.store(1); return nullptr; }
  // RCCL: rank 0 draws the unique id, the region hands it to the others
  if (rank == 0) {
    if (comm_unique_id(h->id, err) != 0) { h->abort_flag.store(1); return nullptr; }
    h->id_ready.store(1, std::memory_order_release);
  } else if (!RegionPeer(peer).wait_until(h->id_ready, 1u, err, "RCCL unique id")) {
    return nullptr;
  }
  Comm* c = comm_create_rccl(h->id, rank, world, err);
  if (!c) { h->abort_flag.store(1); return nullptr; }
  static_cast<RcclComm*>(c)->peer = peer;
  if (!static_cast<RcclComm*>(c)->peer.barrier(err)) { delete c; return nullptr; }
  return c;
}

}  // namespace

Comm* comm_create_from_region(void* region, int rank, int world, Transport transport, uint32_t n_cams, std::string& err) {
  RegionHeader* h = checked_region(region, rank, world, err);
  if (!h) return nullptr;
  RegionPeer peer;
  peer.h = h; peer.world = world;
  // every rank publishes the identity of its GPU; a GPU shared by two ranks rules RCCL out
  int dev = 0;
  if (!publish_gpu(h, rank, &dev, err)) return nullptr;
  if (!peer.barrier(err)) return nullptr;
  if (transport == Transport::Auto) transport = any_shared_gpu(h->facts, world) ? Transport::HostStaged : Transport::Rccl;
  return create_transport(h, peer, rank, world, dev, transport, n_cams, err);
}

int comm_region_facts(void* region, int rank, int world, RankFacts* table, std::string& err) {
  RegionHeader* h = checked_region(region, rank, world, err);
  if (!h) return -1;
  RegionPeer peer;
  peer.h = h; peer.world = world;
  int dev = 0;
  if (!publish_gpu(h, rank, &dev, err)) { h->abort_flag.store(1); return -1; }
  if (!peer.barrier(err)) return -1;
  // every rank's GPU is known: what this rank can reach, and (own GPUs only) whether it has the collective library
  RankFacts& mine = h->facts[rank];
  uint64_t mask = 0;
  for (int r = 0; r < world; ++r) {
    int pdev = -1, can = 0;
    if (r == rank || same_gpu(h->facts[r], mine)) can = 1;
    else if (hipDeviceGetByPCIBusId(&pdev, h->facts[r].bus) != hipSuccess || hipDeviceCanAccessPeer(&can, dev, pdev) != hipSuccess) { can = 0; (void)hipGetLastError(); }
    if (can) mask |= (uint64_t)1 << r;
  }
  mine.peer_mask = mask;
  mine.has_rccl = !any_shared_gpu(h->facts, world) && rccl().handle != nullptr ? 1u : 0u;
  if (!peer.barrier(err)) return -1;
  std::memcpy(table, h->facts, sizeof(RankFacts) * (size_t)world);
  return peer.barrier(err) ? 0 : -1;      // nobody republishes (a later comm_create_from_region on this region) before everyone has read
}

Comm* comm_create_in_region(void* region, int rank, int world, Transport transport, uint32_t n_cams, std::string& err) {
  RegionHeader* h = checked_region(region, rank, world, err);
  if (!h) return nullptr;
  RegionPeer peer;
  peer.h = h; peer.world = world;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { err = "hipGetDevice failed"; h->abort_flag.store(1); return nullptr; }
  return create_transport(h, peer, rank, world, dev, transport, n_cams, err);
}

}  // namespace gbp
