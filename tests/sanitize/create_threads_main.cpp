// gbp_create from several host threads at once, without a device (tests/test_host_sanitizers.py: once under ThreadSanitizer, once under
// AddressSanitizer + UBSan; the host side of the library with tests/sanitize/kernel_stubs.cpp in place of the device code).
// gbp_last_error(NULL) is the creation error OF THE CALLING THREAD (csrc/gbp_api_ctx.cpp: create_error): eight threads make creations
// that fail for different reasons — an empty edge list, n_cams = 0, an index out of range, a bad shard, and a valid problem that finds
// no device —, wait for each other, and then each must read the text of ITS OWN failure, round after round; between them they call
// gbp_default_params and gbp_destroy(NULL).  Exit code 0 and "create_threads: ok" = every thread saw its own text; the sanitizers'
// reports are the test's business.
#include "../../include/gbp_mi355x.h"
#include "../../include/gbp_mi355x_multi.h"

#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace {

constexpr int kThreads = 8, kRounds = 40, kCases = 5;
const char* const kText[kCases] = {"null or empty problem", "null or empty problem", "index out of range", "bad shard", "no HIP device"};
const int kStatus[kCases] = {GBP_ERR_INVALID, GBP_ERR_INVALID, GBP_ERR_INVALID, GBP_ERR_INVALID, GBP_ERR_NO_DEVICE};

std::atomic<int> g_arrived{0};
std::atomic<int> g_failures{0};

void wait_for_all(int round) {      // every thread has arrived `round` times
  g_arrived.fetch_add(1, std::memory_order_acq_rel);
  while (g_arrived.load(std::memory_order_acquire) < round * kThreads) std::this_thread::yield();
}

int failing_create(int which) {
  static const uint32_t cam[6] = {0, 0, 0, 1, 1, 1}, lmk[6] = {0, 1, 2, 0, 1, 2}, lmk_bad[6] = {0, 1, 7, 0, 1, 2};
  static const float K[9] = {500, 0, 320, 0, 500, 240, 0, 0, 1};
  gbp_problem pr{};
  pr.n_cams = 2; pr.n_lmks = 3; pr.n_edges = 6; pr.cam_id = cam; pr.lmk_id = lmk;
  std::memcpy(pr.K, K, sizeof(K));
  gbp_shard sh{2, 2, 0, 3};      // rank >= world
  gbp_params prm;
  gbp_default_params(&prm);
  if (prm.min_linear_iters != 10 || prm.persistent != 0) return 1;
  gbp_ctx* c = nullptr;
  switch (which) {
    case 0: pr.n_edges = 0; break;           // an empty cam_id / lmk_id
    case 1: pr.n_cams = 0; break;
    case 2: pr.lmk_id = lmk_bad; break;      // refused by the layout builder
    case 3: break;                           // (the shard)
    default: break;                          // valid: the device order is built, then no device is found
  }
  const int rc = gbp_create(&pr, which % 2 ? &prm : nullptr, which == 3 ? &sh : nullptr, &c);
  gbp_destroy(nullptr);
  return (rc == kStatus[which] && c == nullptr) ? 0 : 1;
}

void worker(int t, bool have_device) {
  for (int r = 0; r < kRounds; ++r) {
    int which = (t + r) % kCases;
    if (which == 4 && have_device) which = 2;      // (a ctx on a device would run into the aborting launchers of the stubs)
    int bad = failing_create(which);
    wait_for_all(2 * r + 1);                       // everyone has failed in their own way ...
    const std::string mine = gbp_last_error(nullptr);
    if (mine.find(kText[which]) == std::string::npos) {
      std::fprintf(stderr, "thread %d round %d: expected \"%s\" in gbp_last_error(NULL), read \"%s\"\n", t, r, kText[which], mine.c_str());
      ++bad;
    }
    g_failures.fetch_add(bad, std::memory_order_relaxed);
    wait_for_all(2 * r + 2);                       // ... and read before the next round overwrites
  }
}

}  // namespace

int main() {
  const bool have_device = gbp_device_count() != 0;
  if (have_device) std::printf("create_threads: %d HIP device(s) visible: the creation without a device is left out\n", gbp_device_count());
  if (std::strlen(gbp_last_error(nullptr)) != 0) { std::fprintf(stderr, "a thread that has not failed has an error text\n"); return 1; }
  std::vector<std::thread> threads;
  for (int t = 0; t < kThreads; ++t) threads.emplace_back(worker, t, have_device);
  for (std::thread& th : threads) th.join();
  if (std::strlen(gbp_last_error(nullptr)) != 0) { std::fprintf(stderr, "the main thread reads another thread's error\n"); return 1; }
  if (g_failures.load() != 0) { std::fprintf(stderr, "create_threads: %d failures\n", g_failures.load()); return 1; }
  std::puts("create_threads: ok");
  return 0;
}
