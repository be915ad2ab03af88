// cli_common.hpp — shared host driver code of the `ba` and `slam` executables.
//
// Keeps the command-line contract of the reference's two programs (flag names and defaults of
// ba/ba.cpp:394-476 and ba/slam.cpp:394-476, stdout lines of ba.cpp:996,1004,1026-1028 and
// slam.cpp:1073-1076) on top of the C-ABI instead of a Poplar engine.  Boost.Program_options is
// replaced by a small `--name value` / `--name=value` parser.  Differences, all deliberate:
//   * `--help` prints the options and exits 0 (the reference throws an uncaught exception, ba.cpp:469-472);
//   * a malformed data file is an error (the reference only prints "Invalid UW data file.");
//   * `--ipus N` is kept as an alias of `--gpus N`: N > 1 starts one process per GPU (forked before anything touches
//     HIP), landmark-sharded, camera partial sums all-gathered once per iteration by RCCL over xGMI
//     (ba.cpp:414-417,617-649 spread one Poplar graph over N x 1216 tiles); `--camspertile` is accepted and ignored;
//   * `--seed S` makes the initialisation-noise flags reproducible (the reference seeds from the clock,
//     dataio.cpp:334,349,406); `--eval_every K` thins the per-iteration read-back + metric (default 1);
//   * `--lmk_init triangulate` takes the landmarks' prior means and strengths from the observations and the camera prior means
//     (libgbp_mi355x_seed.so) instead of the file's `points` section, which is then not used at all;
//   * slam's `--kf_init resect` refines every new keyframe's pose guess — the reference's copy of its predecessor — against the
//     landmarks mapped so far (libgbp_mi355x_resect.so) before its prior is set; `--kf_init locate` first finds the pose with no
//     guess at all, and the observations that agree with it (libgbp_mi355x_locate.so), and resects from there over those
//     observations — where that fails the keyframe takes the `resect` path; the default, `copy`, is the reference's.
#pragma once
#include "../../include/gbp_mi355x.h"
#include "../../include/gbp_mi355x_multi.h"       // --ipus N: one forked rank per GPU
#include "gbp_transport.hpp"                      // --transport: the names of gbp_comm_init's transport numbers
#include "gbp_metric_gather.hpp"                  // --ipus N: the cross-rank sum of a burst's metric records
#include "../../include/gbp_mi355x_post.h"        // --cov_file: means and marginal covariances of the beliefs (libgbp_mi355x_post.so)
#include "../../include/gbp_mi355x_seed.h"        // --lmk_init triangulate: landmark priors from observations (libgbp_mi355x_seed.so)
#include "../../include/gbp_mi355x_resect.h"      // slam --kf_init resect: the new keyframe's pose from the mapped landmarks (libgbp_mi355x_resect.so)
#include "../../include/gbp_mi355x_locate.h"      // slam --kf_init locate: the new keyframe's pose with no guess (libgbp_mi355x_locate.so)
#include "../../include/gbp_mi355x_compat.h"      // MetricPipe: the metric in two halves (gbp_iterate_eval / gbp_eval_end), so that printing overlaps the next iterations

#include <hip/hip_runtime_api.h>                  // --cov_file: the device arrays the readout works on (nothing else here touches HIP)

#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <sched.h>
#include <chrono>
#include <cmath>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iostream>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include <signal.h>
#include <sys/mman.h>
#include <sys/wait.h>
#include <unistd.h>

namespace cli {

// Where a run spends its wall time, from exec to exit (--profile: the `startup` object of gbp_profile.json; the "Total time" line):
// for the shipped sequences the iteration loop is a few per cent of what a user of ./ba waits for (profiles/r06_configs.md).
struct Phases {
  using clk = std::chrono::steady_clock;
  clk::time_point t_main = clk::now(), last = t_main;
  double exec_to_main_s = 0;                                  // exec -> main(): the dynamic loader (libamdhip64 and what it pulls in)
  std::vector<std::pair<std::string, double>> v;              // phase, seconds — in order
  std::string create_info;                                    // gbp_create's own breakdown (gbp_last_error(ctx) right after it)
  std::string comm_info;                                      // gbp_comm_describe of a sharded run (JSON): the transport, who chose it, what was measured
  Phases() {
    // start time of the process (clock ticks since boot, /proc/self/stat field 22) against the time since boot now: 10 ms resolution
    double up = 0;
    if (FILE* f = std::fopen("/proc/uptime", "r")) { if (std::fscanf(f, "%lf", &up) != 1) up = 0; std::fclose(f); }
    if (FILE* f = std::fopen("/proc/self/stat", "r")) {
      char buf[1024];
      const size_t n = std::fread(buf, 1, sizeof(buf) - 1, f);
      std::fclose(f);
      buf[n] = 0;
      if (const char* p = std::strrchr(buf, ')')) {          // the fields behind "(comm)": state is field 3
        unsigned long long start = 0;
        int field = 2;
        for (const char* q = p + 1; *q && field < 22; ++q)
          if (*q == ' ') { ++field; if (field == 22) start = std::strtoull(q + 1, nullptr, 10); }
        const long hz = sysconf(_SC_CLK_TCK);
        if (start && hz > 0 && up > 0) exec_to_main_s = std::max(0.0, up - (double)start / (double)hz);
      }
    }
  }
  void mark(const char* name) {
    const auto n = clk::now();
    v.emplace_back(name, std::chrono::duration<double>(n - last).count());
    last = n;
  }
  double since_exec() const { return exec_to_main_s + std::chrono::duration<double>(clk::now() - t_main).count(); }
  double get(const char* name) const { for (const auto& p : v) if (p.first == name) return p.second; return 0; }
};
inline Phases& phases() { static Phases p; return p; }

struct Options {
  std::string bal_file;
  int n_iters = 1500;           // ba only
  int iters_between_kfs = 700;  // slam only
  bool profile = false;
  int gpus = 1;
  int cams_per_tile = 1;
  float transnoise = 0.f, rotnoise = 0.f, lmktrans_noise = 0.f;
  bool av_depth_on = false;
  float av_depth = 1.f;
  float reproj_meas_var = 4.f;
  float prior_std_weaker_factor = 100.f;
  float first_cam_prior_std = 0.01f;
  float steps = 5.f;
  int iters_before_damping = 15;
  bool verbose = false;
  unsigned long long seed = 0;
  int eval_every = 1;
  int transport = (int)gbp::Transport::Auto;   // --transport (gbp_transport.hpp): what gbp_comm_init is given
  std::string out_file;         // --out_file: write the refined problem (belief means) in the input's format
  std::string cov_file;         // --cov_file: write every variable's mean and marginal covariance (gbp_post_moments)
  bool triangulate = false;     // --lmk_init triangulate (default: file)
  bool kf_resect = false;       // slam --kf_init resect or locate (default: copy)
  bool kf_locate = false;       // slam --kf_init locate: location in front of the resection
  bool force_sharded = false;   // --force_sharded: run the multi-rank code path (fork, shard ctx, communicator) with one rank
};

inline void usage(bool slam) {
  std::cout << "Options:\n"
               "  --help                         Show command help\n"
               "  --bal_file arg                 Set the bal file\n";
  if (slam) std::cout << "  --iters_between_kfs arg (=700) Number of iterations of GBP between new keyframes\n";
  else std::cout << "  --n_iters arg (=1500)          Number of iterations of synchronous GBP\n";
  std::cout << "  --profile arg (=0)             Save profile report after execution\n"
               "  --gpus arg (=1)                Number of GPUs (alias: --ipus)\n"
               "  --camspertile arg (=1)         accepted for compatibility, ignored\n"
               "  --tn arg (=0)                  Set keyframe translation noise value\n"
               "  --rn arg (=0)                  Set keyframe rotation noise value\n"
               "  --ltn arg (=0)                 Set landmark translation noise noise value\n"
               "  --avdepth_on arg (=0)          initialise landmarks at a depth in front of the first observing keyframe\n"
               "  --avdepth arg (=1)             Average depth\n"
               "  --reproj_meas_var arg (=4)     Variance of the reprojection measurement model\n"
               "  --prior_std_weaker_factor arg (=100)\n"
               "  --first_cam_prior_std arg (=0.01)\n"
               "  --steps arg (=5)               The priors are gradually weakened over this many steps\n"
               "  --undamped_start arg (=15)     Number of undamped iterations before damping GBP\n"
               "  --v arg (=0)                   Verbose: print beliefs\n"
               "  --seed arg (=0)                seed of the initialisation noise (0 = from the clock)\n"
               "  --eval_every arg (=1)          read back + evaluate every K iterations\n"
               "  --transport arg (=auto)        exchange between ranks: auto | rccl | host | p2p | p2p-slices | measured (host, p2p, p2p-slices: ranks may\n"
               "                                 share a GPU; host is also spelled host-staged; measured: time every transport the ranks\n"
               "                                 can form, keep the fastest)\n"
               "  --lmk_init arg (=file)         landmark prior means and strengths: file (the file's points) | triangulate (from the\n"
               "                                 observations and the camera prior means; the file's points are not used; one GPU)\n";
  if (slam) std::cout << "  --kf_init arg (=copy)          a new keyframe's pose guess: copy (its predecessor's pose) | resect (the copy, refined\n"
                         "                                 against the landmarks mapped so far; one GPU) | locate (found with no guess\n"
                         "                                 among wrong matches, then resected over the matches that agree; one GPU)\n";
  std::cout << "  --out_file arg                write the refined cameras / landmarks (belief means) in the input's format\n"
               "  --cov_file arg                 write every camera's / landmark's mean and marginal covariance: line 1 `C L`, then per camera\n"
               "                                 6 + 36 values, per landmark 3 + 9 values (covariances row-major)\n";
}

// returns 0 = run, 1 = exit with code 0 (help), 2 = exit with code 1 (error), 3 = exit with code 2 (a --kf_init that cannot be run)
inline int parse(int argc, char** argv, bool slam, Options& o) {
  std::map<std::string, std::string> kv;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    if (a.rfind("--", 0) != 0) { std::cerr << "unrecognised argument '" << a << "'\n"; return 2; }
    a = a.substr(2);
    if (a == "help") { usage(slam); return 1; }
    std::string val;
    const size_t eq = a.find('=');
    if (eq != std::string::npos) { val = a.substr(eq + 1); a = a.substr(0, eq); }
    else if (i + 1 < argc) val = argv[++i];
    else { std::cerr << "the required argument for option '--" << a << "' is missing\n"; return 2; }
    kv[a] = val;
  }
  auto B = [](const std::string& s) { return s == "1" || s == "true" || s == "on" || s == "yes"; };
  try {
    for (auto& p : kv) {
      const std::string &k = p.first, &v = p.second;
      if (k == "bal_file") o.bal_file = v;
      else if (k == "n_iters" && !slam) o.n_iters = std::stoi(v);
      else if (k == "iters_between_kfs" && slam) o.iters_between_kfs = std::stoi(v);
      else if (k == "profile") o.profile = B(v);
      else if (k == "ipus" || k == "gpus") o.gpus = std::stoi(v);
      else if (k == "camspertile") o.cams_per_tile = std::stoi(v);
      else if (k == "tn") o.transnoise = std::stof(v);
      else if (k == "rn") o.rotnoise = std::stof(v);
      else if (k == "ltn") o.lmktrans_noise = std::stof(v);
      else if (k == "avdepth_on") o.av_depth_on = B(v);
      else if (k == "avdepth") o.av_depth = std::stof(v);
      else if (k == "reproj_meas_var") o.reproj_meas_var = std::stof(v);
      else if (k == "prior_std_weaker_factor") o.prior_std_weaker_factor = std::stof(v);
      else if (k == "first_cam_prior_std") o.first_cam_prior_std = std::stof(v);
      else if (k == "steps") o.steps = std::stof(v);
      else if (k == "undamped_start") o.iters_before_damping = std::stoi(v);
      else if (k == "v") o.verbose = B(v);
      else if (k == "seed") o.seed = std::stoull(v);
      else if (k == "eval_every") o.eval_every = std::max(1, std::stoi(v));
      else if (k == "force_sharded") o.force_sharded = B(v);
      else if (k == "lmk_init") {
        if (v != "file" && v != "triangulate") { std::cerr << "--lmk_init: expected file or triangulate\n"; return 2; }
        o.triangulate = v == "triangulate";
      }
      else if (k == "kf_init" && slam) {
        if (v != "copy" && v != "resect" && v != "locate") { std::cerr << "--kf_init: expected copy, resect or locate\n"; return 3; }
        o.kf_resect = v == "resect" || v == "locate";
        o.kf_locate = v == "locate";
      }
      else if (k == "out_file") o.out_file = v;
      else if (k == "cov_file") o.cov_file = v;
      else if (k == "transport") {
        using T = gbp::Transport;
        o.transport = v == "rccl" ? (int)T::Rccl : (v == "host" || v == "host-staged") ? (int)T::HostStaged : v == "p2p" ? (int)T::P2p : v == "p2p-slices" ? (int)T::P2pSlices :
                      v == "measured" ? (int)T::Measured : v == "auto" ? (int)T::Auto : std::stoi(v);
      }
      else { std::cerr << "unrecognised option '--" << k << "'\n"; return 2; }
    }
  } catch (const std::exception&) {
    std::cerr << "invalid option value\n";
    return 2;
  }
  if (o.bal_file.empty()) { std::cerr << "the option '--bal_file' is required but missing\n"; return 2; }
  if (o.triangulate && o.av_depth_on) { std::cerr << "--lmk_init triangulate and --avdepth_on both place the landmarks: choose one\n"; return 2; }
  if (o.triangulate && (o.gpus > 1 || o.force_sharded)) { std::cerr << "--lmk_init triangulate runs on one GPU\n"; return 2; }
  if (o.kf_resect && (o.gpus > 1 || o.force_sharded)) { std::cerr << "--kf_init " << (o.kf_locate ? "locate" : "resect") << " runs on one GPU\n"; return 3; }
  return 0;
}

// ---- problem data (what ba.cpp:489-604 builds on the host) -----------------------------------------
struct Problem {
  gbp_bal bal{};
  std::vector<uint32_t> cam_id, lmk_id;
  std::vector<double> obs, cams, pts;
  std::vector<float> K, meas, var, cam_file, lmk_file, cam_mean, lmk_mean;
  std::vector<float> cpe, cpl, lpe, lpl, cscale, lscale, damping;
  std::vector<int32_t> count;
  std::vector<uint32_t> active, cwf, lwf;
  gbp_problem prob{};
};

inline int load_problem(const Options& o, Problem& P) {
  const bool trace = std::getenv("GBP_HOST_TRACE") != nullptr;      // milliseconds of every step on stderr
  auto t0 = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!trace) return;
    const auto t1 = std::chrono::steady_clock::now();
    std::fprintf(stderr, "load_problem: %s %.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  };
  if (gbp_bal_read_header(o.bal_file.c_str(), &P.bal) != GBP_OK) {
    std::cerr << "ERROR: unable to open file " << o.bal_file << "\n";  // ba.cpp:484-487
    return 1;
  }
  const uint32_t C = P.bal.n_cams, L = P.bal.n_lmks, E = P.bal.n_edges;
  P.cam_id.resize(E); P.lmk_id.resize(E); P.obs.resize(2 * (size_t)E); P.cams.resize(6 * (size_t)C); P.pts.resize(3 * (size_t)L);
  P.bal.cam_id = P.cam_id.data(); P.bal.lmk_id = P.lmk_id.data(); P.bal.observations = P.obs.data();
  P.bal.cameras = P.cams.data(); P.bal.points = P.pts.data();
  lap("header + arrays");
  if (gbp_bal_read(o.bal_file.c_str(), &P.bal) != GBP_OK) {
    std::cerr << "Invalid UW data file.\nERROR: unable to read file " << o.bal_file << "\n";
    return 1;
  }
  lap("gbp_bal_read");
  P.K = {(float)P.bal.fx, 0.f, (float)P.bal.cx, 0.f, (float)P.bal.fy, (float)P.bal.cy, 0.f, 0.f, 1.f};  // ba.cpp:494-495
  P.meas.resize(2 * (size_t)E);
  for (size_t i = 0; i < 2 * (size_t)E; ++i) P.meas[i] = (float)P.obs[i];
  P.var.assign(E, o.reproj_meas_var);
  P.cam_file.resize(6 * (size_t)C); P.lmk_file.resize(3 * (size_t)L);
  for (size_t i = 0; i < P.cam_file.size(); ++i) P.cam_file[i] = (float)P.cams[i];
  for (size_t i = 0; i < P.lmk_file.size(); ++i) P.lmk_file[i] = (float)P.pts[i];
  P.cam_mean = P.cam_file; P.lmk_mean = P.lmk_file;
  P.prob.n_cams = C; P.prob.n_lmks = L; P.prob.n_edges = E; P.prob.cam_id = P.cam_id.data(); P.prob.lmk_id = P.lmk_id.data();
  std::memcpy(P.prob.K, P.K.data(), 9 * sizeof(float));

  lap("measurements, variances, means as float");
  // ba.cpp:536-548; the reference seeds from the clock (dataio.cpp:334,349,406): --seed 0 does the same
  const unsigned long long seed = o.seed ? o.seed : (unsigned long long)std::chrono::system_clock::now().time_since_epoch().count();
  if (o.transnoise != 0.f)
    std::cout << "\nAdding Gaussian noise with std: " << o.transnoise << "m to the keyframe translaton intialisations\n";
  if (o.rotnoise != 0.f)
    std::cout << "Adding Gaussian noise with std: " << o.rotnoise << " to the keyframe rotation intialisations\n";
  const bool lmk_noise = o.lmktrans_noise != 0.f && !o.av_depth_on && !o.triangulate;      // (triangulate: the file's points are not used, noised or not)
  if (lmk_noise)
    std::cout << "Adding Gaussian noise with std: " << o.lmktrans_noise << "m to the landmark intialisations\n";
  gbp_init_add_noise(C, L, o.transnoise, o.rotnoise, lmk_noise ? o.lmktrans_noise : 0.f, seed, P.cam_mean.data(), P.lmk_mean.data());
  if (o.av_depth_on) {
    std::cout << "Initialising all landmarks at an average depth of: " << o.av_depth << "\n";
    gbp_init_av_depth(&P.prob, P.cam_mean.data(), P.lmk_mean.data());
  }

  lap("initialisation options");
  P.cpe.resize(6 * (size_t)C); P.cpl.resize(36 * (size_t)C); P.lpe.resize(3 * (size_t)L); P.lpl.resize(9 * (size_t)L);
  gbp_set_prior_lambda(&P.prob, o.reproj_meas_var, P.cam_file.data(), P.lmk_file.data(), P.cam_mean.data(), P.lmk_mean.data(),
                       P.cpe.data(), P.cpl.data(), P.lpe.data(), P.lpl.data());
  lap("gbp_set_prior_lambda");
  P.cscale.resize(C); P.lscale.resize(L);
  gbp_prior_scalings(C, L, P.cpl.data(), o.steps, o.prior_std_weaker_factor, o.first_cam_prior_std, P.cscale.data(), P.lscale.data());
  std::cout << "Completed loading data!\n";
  P.damping.assign(E, 0.f);
  P.count.assign(E, -o.iters_before_damping);  // ba.cpp:581
  lap("scalings, damping state");
  // mu / oldmu: the reference uploads 9 E zeros for each (ba.cpp:582-583); gbp_upload takes NULL for "zeros" — 72 MB per million factors
  // that are neither allocated nor compared here
  return 0;
}

inline gbp_state_in state_in(const Problem& P) {
  gbp_state_in s{};
  s.damping = P.damping.data(); s.damping_count = P.count.data(); s.mu = nullptr; s.oldmu = nullptr;
  s.active_flag = P.active.data(); s.cam_scaling = P.cscale.data(); s.lmk_scaling = P.lscale.data();
  s.cam_weaken_flag = P.cwf.data(); s.lmk_weaken_flag = P.lwf.data();
  s.cam_priors_eta = P.cpe.data(); s.cam_priors_lambda = P.cpl.data(); s.lmk_priors_eta = P.lpe.data();
  s.lmk_priors_lambda = P.lpl.data(); s.measurements = P.meas.data(); s.meas_variances = P.var.data();
  return s;
}

struct Readback {
  std::vector<float> cbe, cbl, lbe, lbl;
  gbp_state_out out{};
  Readback(uint32_t C, uint32_t L) : cbe(6 * (size_t)C), cbl(36 * (size_t)C), lbe(3 * (size_t)L), lbl(9 * (size_t)L) {
    out.cam_beliefs_eta = cbe.data(); out.cam_beliefs_lambda = cbl.data();
    out.lmk_beliefs_eta = lbe.data(); out.lmk_beliefs_lambda = lbl.data();
  }
};

inline void print_verbose(const Readback& r) {  // ba.cpp:1030-1051
  std::cout << "\nKeyframe Eta beliefs: \n";
  for (unsigned i = 0; i < 6; ++i) std::printf("%.12f  ", r.cbe[6 + i]);
  std::cout << "\nKeyframe Lambda beliefs: \n";
  for (unsigned i = 0; i < 36; ++i) std::printf("%.12f  ", r.cbl[36 + i]);
  std::cout << '\n';
  std::cout << "\nLandmark Eta beliefs: \n";
  for (unsigned i = 0; i < 12; ++i) std::printf("%.12f  ", r.lbe[i]);
  std::cout << "\nLandmark Lambda beliefs: \n";
  for (unsigned i = 0; i < 18; ++i) std::printf("%.12f  ", r.lbl[i]);
  std::cout << '\n';
  std::fflush(stdout);
}

// ---- --lmk_init triangulate: the landmark priors from the observations (include/gbp_mi355x_seed.h) ----------------------
// The device arrays of the seeding calls, allocated once.  Everything goes through the default stream with blocking copies, as
// write_cov_file does.  start(): every landmark from ALL its observations at the camera prior means — the landmark priors of the
// upload, and the points the camera priors' strengths are taken at (gbp_set_prior_lambda's "file" points: the file's are not used).
// keyframe(): slam's per-keyframe step — the new camera's prior eta (gbp_seed_keyframe in place of gbp_slam_initialise_new_kf, the
// same bits), then the landmarks this keyframe activated from every now-active observation, at the belief means of the cameras so
// far and the new camera's pose guess; every other prior passes through.
struct Seeder {
  uint32_t C = 0, L = 0, E = 0;
  std::vector<uint32_t> lmk_start, lmk_edges, status, select;
  std::vector<float> cam_mean;
  std::vector<double> cams64, pts64;
  gbp_seed_options opts{};
  char* base = nullptr;
  uint32_t *d_cam_id = nullptr, *d_start = nullptr, *d_edges = nullptr, *d_active = nullptr, *d_select = nullptr, *d_status = nullptr;
  float *d_meas = nullptr, *d_cam_mean = nullptr, *d_lmk_mean = nullptr, *d_lpe = nullptr, *d_lpl = nullptr;
  float *d_cbe = nullptr, *d_cbl = nullptr, *d_cpl = nullptr, *d_cpe = nullptr, *d_guess = nullptr;
  void* d_ws = nullptr;
  ~Seeder() { if (base) (void)hipFree(base); }
  static bool ok(hipError_t e, const char* what) {
    if (e != hipSuccess) std::cerr << "--lmk_init triangulate: " << what << " failed: " << hipGetErrorString(e) << "\n";
    return e == hipSuccess;
  }
  static bool seed_ok(int rc) {
    if (rc != GBP_OK) std::cerr << "--lmk_init triangulate: " << gbp_seed_last_error() << "\n";
    return rc == GBP_OK;
  }
  template <class T> bool up(T* d, const T* h, size_t n) { return n == 0 || ok(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy"); }
  template <class T> bool down(T* h, const T* d, size_t n) { return n == 0 || ok(hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy"); }

  int init(const Options& o, const Problem& P) {
    C = P.bal.n_cams; L = P.bal.n_lmks; E = P.bal.n_edges;
    gbp_seed_default_options(&opts);
    opts.reproj_meas_var = o.reproj_meas_var;
    lmk_start.resize((size_t)L + 1); lmk_edges.resize(E); status.resize(L); select.resize(L);
    if (!seed_ok(gbp_seed_index(L, E, P.lmk_id.data(), lmk_start.data(), lmk_edges.data()))) return 1;
    size_t at = 0;
    const auto take = [&at](size_t bytes) { const size_t here = at; at += (bytes + 255) & ~(size_t)255; return here; };
    const size_t o_ws = take(gbp_seed_workspace_bytes(C)), o_cam_id = take(4 * (size_t)E), o_start = take(4 * ((size_t)L + 1)), o_edges = take(4 * (size_t)E),
                 o_active = take(4 * (size_t)E), o_select = take(4 * (size_t)L), o_status = take(4 * (size_t)L), o_meas = take(8 * (size_t)E),
                 o_cam_mean = take(24 * (size_t)C), o_lmk_mean = take(12 * (size_t)L), o_lpe = take(12 * (size_t)L), o_lpl = take(36 * (size_t)L),
                 o_cbe = take(24 * (size_t)C), o_cbl = take(144 * (size_t)C), o_cpl = take(144 * (size_t)C), o_cpe = take(24 * (size_t)C), o_guess = take(24);
    if (!ok(hipMalloc(reinterpret_cast<void**>(&base), at), "hipMalloc")) return 1;
    d_ws = base + o_ws;
    const auto u32 = [this](size_t off) { return reinterpret_cast<uint32_t*>(base + off); };
    const auto f32 = [this](size_t off) { return reinterpret_cast<float*>(base + off); };
    d_cam_id = u32(o_cam_id); d_start = u32(o_start); d_edges = u32(o_edges); d_active = u32(o_active); d_select = u32(o_select); d_status = u32(o_status);
    d_meas = f32(o_meas); d_cam_mean = f32(o_cam_mean); d_lmk_mean = f32(o_lmk_mean); d_lpe = f32(o_lpe); d_lpl = f32(o_lpl);
    d_cbe = f32(o_cbe); d_cbl = f32(o_cbl); d_cpl = f32(o_cpl); d_cpe = f32(o_cpe); d_guess = f32(o_guess);
    return up(d_cam_id, P.cam_id.data(), E) && up(d_start, lmk_start.data(), (size_t)L + 1) && up(d_edges, lmk_edges.data(), E) &&
                   up(d_meas, P.meas.data(), 2 * (size_t)E) ? 0 : 1;
  }

  // the landmarks `sel` (NULL: all) from the observations `active` (NULL: all) at the camera means `cams`, into P's landmark priors
  int landmarks(Problem& P, const float* cams, const uint32_t* active, const uint32_t* sel) {
    if (!up(d_cam_mean, cams, 6 * (size_t)C) || (active && !up(d_active, active, E)) || (sel && !up(d_select, sel, L)) ||
        !up(d_lmk_mean, P.lmk_mean.data(), 3 * (size_t)L) || !up(d_lpe, P.lpe.data(), 3 * (size_t)L) || !up(d_lpl, P.lpl.data(), 9 * (size_t)L))
      return 1;
    if (!seed_ok(gbp_seed_landmarks(nullptr, C, L, E, d_cam_id, d_start, d_edges, P.K.data(), d_cam_mean, d_meas, active ? d_active : nullptr,
                                    sel ? d_select : nullptr, &opts, d_ws, d_lmk_mean, d_lpe, d_lpl, d_status, nullptr)))
      return 1;
    return down(P.lmk_mean.data(), d_lmk_mean, 3 * (size_t)L) && down(P.lpe.data(), d_lpe, 3 * (size_t)L) && down(P.lpl.data(), d_lpl, 9 * (size_t)L) &&
                   down(status.data(), d_status, L) ? 0 : 1;
  }

  int start(const Options& o, Problem& P) {
    if (init(o, P)) return 1;
    std::fill(P.lmk_mean.begin(), P.lmk_mean.end(), 0.f);      // a landmark nobody observes: zero mean, zero prior (as the file rule gives it)
    std::fill(P.lpe.begin(), P.lpe.end(), 0.f);
    std::fill(P.lpl.begin(), P.lpl.end(), 0.f);
    if (landmarks(P, P.cam_mean.data(), nullptr, nullptr)) return 1;
    size_t n_tri = 0, n_placed = 0, n_none = 0;
    for (uint32_t l = 0; l < L; ++l) {
      if (status[l] & GBP_SEED_NO_VIEW) ++n_none;
      else if (status[l] & (GBP_SEED_ONE_VIEW | GBP_SEED_LOW_PARALLAX | GBP_SEED_NONFINITE)) ++n_placed;
      else ++n_tri;
    }
    std::cout << "Triangulating the landmarks from their observations: " << n_tri << " triangulated, " << n_placed
              << " placed on the ray of their first observation, " << n_none << " without an observation\n";
    // the camera priors by today's rule, their strengths taken at the seeded points; the landmark priors stay the seeded ones
    std::vector<float> lpe(P.lpe.size()), lpl(P.lpl.size());
    gbp_set_prior_lambda(&P.prob, o.reproj_meas_var, P.cam_file.data(), P.lmk_mean.data(), P.cam_mean.data(), P.lmk_mean.data(), P.cpe.data(),
                         P.cpl.data(), lpe.data(), lpl.data());
    gbp_prior_scalings(C, L, P.cpl.data(), o.steps, o.prior_std_weaker_factor, o.first_cam_prior_std, P.cscale.data(), P.lscale.data());
    return 0;
  }

  // slam: P.cpe / P.cpl / P.lpe / P.lpl hold gbp_read_priors' arrays, rb the beliefs, P.active / P.lwf the flags gbp_slam_update_flags left
  // refine (may be empty): called with the new camera's pose guess [6] once P.cpe holds its copied prior eta — --kf_init resect
  int keyframe(Problem& P, uint32_t data_counter, const float* cbe, const float* cbl, const float* lbe, const float* lbl,
               const std::function<int(float*)>& refine = {}) {
    if (!up(d_cbe, cbe, 6 * (size_t)C) || !up(d_cbl, cbl, 36 * (size_t)C) || !up(d_cpl, P.cpl.data(), 36 * (size_t)C) || !up(d_cpe, P.cpe.data(), 6 * (size_t)C))
      return 1;
    if (!seed_ok(gbp_seed_keyframe(nullptr, C, data_counter, data_counter + 1, d_cbe, d_cbl, d_cpl, d_cpe, d_guess))) return 1;
    cams64.resize(6 * (size_t)C); pts64.resize(3 * (size_t)L); cam_mean.resize(6 * (size_t)C);
    gbp_belief_means(C, L, cbe, cbl, lbe, lbl, cams64.data(), pts64.data());
    for (size_t i = 0; i < cam_mean.size(); ++i) cam_mean[i] = (float)cams64[i];
    if (!down(P.cpe.data(), d_cpe, 6 * (size_t)C) || !down(cam_mean.data() + 6 * ((size_t)data_counter + 1), d_guess, 6)) return 1;
    if (refine && refine(cam_mean.data() + 6 * ((size_t)data_counter + 1))) return 1;
    for (uint32_t l = 0; l < L; ++l) select[l] = P.lwf[l] != 0u;      // what this keyframe activated (gbp_slam_update_flags)
    return landmarks(P, cam_mean.data(), P.active.data(), select.data());
  }
};

struct Resecter;
// ---- slam --kf_init locate: in front of the resection, the new keyframe's pose with no guess (include/gbp_mi355x_locate.h) ----
// Works on the Resecter's device arrays, once keyframe() has filled them; its own: the mask, the count, the masked active flags.
// located(): 1 the camera was located and resected from there over the observations that agree (eta, guess and `line` are set),
// 0 it was not (the Resecter's arrays hold again what they held: the keyframe takes the resect path), -1 a call failed.
struct Locator {
  gbp_locate_options opts{};
  char* base = nullptr;
  uint32_t *d_inlier = nullptr, *d_ninl = nullptr, *d_masked = nullptr;
  std::vector<uint32_t> inlier, masked;
  ~Locator() { if (base) (void)hipFree(base); }
  int start(const Resecter& R);
  int located(Resecter& R, Problem& P, uint32_t kf, float* guess, std::string& line);
};

// ---- slam --kf_init resect: the new keyframe's pose from the landmarks mapped so far (include/gbp_mi355x_resect.h) -------
// The device arrays of the resection call, allocated once; blocking copies on the default stream, as Seeder.  keyframe(): camera
// data_counter + 1 alone, from its pose guess (`guess` [6], or the belief mean of camera data_counter where it is NULL), against the
// belief means of the landmarks that were mapped before this keyframe (lmk_active != 0 and lmk_weaken_flag == 0 as
// gbp_slam_update_flags left them), over the updated active flags.  P.cpe / P.cpl hold the priors with the COPIED eta of the new
// camera: a resected pose replaces that eta (prior Lambda . pose) and the guess; otherwise both stand.  `line` says which happened.
struct Resecter {
  Locator* locator = nullptr;   // --kf_init locate
  uint32_t C = 0, L = 0, E = 0;
  std::vector<uint32_t> cam_start, cam_edges, lmk_use, select;
  std::vector<float> cam_mean, lmk_mean;
  std::vector<double> cams64, pts64;
  gbp_resect_options opts{};
  char* base = nullptr;
  uint32_t *d_lmk_id = nullptr, *d_start = nullptr, *d_edges = nullptr, *d_active = nullptr, *d_use = nullptr, *d_select = nullptr, *d_status = nullptr,
           *d_views = nullptr;
  float *d_meas = nullptr, *d_cam_mean = nullptr, *d_lmk_mean = nullptr, *d_cpl = nullptr, *d_cpe = nullptr, *d_report = nullptr;
  ~Resecter() { if (base) (void)hipFree(base); }
  static bool ok(hipError_t e, const char* what) {
    if (e != hipSuccess) std::cerr << "--kf_init resect: " << what << " failed: " << hipGetErrorString(e) << "\n";
    return e == hipSuccess;
  }
  static bool resect_ok(int rc) {
    if (rc != GBP_OK) std::cerr << "--kf_init resect: " << gbp_resect_last_error() << "\n";
    return rc == GBP_OK;
  }
  template <class T> bool up(T* d, const T* h, size_t n) { return n == 0 || ok(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy"); }
  template <class T> bool down(T* h, const T* d, size_t n) { return n == 0 || ok(hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy"); }

  int start(const Options& o, const Problem& P) {
    C = P.bal.n_cams; L = P.bal.n_lmks; E = P.bal.n_edges;
    gbp_resect_default_options(&opts);
    opts.reproj_meas_var = o.reproj_meas_var;
    cam_start.resize((size_t)C + 1); cam_edges.resize(E); lmk_use.resize(L); select.assign(C, 0u);
    if (!resect_ok(gbp_resect_index(C, E, P.cam_id.data(), cam_start.data(), cam_edges.data()))) return 1;
    size_t at = 0;
    const auto take = [&at](size_t bytes) { const size_t here = at; at += (bytes + 255) & ~(size_t)255; return here; };
    const size_t o_lmk_id = take(4 * (size_t)E), o_start = take(4 * ((size_t)C + 1)), o_edges = take(4 * (size_t)E), o_active = take(4 * (size_t)E),
                 o_use = take(4 * (size_t)L), o_select = take(4 * (size_t)C), o_status = take(4 * (size_t)C), o_views = take(4 * (size_t)C),
                 o_meas = take(8 * (size_t)E), o_cam_mean = take(24 * (size_t)C), o_lmk_mean = take(12 * (size_t)L), o_cpl = take(144 * (size_t)C),
                 o_cpe = take(24 * (size_t)C), o_report = take(16 * (size_t)C);
    if (!ok(hipMalloc(reinterpret_cast<void**>(&base), at), "hipMalloc")) return 1;
    const auto u32 = [this](size_t off) { return reinterpret_cast<uint32_t*>(base + off); };
    const auto f32 = [this](size_t off) { return reinterpret_cast<float*>(base + off); };
    d_lmk_id = u32(o_lmk_id); d_start = u32(o_start); d_edges = u32(o_edges); d_active = u32(o_active); d_use = u32(o_use); d_select = u32(o_select);
    d_status = u32(o_status); d_views = u32(o_views); d_meas = f32(o_meas); d_cam_mean = f32(o_cam_mean); d_lmk_mean = f32(o_lmk_mean);
    d_cpl = f32(o_cpl); d_cpe = f32(o_cpe); d_report = f32(o_report);
    return up(d_lmk_id, P.lmk_id.data(), E) && up(d_start, cam_start.data(), (size_t)C + 1) && up(d_edges, cam_edges.data(), E) &&
                   up(d_meas, P.meas.data(), 2 * (size_t)E) ? 0 : 1;
  }

  int keyframe(Problem& P, uint32_t data_counter, const float* cbe, const float* cbl, const float* lbe, const float* lbl, const uint32_t* lmk_active,
               float* guess, std::string& line) {
    const uint32_t kf = data_counter + 1;
    cams64.resize(6 * (size_t)C); pts64.resize(3 * (size_t)L); cam_mean.resize(6 * (size_t)C); lmk_mean.resize(3 * (size_t)L);
    gbp_belief_means(C, L, cbe, cbl, lbe, lbl, cams64.data(), pts64.data());
    for (size_t i = 0; i < cam_mean.size(); ++i) cam_mean[i] = (float)cams64[i];
    for (size_t i = 0; i < lmk_mean.size(); ++i) lmk_mean[i] = (float)pts64[i];
    for (int i = 0; i < 6; ++i) cam_mean[6 * (size_t)kf + i] = guess ? guess[i] : cam_mean[6 * (size_t)data_counter + i];
    for (uint32_t l = 0; l < L; ++l) lmk_use[l] = lmk_active[l] != 0u && P.lwf[l] == 0u;
    std::fill(select.begin(), select.end(), 0u);
    select[kf] = 1u;
    if (!up(d_cam_mean, cam_mean.data(), 6 * (size_t)C) || !up(d_lmk_mean, lmk_mean.data(), 3 * (size_t)L) || !up(d_active, P.active.data(), E) ||
        !up(d_use, lmk_use.data(), L) || !up(d_select, select.data(), C) || !up(d_cpl, P.cpl.data(), 36 * (size_t)C) || !up(d_cpe, P.cpe.data(), 6 * (size_t)C))
      return 1;
    if (locator) {
      const int done = locator->located(*this, P, kf, guess, line);
      if (done) return done < 0 ? 1 : 0;
    }
    if (!resect_ok(gbp_resect_cameras(nullptr, C, L, E, d_lmk_id, d_start, d_edges, P.K.data(), d_lmk_mean, d_meas, d_active, d_use, d_select, &opts,
                                      d_cam_mean, d_cpl, d_cpe, nullptr, d_report, d_status, d_views)))
      return 1;
    uint32_t st = 0, n = 0;
    float report[4] = {0.f, 0.f, 0.f, 0.f};
    if (!down(&st, d_status + kf, 1) || !down(&n, d_views + kf, 1)) return 1;
    char buf[200];
    if (st & (GBP_RESECT_NO_VIEW | GBP_RESECT_FEW_VIEWS | GBP_RESECT_NONFINITE | GBP_RESECT_STALLED)) {
      std::snprintf(buf, sizeof(buf), "Keyframe %u: pose copied from keyframe %u (resection status %u, %u views)\n", kf + 1, kf, st, n);
    } else {
      if (!down(report, d_report + 4 * (size_t)kf, 4) || !down(P.cpe.data() + 6 * (size_t)kf, d_cpe + 6 * (size_t)kf, 6) ||
          (guess && !down(guess, d_cam_mean + 6 * (size_t)kf, 6)))
        return 1;
      std::snprintf(buf, sizeof(buf), "Keyframe %u: pose resected from %u views, cost %.6f -> %.6f (status %u)\n", kf + 1, n, report[0], report[1], st);
    }
    line = buf;
    return 0;
  }
};

inline int Locator::start(const Resecter& R) {
  gbp_locate_default_options(&opts);
  const size_t e_bytes = (4 * (size_t)R.E + 255) & ~(size_t)255, c_bytes = (4 * (size_t)R.C + 255) & ~(size_t)255;
  if (!Resecter::ok(hipMalloc(reinterpret_cast<void**>(&base), 2 * e_bytes + c_bytes), "hipMalloc")) return 1;
  d_inlier = reinterpret_cast<uint32_t*>(base); d_masked = reinterpret_cast<uint32_t*>(base + e_bytes); d_ninl = reinterpret_cast<uint32_t*>(base + 2 * e_bytes);
  inlier.resize(R.E); masked.resize(R.E);
  return 0;
}

inline int Locator::located(Resecter& R, Problem& P, uint32_t kf, float* guess, std::string& line) {
  const auto locate_ok = [](int rc) {
    if (rc != GBP_OK) std::cerr << "--kf_init locate: " << gbp_locate_last_error() << "\n";
    return rc == GBP_OK;
  };
  if (R.E && !Resecter::ok(hipMemset(d_inlier, 0, 4 * (size_t)R.E), "hipMemset")) return -1;
  if (!locate_ok(gbp_locate_cameras(nullptr, R.C, R.L, R.E, R.d_lmk_id, R.d_start, R.d_edges, P.K.data(), R.d_lmk_mean, R.d_meas, R.d_active, R.d_use,
                                    R.d_select, &opts, R.d_cam_mean, d_inlier, nullptr, R.d_status, R.d_views, d_ninl)))
    return -1;
  uint32_t st = 0, n = 0, n_in = 0;
  if (!R.down(&st, R.d_status + kf, 1)) return -1;
  if (st & (GBP_LOCATE_NO_VIEW | GBP_LOCATE_FEW_VIEWS | GBP_LOCATE_FEW_INLIERS | GBP_LOCATE_NO_HYPOTHESIS)) return 0;      // (nothing of the pose arrays was written)
  if (!R.down(&n, R.d_views + kf, 1) || !R.down(&n_in, d_ninl + kf, 1) || !R.down(inlier.data(), d_inlier, R.E)) return -1;
  for (uint32_t e = 0; e < R.E; ++e) masked[e] = P.active[e] == 1u && inlier[e] == 1u;
  if (!R.up(d_masked, masked.data(), R.E)) return -1;
  if (!Resecter::resect_ok(gbp_resect_cameras(nullptr, R.C, R.L, R.E, R.d_lmk_id, R.d_start, R.d_edges, P.K.data(), R.d_lmk_mean, R.d_meas, d_masked, R.d_use,
                                              R.d_select, &R.opts, R.d_cam_mean, R.d_cpl, R.d_cpe, nullptr, R.d_report, R.d_status, R.d_views)))
    return -1;
  uint32_t rst = 0;
  if (!R.down(&rst, R.d_status + kf, 1)) return -1;
  if (rst & (GBP_RESECT_NO_VIEW | GBP_RESECT_FEW_VIEWS | GBP_RESECT_NONFINITE | GBP_RESECT_STALLED))      // back to what keyframe() uploaded
    return R.up(R.d_cam_mean, R.cam_mean.data(), 6 * (size_t)R.C) && R.up(R.d_cpe, P.cpe.data(), 6 * (size_t)R.C) ? 0 : -1;
  float report[4] = {0.f, 0.f, 0.f, 0.f};
  if (!R.down(report, R.d_report + 4 * (size_t)kf, 4) || !R.down(P.cpe.data() + 6 * (size_t)kf, R.d_cpe + 6 * (size_t)kf, 6) ||
      (guess && !R.down(guess, R.d_cam_mean + 6 * (size_t)kf, 6)))
    return -1;
  char buf[240];
  std::snprintf(buf, sizeof(buf), "Keyframe %u: pose located from %u of %u views and resected, cost %.6f -> %.6f (status %u)\n", kf + 1, n_in, n, report[0], report[1], rst);
  line = buf;
  return 1;
}

// ---- one process per GPU (`--ipus N` / `--gpus N`) -------------------------------------------------------------------
struct RankCtx {
  int rank = 0, world = 1;
  void* region = nullptr;       // shared rendezvous / staging region (gbp_comm_region_*), world > 1 only
  void* metric_area = nullptr;  // shared [2 parities][world][gbp::kMetricBurstMax] metric records (gbp_metric_gather.hpp), mapped with the region
  float* result = nullptr;      // --out_file of a forked run: the shared belief arrays (result_floats), mapped with the region
  unsigned bursts = 0;          // bursts summed so far: the parity of the next one
  gbp_shard shard{0, 1, 0, 0};
};

// The result area of a forked run with --out_file / --cov_file: cam_beliefs_eta [6C], cam_beliefs_lambda [36C], lmk_beliefs_eta [3L], lmk_beliefs_lambda [9L]
inline size_t result_floats(uint32_t C, uint32_t L) { return 42 * (size_t)C + 12 * (size_t)L; }

inline bool wants_result(const Options& o) { return !o.out_file.empty() || !o.cov_file.empty(); }

constexpr int kLeaveNow = 2;      // write_solution: this rank failed where the others still wait for it — it leaves without meeting them again

// --out_file: the belief means in the format of the input, observations unchanged
inline int write_out_file(const Options& o, const Problem& P, const float* cbe, const float* cbl, const float* lbe, const float* lbl) {
  if (o.out_file.empty()) return 0;
  const uint32_t C = P.bal.n_cams, L = P.bal.n_lmks;
  std::vector<double> cams(6 * (size_t)C), pts(3 * (size_t)L);
  gbp_belief_means(C, L, cbe, cbl, lbe, lbl, cams.data(), pts.data());
  gbp_bal res = P.bal;
  res.cameras = cams.data(); res.points = pts.data();
  if (gbp_bal_write(o.out_file.c_str(), &res) != GBP_OK) { std::cerr << "ERROR: unable to write " << o.out_file << "\n"; return 1; }
  std::cout << "Refined problem written to " << o.out_file << "\n";
  return 0;
}

// --cov_file: mean and marginal covariance of every variable from the beliefs in host arrays (a forked run's gathered ones alike), through
// the readout library on the current device.  Line 1 `C L`, then per camera 6 + 36 values, per landmark 3 + 9 values, %.9g.  Nothing on stdout.
inline int write_cov_file(const Options& o, const Problem& P, const float* cbe, const float* cbl, const float* lbe, const float* lbl) {
  if (o.cov_file.empty()) return 0;
  const uint32_t C = P.bal.n_cams, L = P.bal.n_lmks;
  const size_t n_in = result_floats(C, L), n = 2 * n_in;
  struct Dev {
    float* p = nullptr;
    ~Dev() { if (p) (void)hipFree(p); }
  } dev;
  std::vector<float> host(n_in);
  auto hip_ok = [](hipError_t e, const char* what) {
    if (e != hipSuccess) std::cerr << "--cov_file: " << what << " failed: " << hipGetErrorString(e) << "\n";
    return e == hipSuccess;
  };
  if (!hip_ok(hipMalloc(reinterpret_cast<void**>(&dev.p), n * sizeof(float)), "hipMalloc")) return 1;
  float *d_cbe = dev.p, *d_cbl = d_cbe + 6 * (size_t)C, *d_lbe = d_cbl + 36 * (size_t)C, *d_lbl = d_lbe + 3 * (size_t)L;
  float *d_cm = dev.p + n_in, *d_cc = d_cm + 6 * (size_t)C, *d_lm = d_cc + 36 * (size_t)C, *d_lc = d_lm + 3 * (size_t)L;
  const struct { float* d; const float* h; size_t count; } in[4] = {{d_cbe, cbe, 6 * (size_t)C}, {d_cbl, cbl, 36 * (size_t)C}, {d_lbe, lbe, 3 * (size_t)L}, {d_lbl, lbl, 9 * (size_t)L}};
  for (const auto& a : in)
    if (a.count && !hip_ok(hipMemcpy(a.d, a.h, a.count * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy")) return 1;
  // (the default stream: the blocking copies before and behind the launch are ordered with it)
  if (gbp_post_moments(nullptr, C, L, d_cbe, d_cbl, d_lbe, d_lbl, d_cm, d_cc, d_lm, d_lc, nullptr, nullptr) != GBP_OK) {
    std::cerr << "--cov_file: " << gbp_post_last_error() << "\n";
    return 1;
  }
  if (n_in && !hip_ok(hipMemcpy(host.data(), d_cm, n_in * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy")) return 1;
  FILE* f = std::fopen(o.cov_file.c_str(), "w");
  if (!f) { std::cerr << "ERROR: unable to write " << o.cov_file << "\n"; return 1; }
  std::fprintf(f, "%u %u\n", C, L);
  const float *cm = host.data(), *cc = cm + 6 * (size_t)C, *lm = cc + 36 * (size_t)C, *lc = lm + 3 * (size_t)L;
  auto line = [f](const float* mean, const float* cov, int w) {
    for (int i = 0; i < w; ++i) std::fprintf(f, "%.9g ", mean[i]);
    for (int i = 0; i < w * w; ++i) std::fprintf(f, i + 1 < w * w ? "%.9g " : "%.9g\n", cov[i]);
  };
  for (uint32_t c = 0; c < C; ++c) line(cm + 6 * (size_t)c, cc + 36 * (size_t)c, 6);
  for (uint32_t l = 0; l < L; ++l) line(lm + 3 * (size_t)l, lc + 9 * (size_t)l, 3);
  const bool bad = std::ferror(f) != 0;
  if (std::fclose(f) != 0 || bad) { std::cerr << "ERROR: unable to write " << o.cov_file << "\n"; return 1; }
  return 0;
}

// --out_file / --cov_file of a forked run.  Every rank reads its beliefs into the SHARED arrays: gbp_read on a sharded ctx writes the landmarks of the
// rank's own range at their global indices, so the ranks fill disjoint bytes; the cameras, replicated and bit-identical, are rank 0's.
// ONE barrier (the region's: release / acquire on its shared words, whatever the transport) lies between every rank's writes and rank 0's
// reads.  A rank whose read or barrier fails writes nothing and does not reach another barrier: the file never holds arrays that some
// rank has not filled.
inline int write_solution_ranks(const Options& o, const Problem& P, gbp_ctx* ctx, const RankCtx& rk) {
  const uint32_t C = P.bal.n_cams, L = P.bal.n_lmks;
  if (!rk.result) { std::cerr << "rank " << rk.rank << ": no shared result area for --out_file / --cov_file\n"; return kLeaveNow; }
  float *cbe = rk.result, *cbl = cbe + 6 * (size_t)C, *lbe = cbl + 36 * (size_t)C, *lbl = lbe + 3 * (size_t)L;
  gbp_state_out out{};
  out.lmk_beliefs_eta = lbe; out.lmk_beliefs_lambda = lbl;
  if (rk.rank == 0) { out.cam_beliefs_eta = cbe; out.cam_beliefs_lambda = cbl; }
  if (gbp_read(ctx, &out) != GBP_OK) { std::cerr << "rank " << rk.rank << ": gbp_read failed: " << gbp_last_error(ctx) << "\n"; return kLeaveNow; }
  if (gbp_comm_barrier(ctx) != GBP_OK) { std::cerr << "rank " << rk.rank << ": gbp_comm_barrier failed: " << gbp_last_error(ctx) << "\n"; return kLeaveNow; }
  if (rk.rank != 0) return 0;
  if (const int rc = write_out_file(o, P, cbe, cbl, lbe, lbl)) return rc;
  return write_cov_file(o, P, cbe, cbl, lbe, lbl);
}

// --out_file / --cov_file: the solution from the beliefs the run ends with.  A forked run (--ipus N, --force_sharded):
// write_solution_ranks.
inline int write_solution(const Options& o, const Problem& P, gbp_ctx* ctx, const RankCtx& rk) {
  if (!wants_result(o)) return 0;
  if (rk.region) return write_solution_ranks(o, P, ctx, rk);
  const uint32_t C = P.bal.n_cams, L = P.bal.n_lmks;
  std::vector<float> cbe(6 * (size_t)C), cbl(36 * (size_t)C), lbe(3 * (size_t)L), lbl(9 * (size_t)L);
  gbp_state_out out{};
  out.cam_beliefs_eta = cbe.data(); out.cam_beliefs_lambda = cbl.data(); out.lmk_beliefs_eta = lbe.data(); out.lmk_beliefs_lambda = lbl.data();
  if (gbp_read(ctx, &out) != GBP_OK) { std::cerr << "gbp_read failed: " << gbp_last_error(ctx) << "\n"; return 1; }
  if (const int rc = write_out_file(o, P, cbe.data(), cbl.data(), lbe.data(), lbl.data())) return rc;
  return write_cov_file(o, P, cbe.data(), cbl.data(), lbe.data(), lbl.data());
}

// A single-process run brings the HIP runtime up (120 - 240 ms: the first call that needs it) on a second thread WHILE the main thread
// reads the file and builds the priors — nothing for the shipped sequences (4 ms of host work), the runtime's whole start-up for a
// file of a million factors (1 - 2 s of parsing).  Never with --ipus N > 1: the ranks are forked before anything touches HIP.
struct RuntimeWarmup {
  std::thread t;
  void start(bool on) {      // (the switch: profiles/big_file_cli.py's A/B; a system that refuses the thread: the first HIP call stays where it was)
    if (!on || std::getenv("GBP_CLI_NO_WARMUP")) return;
    try { t = std::thread([] { (void)gbp_device_count(); }); } catch (...) {}
  }
  void wait() { if (t.joinable()) t.join(); }
  ~RuntimeWarmup() { wait(); }
};
inline RuntimeWarmup& runtime_warmup() { static RuntimeWarmup w; return w; }

// EMPIRICAL, measured and not explained (profiles/r06_exit_probe.txt, profiles/exit_probe.py): on this driver stack (ROCm 7.0 user space, the pool's
// amdgpu / KFD) a process whose address space has taken page faults from SIX OR MORE threads before the HIP runtime comes up is gone 40 - 60 ms sooner
// after its main() has ended — `ba fr1xyz --n_iters 200`: 0.15 - 0.19 s -> 0.105 - 0.12 s of process wall — than one whose memory was only ever touched by
// one to four threads.  What it takes: threads that TOUCH fresh memory (eight threads that allocate and free without touching, or thirty-two that do
// nothing: no effect; one thread touching 128 MB: no effect; malloc's arenas and thresholds, CPU affinity: no effect).  It showed first as the multi-threaded
// file reader making the 10^6-factor run exit faster than the 12 908-factor one.  Eight threads write 1 MB each: < 1 ms.  GBP_CLI_NO_PRIME=1 turns it off.
inline void prime_address_space() {
  if (std::getenv("GBP_CLI_NO_PRIME")) return;
  constexpr int kThreads = 8;
  constexpr size_t kBytes = (size_t)1 << 20;
  std::unique_ptr<char[]> buf(new (std::nothrow) char[kThreads * kBytes]);
  if (!buf) return;
  std::thread th[kThreads];
  try {      // (a system that refuses threads: the run goes on without them)
    const int pin = std::getenv("GBP_CLI_PRIME_PIN") ? sched_getcpu() : -1;      // (experiment: all eight on the caller's CPU — r06_exit_probe.txt)
    for (int i = 0; i < kThreads; ++i)
      th[i] = std::thread([p = buf.get() + (size_t)i * kBytes, i, pin] {
        if (pin >= 0) { cpu_set_t set; CPU_ZERO(&set); CPU_SET(pin, &set); (void)sched_setaffinity(0, sizeof(set), &set); }
        std::memset(p, i + 1, kBytes);
      });
  } catch (...) {
  }
  for (auto& t : th)
    if (t.joinable()) t.join();
  asm volatile("" ::"r"(buf.get()) : "memory");
}

inline int round_up_pow2(int n) {   // ba.cpp:617-621: nIPUs is rounded up to a power of two
  int p = 1;
  while (p < n) p *= 2;
  return p;
}

// Creates the ctx of this rank on its GPU, landmark-sharded for world > 1, with the communicator attached.
inline int create_rank_ctx(const Options& o, const Problem& P, RankCtx& rk, gbp_ctx** ctx) {
  phases().mark("host_setup_s");                                  // (flags, fork, the lines printed so far)
  runtime_warmup().wait();
  const int ndev = gbp_device_count();
  phases().mark("runtime_init_s");                                // the HIP runtime comes up with the first call that needs it — what of it the file's parsing did not hide
  if (ndev <= 0) {
    std::cout << "Could not find a device\n";                      // ba.cpp:652-655
    return 255;
  }
  const bool sharded = rk.region != nullptr;
  if (sharded) {
    if (gbp_set_device(rk.rank % ndev) != GBP_OK) { std::cout << "Could not find a device\n" << gbp_last_error(nullptr) << "\n"; return 255; }
    std::vector<uint32_t> bounds((size_t)rk.world + 1);
    gbp_landmark_partition(&P.prob, rk.world, bounds.data());
    rk.shard = gbp_shard{rk.rank, rk.world, bounds[rk.rank], bounds[rk.rank + 1]};
  } else {
    rk.shard = gbp_shard{0, 1, 0, P.bal.n_lmks};
  }
  if (gbp_create(&P.prob, nullptr, sharded ? &rk.shard : nullptr, ctx) != GBP_OK) {
    std::cout << "Could not find a device\n" << gbp_last_error(nullptr) << "\n";
    return 255;
  }
  if (sharded) {
    if (gbp_comm_init(*ctx, rk.region, o.transport) != GBP_OK) {
      std::cerr << "rank " << rk.rank << ": " << gbp_last_error(*ctx) << "\n";
      return 1;
    }
    std::cout << "Exchange between the " << rk.world << " ranks: " << gbp_comm_transport(*ctx)
              << (ndev < rk.world ? " (fewer GPUs than ranks: ranks share a GPU)" : "") << "\n";
    if (o.transport == (int)gbp::Transport::Measured)
      if (const char* info = gbp_last_error(*ctx))
        if (const char* m = std::strstr(info, "info: gbp_comm_init:")) std::cout << m + 6 << "\n";
    std::vector<char> desc(16384);
    if (gbp_comm_describe(*ctx, desc.data(), desc.size()) == GBP_OK) phases().comm_info = desc.data();
  }
  if (const char* info = gbp_last_error(*ctx)) phases().create_info = info;
  phases().mark("create_s");
  return 0;
}

// Runs body(rank) in `world` processes forked from this one — which must not have touched HIP yet — and supervises them:
// the exit status is the first failing rank's, and a rank that dies wakes the others out of their barriers.  result_count > 0 (--out_file):
// that many shared floats for the beliefs the ranks end with (result_floats, write_solution_ranks).
template <class F> int run_ranks(int world, uint32_t n_cams, bool force, size_t result_count, F&& body) {
  RankCtx rk;
  if (world <= 1 && !force) return body(rk);
  if (!std::getenv("HSA_ENABLE_IPC_MODE_LEGACY")) setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 1);   // dmabuf IPC for RCCL
  const size_t bytes = gbp_comm_region_bytes(n_cams, world);
  void* region = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
  if (region == MAP_FAILED || gbp_comm_region_init(region, bytes, n_cams, world) != GBP_OK) {
    std::cerr << "could not create the shared region of the ranks\n";
    return 1;
  }
  const size_t metric_bytes = gbp::metric_area_bytes(world);
  void* metric_area = mmap(nullptr, metric_bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
  if (metric_area == MAP_FAILED) {
    std::cerr << "could not create the shared metric records of the ranks\n";
    munmap(region, bytes);
    return 1;
  }
  const size_t result_bytes = result_count * sizeof(float);
  void* result = nullptr;
  if (result_bytes) {
    result = mmap(nullptr, result_bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    if (result == MAP_FAILED) {
      std::cerr << "could not create the shared result arrays of the ranks (--out_file: " << result_bytes << " bytes)\n";
      munmap(metric_area, metric_bytes);
      munmap(region, bytes);
      return 1;
    }
  }
  std::cout.flush();
  std::fflush(nullptr);
  std::vector<pid_t> pid((size_t)world, -1);
  bool fork_failed = false;
  for (int r = 0; r < world; ++r) {
    pid[r] = fork();
    if (pid[r] < 0) { std::cerr << "fork failed\n"; gbp_comm_region_abort(region); fork_failed = true; break; }
    if (pid[r] == 0) {
      rk.rank = r; rk.world = world; rk.region = region; rk.metric_area = metric_area; rk.result = static_cast<float*>(result);
      if (r != 0 && !std::freopen("/dev/null", "w", stdout)) std::_Exit(1);     // rank 0 prints (ba.cpp:996,1026-1028)
      int rc = 1;
      try { rc = body(rk); } catch (const std::exception& e) { std::cerr << "rank " << r << ": " << e.what() << "\n"; }
      std::cout.flush();
      std::fflush(nullptr);
      std::_Exit(rc);
    }
  }
  int status = 0, left = 0, first_bad = fork_failed ? 1 : 0;   // a run that could not start all its ranks never exits 0
  for (pid_t p : pid) left += p > 0;
  auto code_of = [](int st) { return WIFEXITED(st) ? WEXITSTATUS(st) : 128 + (WIFSIGNALED(st) ? WTERMSIG(st) : 0); };
  auto reap = [&](pid_t p, int st) {
    for (pid_t& q : pid) if (q == p) q = -1;
    --left;
    if (code_of(st) != 0 && first_bad == 0) {
      first_bad = code_of(st);
      gbp_comm_region_abort(region);            // the others leave their barriers with an error instead of waiting
    }
  };
  while (left > 0 && first_bad == 0) {
    const pid_t p = wait(&status);
    if (p < 0) {
      if (errno == EINTR) continue;            // a signal is not a failed rank
      break;
    }
    reap(p, status);
  }
  // a rank failed: the others normally notice at their next barrier; one that is stuck inside a collective whose peer
  // is gone never will, so after a grace period the remaining ranks are killed
  for (int waited_ms = 0; left > 0; waited_ms += 20) {
    const pid_t p = waitpid(-1, &status, WNOHANG);
    if (p > 0) { reap(p, status); continue; }
    if (p < 0) break;
    if (waited_ms >= 5000) {
      for (pid_t q : pid) if (q > 0) kill(q, SIGKILL);
      while (left > 0 && (wait(&status)) > 0) --left;
      break;
    }
    usleep(20000);
  }
  if (result) munmap(result, result_bytes);
  munmap(metric_area, metric_bytes);
  munmap(region, bytes);
  return first_bad;
}

// The reference's loop prints the metric after every iteration (ba.cpp:1009-1028).  To keep that output without making
// the GPU wait for the host every iteration, the metric of iteration i is queued (gbp_eval_begin) and printed only after
// iteration i+1 has been queued too; lines that belong after it ("Weakening priors") are deferred with it, so stdout is
// byte-identical to the unpipelined loop.  Off for --v, and for multi-rank runs: at the default --eval_every 1 those issue the same bursts
// as a single process and sum the records over the ranks (sum_burst_over_ranks); otherwise every metric is a gbp_eval_global.
struct MetricPipe {
  gbp_ctx* ctx = nullptr;
  bool on = false, pending = false;
  std::function<void(const gbp_eval_out&)> printer;
  std::string deferred;
  void line(const std::string& s) { if (pending) deferred += s; else std::cout << s; }
  int flush() {
    if (!pending) return GBP_OK;
    gbp_eval_out ev{};
    const int rc = gbp_eval_end(ctx, &ev);
    pending = false;
    if (rc != GBP_OK) return rc;
    printer(ev);
    std::cout << deferred;
    deferred.clear();
    return GBP_OK;
  }
  // metric of the current beliefs, printed by `p` — now (pipe off) or once the next submit / flush comes.
  // iterate_first > 0: that many GBP iterations are issued first, in the SAME call as the metric (gbp_iterate_eval: one
  // launch for both on graphs that run in the persistent kernel).
  int submit(std::function<void(const gbp_eval_out&)> p, int iterate_first = 0) {
    if (!on) {
      if (iterate_first > 0) { const int rc = gbp_iterate(ctx, iterate_first); if (rc != GBP_OK) return rc; }
      gbp_eval_out ev{};
      const int rc = gbp_eval_global(ctx, &ev);
      if (rc == GBP_OK) p(ev);
      return rc;
    }
    int rc = iterate_first > 0 ? gbp_iterate_eval(ctx, iterate_first) : gbp_eval_begin(ctx);   // the metric is queued behind the iterations
    if (rc != GBP_OK) return rc;
    if (pending) {                     // the previous metric: its kernels finished long ago
      gbp_eval_out ev{};
      rc = gbp_eval_end(ctx, &ev);
      if (rc != GBP_OK) return rc;
      printer(ev);
      std::cout << deferred;
      deferred.clear();
    }
    printer = std::move(p);
    pending = true;
    return GBP_OK;
  }
};

// The metric lines of the reference's default loop (one per iteration: 1 500 - 13 299 of them) are formatted and written by ONE
// writer thread, in order, while the main thread has already issued the next burst: iostream formatting costs ~1.3 us a line,
// time the GPU would otherwise sit idle between two launches (ba fr1xyz: 2 ms of a 22 ms loop).  Everything else the loop prints
// (rare: "Weakening priors", keyframe banners, --v dumps) first waits for the writer (drain), so stdout stays byte-identical.
struct AsyncLines {
  std::mutex mu;
  std::condition_variable cv, idle;
  std::deque<std::function<void()>> q;
  bool done = false, busy = false;
  std::thread th;
  AsyncLines() : th([this] { run(); }) {}
  ~AsyncLines() { finish(); }
  void post(std::function<void()> f) {
    { std::lock_guard<std::mutex> lk(mu); q.push_back(std::move(f)); }
    cv.notify_one();
  }
  void drain() {
    std::unique_lock<std::mutex> lk(mu);
    idle.wait(lk, [&] { return q.empty() && !busy; });
  }
  void finish() {
    if (!th.joinable()) return;
    { std::lock_guard<std::mutex> lk(mu); done = true; }
    cv.notify_one();
    th.join();
  }
  void run() {
    for (;;) {
      std::function<void()> f;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return done || !q.empty(); });
        if (q.empty()) return;
        f = std::move(q.front());
        q.pop_front();
        busy = true;
      }
      f();
      { std::lock_guard<std::mutex> lk(mu); busy = false; }
      idle.notify_all();
    }
  }
};

// A multi-rank run's burst (gbp_ba_loop with a host `out`: the LOCAL shard's sums of n <= gbp::kMetricBurstMax passes) -> the sums over all
// ranks, in place: this rank's row of the burst's parity, ONE barrier, the rows added in rank order (gbp_metric_gather.hpp: what
// gbp_eval_global returns, pass for pass).  A single-process run: nothing to do.
inline int sum_burst_over_ranks(gbp_ctx* ctx, RankCtx& rk, gbp_eval_out* series, int n) {
  if (!rk.region) return GBP_OK;
  const int parity = (int)(rk.bursts++ & 1u);
  std::memcpy(gbp::metric_row(rk.metric_area, rk.world, parity, rk.rank), series, sizeof(gbp_eval_out) * (size_t)n);
  if (const int rc = gbp_comm_barrier(ctx)) return rc;
  gbp::metric_sum_ranks(gbp::metric_row(rk.metric_area, rk.world, parity, 0), rk.world, n, series);
  return GBP_OK;
}

#define CLI_CHECK(ctx, call)                                                              \
  do {                                                                                    \
    const int rc_ = (call);                                                               \
    if (rc_ != GBP_OK) {                                                                  \
      std::cerr << #call << " failed (" << rc_ << "): " << gbp_last_error(ctx) << "\n";  \
      return 1;                                                                           \
    }                                                                                     \
  } while (0)

// a call that returned GBP_OK can leave a `warning: ...` in gbp_last_error (a recovered time-out of the persistent kernel)
inline void print_warning(gbp_ctx* ctx) {
  const char* w = gbp_last_error(ctx);
  if (w && std::strncmp(w, "warning:", 8) == 0) std::cerr << w << "\n";
}

// --profile (ba.cpp:410-413,1060-1082 dump Poplar's execution / graph profile): here a one-line JSON report with the times of
// the run, which iteration path the library chose and the LAST printed metric at full precision (stdout carries six digits).
// bench.py reads it for the fr1xyz / fr2robot2 halves of BASELINE.json's metric.
struct RunReport {
  double wall_s = 0, setup_s = 0, loop_s = 0;
  long iters = 0;
  bool have_metric = false;
  gbp_eval_out last{};
};

// (called after the ctx is gone — its teardown is one of the phases — with what was read from it before)
inline void write_profile(const gbp_timing_out& t, int graph_state, const char* tool, const RunReport& r) {
  const char* dir = std::getenv("GC_PROFILE_LOG_DIR");
  const std::string path = std::string(dir ? dir : ".") + "/gbp_profile.json";
  if (FILE* f = std::fopen(path.c_str(), "w")) {
    std::fprintf(f, "{\"tool\": \"%s\", \"iterations\": %ld, \"wall_s\": %.6f, \"setup_s\": %.6f, \"loop_s\": %.6f, \"device_ms\": %.3f, "
                    "\"device_iterations\": %llu, \"iters_per_s_device\": %.3f, \"graph_state\": %d, "
                    "\"algorithmic_bytes_per_iter\": %llu, \"device_bytes_allocated\": %llu",
                 tool, r.iters, r.wall_s, r.setup_s, r.loop_s, t.total_ms, (unsigned long long)t.iterations,
                 t.total_ms > 0 ? 1e3 * (double)t.iterations / t.total_ms : 0.0, graph_state,
                 (unsigned long long)t.algorithmic_bytes_per_iter, (unsigned long long)t.device_bytes_allocated);
    if (r.have_metric && r.last.n_active) {
      const double n = (double)r.last.n_active;
      std::fprintf(f, ", \"final_mean_reproj_px\": %.9g, \"final_cost\": %.9g, \"final_rmse_px\": %.9g, \"n_active\": %llu, "
                      "\"n_relin\": %llu, \"n_robust\": %llu, \"n_nonfinite\": %llu",
                   r.last.sum_norm / n, r.last.sum_half_sq, std::sqrt(2.0 * r.last.sum_half_sq / n), (unsigned long long)r.last.n_active,
                   (unsigned long long)r.last.n_relin, (unsigned long long)r.last.n_robust, (unsigned long long)r.last.n_nonfinite);
    }
    {  // where the wall time of the PROCESS went
      const Phases& ph = phases();
      std::fprintf(f, ", \"startup\": {\"process_s\": %.6f, \"exec_to_main_s\": %.3f", ph.since_exec(), ph.exec_to_main_s);
      for (const auto& p : ph.v) std::fprintf(f, ", \"%s\": %.6f", p.first.c_str(), p.second);
      std::string info = ph.create_info;
      for (char& ch : info) if (ch == '"' || ch == '\\') ch = '\'';
      std::fprintf(f, ", \"create\": \"%s\"}", info.c_str());
      if (!ph.comm_info.empty()) std::fprintf(f, ", \"comm\": %s", ph.comm_info.c_str());
    }
    std::fprintf(f, "}\n");
    std::fclose(f);
    std::cout << "Profile written to " << path << "\n";
  }
}

// The end of a run, shared by ./ba and ./slam: the ctx is destroyed FIRST (its teardown is part of what the user waits for), then the
// "Total time" line — which covers the process from exec to here — and the --profile report.
inline int finish_run(const Options& o, const Problem& P, gbp_ctx* ctx, const RankCtx& rk, const char* tool, RunReport& rep, long iters) {
  if (rk.region) {      // the communicator's record as the run leaves it: its "metric" member says which path the loop's bursts took
    std::vector<char> desc(16384);
    if (gbp_comm_describe(ctx, desc.data(), desc.size()) == GBP_OK) phases().comm_info = desc.data();
  }
  gbp_timing_out tm{};
  gbp_timing(ctx, &tm, 0);
  const int gs = gbp_graph_state(ctx);
  print_warning(ctx);
  const int wrc = write_solution(o, P, ctx, rk);
  if (wrc == kLeaveNow) return 1;      // like a failed call of the loop: the process ends, the supervisor wakes the other ranks
  phases().mark("loop_s");
  gbp_destroy(ctx);
  phases().mark("teardown_s");
  const Phases& ph = phases();
  rep.loop_s = ph.get("loop_s");
  rep.setup_s = ph.get("upload_s") + ph.get("linearise_s");
  rep.wall_s = rep.setup_s + rep.loop_s;
  rep.iters = iters;
  std::cout << "Total time: " << ph.since_exec() << " s from exec (loader " << ph.exec_to_main_s << " s, file + priors " << ph.get("file_parse_s")
            << " s, runtime " << ph.get("runtime_init_s") << " s, gbp_create " << ph.get("create_s") << " s, upload " << ph.get("upload_s")
            << " s, linearise + first metric " << ph.get("linearise_s") << " s, iteration loop " << rep.loop_s << " s, teardown " << ph.get("teardown_s")
            << " s); device time in GBP iterations: " << tm.total_ms << " ms over " << tm.iterations
            << " iterations (" << (tm.total_ms > 0 ? 1e3 * (double)tm.iterations / tm.total_ms : 0.0) << " iters/s)\n";
  if (o.profile) write_profile(tm, gs, tool, rep);
  return wrc;
}

// --steps as gbp_ba_loop takes it: a whole, non-negative number below 2^30 (the loop's test is `iter < 2 * steps`: the product must not
// wrap, and a float beyond UINT_MAX must not be cast at all) — anything else keeps the loop's own float test, call by call
inline bool whole_steps(float steps) { return steps >= 0.f && steps < 1073741824.f && steps == (float)(unsigned)steps; }

// The last step of main(): everything is written, the ctx is destroyed.  Normally the process then leaves WITHOUT running exit handlers
// (std::_Exit) — the HIP runtime's take 15 - 30 ms in which the user's prompt does not come back, and the driver reclaims the process's
// resources either way.  Under an injected library (LD_PRELOAD: rocprofv3, sanitizers — their reports are written by exit handlers) or
// with GBP_CLI_FULL_EXIT set, the ordinary return.
inline int leave(int rc) {
  if (std::getenv("GBP_HOST_TRACE")) {      // what the kernel will have to tear down: the address space as it stands (profiles/r06_exit_probe.txt)
    size_t vmas = 0;
    if (FILE* f = std::fopen("/proc/self/maps", "r")) { int ch; while ((ch = std::fgetc(f)) != EOF) vmas += ch == '\n'; std::fclose(f); }
    std::fprintf(stderr, "leave: %zu mappings;", vmas);
    for (const char* path : {"/proc/self/status", "/proc/self/smaps_rollup"})
      if (FILE* f = std::fopen(path, "r")) {
        char line[256];
        while (std::fgets(line, sizeof(line), f))
          for (const char* key : {"VmRSS:", "VmPTE:", "RssAnon:", "RssFile:", "RssShmem:", "Threads:", "AnonHugePages:", "ShmemPmdMapped:", "FilePmdMapped:", "Locked:", "VmLck:", "VmPin:"})
            if (!std::strncmp(line, key, std::strlen(key))) { line[std::strcspn(line, "\n")] = 0; std::fprintf(stderr, " %s", line); }
        std::fclose(f);
      }
    std::fprintf(stderr, "\n");
  }
  std::cout.flush();
  std::cerr.flush();
  std::fflush(nullptr);
  if (std::getenv("LD_PRELOAD") || std::getenv("GBP_CLI_FULL_EXIT") || std::getenv("ROCP_TOOL_LIBRARIES")) return rc;
  std::_Exit(rc);
}

}  // namespace cli
