// The host index of the ctx-less libraries (gbp_poplar_amd/stateless/stateless_index.hpp: the body of gbp_seed_index, gbp_resect_index
// and their checks) compiled for the HOST, on its own.  Built by tests/test_stateless_cpu.py under ASan + UBSan and run as a process;
// never loaded into python.  Every array has exactly the size the header documents, so a step past its end is the sanitizer's.
//
//   stateless_index_main            -> "stateless_index: ok" and status 0, or one line per mismatch and status 1
#include "../../include/gbp_mi355x_seed.h"
#include "../../gbp_poplar_amd/stateless/stateless_index.hpp"

#include <cstdio>
#include <string>
#include <vector>

using namespace gbp::stateless;
using U32 = std::vector<uint32_t>;

static int g_failures = 0;
static void expect(bool ok, const std::string& what) {
  if (ok) return;
  std::printf("MISMATCH %s (text: \"%s\")\n", what.c_str(), last_error().c_str());
  ++g_failures;
}
static uint32_t* data(U32& v) { return v.empty() ? nullptr : v.data(); }
static const uint32_t* data(const U32& v) { return v.empty() ? nullptr : v.data(); }

// a success: the index is the stable sort of the edges by id, written plainly, and a stale text is cleared
static void builds(const char* what, const IndexNames& nm, uint32_t n, const U32& id) {
  U32 start(n + 1, 0xdeadbeefu), edges(id.size(), 0xdeadbeefu), want_start(n + 1, 0u), want_edges;
  for (uint32_t i = 0; i < n; ++i) {
    for (uint32_t e = 0; e < id.size(); ++e)
      if (id[e] == i) want_edges.push_back(e);
    want_start[i + 1] = (uint32_t)want_edges.size();
  }
  fail(GBP_ERR_INVALID, "stale");
  const int rc = build_index("fn", nm, n, (uint32_t)id.size(), data(id), start.data(), data(edges));
  expect(rc == GBP_OK && last_error().empty(), std::string(what) + ": build_index succeeds and clears the text");
  expect(start == want_start && edges == want_edges, std::string(what) + ": the index is the stable sort");
  fail(GBP_ERR_INVALID, "stale");
  expect(check_index("fn", nm, n, (uint32_t)id.size(), start.data(), data(edges), false) == GBP_OK && last_error().empty(),
         std::string(what) + ": its own check accepts it and clears the text");
  expect(check_index("fn", nm, n, (uint32_t)id.size(), start.data(), nullptr, true) == GBP_OK, std::string(what) + ": ... and without edges");
}

static void refused(const char* what, int rc, const char* text) {
  expect(rc == GBP_ERR_INVALID && last_error() == text, std::string(what) + ": expected \"" + text + "\"");
}

int main() {
  // ---- the index ----
  builds("no edge, NULL ids and edges", kLmkIndex, 3, {});
  builds("no item", kCamIndex, 0, {});
  builds("one item", kLmkIndex, 1, {0, 0, 0});
  builds("an unobserved item", kCamIndex, 4, {3, 0, 3, 1});
  builds("duplicates", kLmkIndex, 3, {2, 1, 2, 2, 0, 1, 1, 0});
  {
    U32 start(8), edges(4);
    const U32 id = {0, 6, 7, 1};
    refused("an id equal to n", build_index("gbp_resect_index", kCamIndex, 7, 4, id.data(), start.data(), edges.data()),
            "gbp_resect_index: cam_id[2] = 7 is not below n_cams");
    refused("an id with no item", build_index("gbp_seed_index", kLmkIndex, 0, 4, id.data(), start.data(), edges.data()),
            "gbp_seed_index: lmk_id[0] = 0 is not below n_lmks");
    refused("start NULL", build_index("gbp_seed_index", kLmkIndex, 7, 4, id.data(), nullptr, edges.data()), "gbp_seed_index: lmk_start is NULL");
    refused("ids NULL", build_index("gbp_seed_index", kLmkIndex, 7, 4, nullptr, start.data(), edges.data()), "gbp_seed_index: lmk_id is NULL");
    refused("edges NULL", build_index("gbp_resect_index", kCamIndex, 7, 4, id.data(), start.data(), nullptr), "gbp_resect_index: cam_edges is NULL");
  }
  // ---- the check: 3 items, 4 edges ----
  const U32 good = {0, 2, 3, 4}, identity = {0, 1, 2, 3};
  const char *sfn = "gbp_seed_check_index", *rfn = "gbp_resect_check_index";
  refused("start[0] != 0", check_index(sfn, kLmkIndex, 3, 4, U32{1, 2, 3, 4}.data(), identity.data(), false), "gbp_seed_check_index: lmk_start[0] is not 0");
  refused("a descent", check_index(rfn, kCamIndex, 3, 4, U32{0, 3, 2, 4}.data(), identity.data(), true),
          "gbp_resect_check_index: cam_start is not ascending at 2");
  refused("start[n] != n_edges", check_index(sfn, kLmkIndex, 3, 4, U32{0, 2, 3, 3}.data(), identity.data(), false),
          "gbp_seed_check_index: lmk_start[n_lmks] = 3 is not n_edges = 4");
  refused("start[n] != n_edges (cam)", check_index(rfn, kCamIndex, 3, 4, U32{0, 2, 3, 5}.data(), identity.data(), true),
          "gbp_resect_check_index: cam_start[n_cams] = 5 is not n_edges = 4");
  refused("an edge entry equal to n_edges", check_index(sfn, kLmkIndex, 3, 4, good.data(), U32{0, 1, 2, 4}.data(), false),
          "gbp_seed_check_index: lmk_edges[3] is not below n_edges");
  refused("an edge entry equal to n_edges (cam)", check_index(rfn, kCamIndex, 3, 4, good.data(), U32{4, 1, 2, 3}.data(), true),
          "gbp_resect_check_index: cam_edges[0] is not below n_edges");
  fail(GBP_ERR_INVALID, "stale");
  expect(check_index(rfn, kCamIndex, 3, 4, good.data(), nullptr, true) == GBP_OK && last_error().empty(), "NULL edges with the flag on: the identity index");
  refused("NULL edges with the flag on, a descent", check_index(rfn, kCamIndex, 3, 4, U32{0, 3, 2, 4}.data(), nullptr, true),
          "gbp_resect_check_index: cam_start is not ascending at 2");
  refused("NULL edges with the flag off", check_index(sfn, kLmkIndex, 3, 4, good.data(), nullptr, false), "gbp_seed_check_index: lmk_edges is NULL");
  expect(check_index(sfn, kLmkIndex, 3, 0, U32{0, 0, 0, 0}.data(), nullptr, false) == GBP_OK && last_error().empty(),
         "NULL edges with the flag off and no edge");
  refused("start NULL", check_index(rfn, kCamIndex, 3, 4, nullptr, identity.data(), true), "gbp_resect_check_index: cam_start is NULL");
  if (g_failures) return 1;
  std::printf("stateless_index: ok\n");
  return 0;
}
