// stateless/stateless_index.hpp — the HOST index of a graph by one of its two kinds of vertex (gbp_seed_index: by landmark,
// gbp_resect_index: by camera) and its check, written once.  The exports stay in their library's .hip and name their arrays in the
// failure texts through IndexNames.  Include it behind the library's public header, as stateless_export.hpp.
#pragma once
#include "stateless_export.hpp"

#include <vector>

namespace gbp {
namespace stateless {

struct IndexNames {      // what the failure texts call the ids, their bound, and the two arrays of the index
  const char *id, *n, *start, *edges;
};
constexpr IndexNames kLmkIndex{"lmk_id", "n_lmks", "lmk_start", "lmk_edges"}, kCamIndex{"cam_id", "n_cams", "cam_start", "cam_edges"};

// the edges of item i are edges[start[i] .. start[i + 1]), in file order
inline int build_index(const char* fn, const IndexNames& nm, uint32_t n, uint32_t n_edges, const uint32_t* id, uint32_t* start, uint32_t* edges) {
  if (!start) return null_arg(fn, nm.start);
  if (n_edges && !id) return null_arg(fn, nm.id);
  if (n_edges && !edges) return null_arg(fn, nm.edges);
  for (uint32_t e = 0; e < n_edges; ++e)
    if (id[e] >= n) return bad_arg(fn, std::string(nm.id) + "[" + std::to_string(e) + "] = " + std::to_string(id[e]) + " is not below " + nm.n);
  // counting sort: the degrees, their running sum, then every edge to the next free place of its item (ascending e: stable)
  for (uint64_t i = 0; i <= n; ++i) start[i] = 0u;
  for (uint32_t e = 0; e < n_edges; ++e) ++start[id[e] + 1];
  for (uint64_t i = 0; i < n; ++i) start[i + 1] += start[i];
  std::vector<uint32_t> next(start, start + n);
  for (uint32_t e = 0; e < n_edges; ++e) edges[next[id[e]]++] = e;
  last_error().clear();
  return GBP_OK;
}

// edges_may_be_null: NULL edges are the identity index (entry k is edge k), and only start is checked
inline int check_index(const char* fn, const IndexNames& nm, uint32_t n, uint32_t n_edges, const uint32_t* start, const uint32_t* edges,
                       bool edges_may_be_null) {
  if (!start) return null_arg(fn, nm.start);
  if (!edges_may_be_null && n_edges && !edges) return null_arg(fn, nm.edges);
  if (start[0] != 0u) return bad_arg(fn, std::string(nm.start) + "[0] is not 0");
  for (uint64_t i = 0; i < n; ++i)
    if (start[i + 1] < start[i]) return bad_arg(fn, std::string(nm.start) + " is not ascending at " + std::to_string(i + 1));
  if (start[n] != n_edges)
    return bad_arg(fn, std::string(nm.start) + "[" + nm.n + "] = " + std::to_string(start[n]) + " is not n_edges = " + std::to_string(n_edges));
  if (edges)
    for (uint32_t k = 0; k < n_edges; ++k)
      if (edges[k] >= n_edges) return bad_arg(fn, std::string(nm.edges) + "[" + std::to_string(k) + "] is not below n_edges");
  last_error().clear();
  return GBP_OK;
}

}  // namespace stateless
}  // namespace gbp
