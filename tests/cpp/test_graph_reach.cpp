// C++ checks of LeannIndex::reachability / cover_entry_seeds and HnswGraph::reachability (include/islands_amd.hpp over
// isl_index_reachability, isl_hnsw_reachability and isl_index_cover_entry_seeds).  `test_graph_reach cpu`: what is
// answered without a device; `test_graph_reach gpu` adds hand graphs whose answers follow from the definitions.
#include <cstdio>
#include <cstring>
#include <random>

#include "islands_amd.hpp"

using namespace islands::core;

static int failures = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)

template <class F>
static bool throws(isl_status st, F f, uint64_t node = 0) {
  try { f(); } catch (const CoreError& e) {
    return e.status == st && (st != ISL_ERR_NODE_NOT_FOUND || e.node == node);
  }
  return false;
}

// a ring of n nodes entered at `entry`: node i lists (i + 1) % n
static CsrGraph ring(uint64_t n, uint64_t entry) {
  CsrGraph g;
  g.num_nodes = n;
  g.node_offsets.assign(1, 0);
  for (uint64_t i = 0; i < n; ++i) {
    g.neighbors.push_back((i + 1) % n);
    g.node_offsets.push_back(g.neighbors.size());
  }
  g.levels.assign(n, 0);
  g.degree_counts.assign(n, 1);
  g.entry_point = entry;
  return g;
}

int main(int argc, char** argv) {
  const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
  static_assert(sizeof(isl_reach_report) == 64, "eight uint64_t");
  LeannConfig cfg;
  cfg.m = 4; cfg.m0 = 8; cfg.ef_construction = 40;
  {
    isl_reach_report rep;
    uint64_t src = 0, n = 7, un = 7;
    EXPECT(isl_index_reachability(nullptr, nullptr, 0, nullptr, nullptr, ISL_MEM_HOST, &rep) == ISL_ERR_INVALID_ARGUMENT);
    EXPECT(isl_hnsw_reachability(nullptr, 0, nullptr, 0, nullptr, nullptr, ISL_MEM_HOST, &rep) == ISL_ERR_INVALID_ARGUMENT);
    EXPECT(isl_index_cover_entry_seeds(nullptr, 4, nullptr, &n, &un) == ISL_ERR_INVALID_ARGUMENT && n == 0 && un == 0);
    LeannIndex empty;
    EXPECT(throws(ISL_ERR_EMPTY_COLLECTION, [&] { empty.reachability(); }));
    EXPECT(throws(ISL_ERR_EMPTY_COLLECTION, [&] { empty.cover_entry_seeds(4); }));
    EXPECT(throws(ISL_ERR_UNSUPPORTED, [&] { empty.cover_entry_seeds(ISL_MAX_ENTRY_SEEDS + 1); }));
    LeannIndex host = LeannIndex::from_csr(ring(5, 2), cfg, 4);  // never uploaded
    const std::vector<uint8_t> before = host.to_bytes();
    EXPECT(isl_index_reachability(host.handle(), &src, 1, nullptr, nullptr, 9, &rep) == ISL_ERR_INVALID_ARGUMENT);
    EXPECT(isl_index_reachability(host.handle(), nullptr, 1, nullptr, nullptr, ISL_MEM_HOST, &rep) == ISL_ERR_INVALID_ARGUMENT);
    EXPECT(throws(ISL_ERR_NODE_NOT_FOUND, [&] { host.reachability({1, 5}); }, 5));
    EXPECT(throws(ISL_ERR_UNSUPPORTED, [&] { host.reachability(); }));
    EXPECT(throws(ISL_ERR_UNSUPPORTED, [&] { host.cover_entry_seeds(); }));
    EXPECT(host.to_bytes() == before && host.entry_seeds().empty());
  }
  if (gpu) {
    // a ring of 70 entered at node 5: 70 levels, every frontier one node
    LeannIndex idx = LeannIndex::from_csr(ring(70, 5), cfg, 4);
    idx.upload(0);
    Reachability r = idx.reachability({}, true, true);
    EXPECT(r.report.nodes == 70 && r.report.sources == 1 && r.report.reached == 70 && r.report.levels == 70);
    EXPECT(r.report.edges == 70 && r.report.dangling_edges == 0 && r.report.no_inbound == 0 && r.report.max_in_degree == 1);
    bool ok = r.depth.size() == 70 && r.in_degree.size() == 70;
    for (uint64_t i = 0; ok && i < 70; ++i) ok = r.depth[i] == (i + 70 - 5) % 70 && r.in_degree[i] == 1;
    EXPECT(ok);
    r = idx.reachability({7, 7, 40});
    EXPECT(r.report.sources == 2 && r.report.reached == 70 && r.report.levels == 37 && r.depth.empty());
    EXPECT(throws(ISL_ERR_NODE_NOT_FOUND, [&] { idx.reachability({70}); }, 70));
    // two rings of 4 and 3, no edge between them, with rows: the cover adds the first node of the second ring
    CsrGraph g = ring(4, 0);
    g.num_nodes = 7;
    for (uint64_t i = 0; i < 3; ++i) {
      g.neighbors.push_back(4 + (i + 1) % 3);
      g.node_offsets.push_back(g.neighbors.size());
    }
    g.levels.assign(7, 0);
    g.degree_counts.assign(7, 1);
    LeannIndex two = LeannIndex::from_csr(g, cfg, 4);
    two.upload(0);
    std::mt19937 rng(3);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    std::vector<float> v(7 * 4);
    for (auto& x : v) x = u(rng);
    two.attach(InMemoryEmbeddingProvider(v, 4));
    EXPECT(two.reachability().report.reached == 4);
    CoveredSeeds c = two.cover_entry_seeds(1);  // S = [0] already holds one seed
    EXPECT(c.ids.empty() && c.unreached == 3 && two.entry_seeds().empty());
    c = two.cover_entry_seeds();
    EXPECT(c.ids == std::vector<uint64_t>({0, 4}) && c.unreached == 0 && two.entry_seeds() == c.ids);
    EXPECT(two.reachability().report.reached == 7 && two.reachability().report.sources == 2);
    c = two.cover_entry_seeds();  // nothing left to add
    EXPECT(c.ids == std::vector<uint64_t>({0, 4}) && c.unreached == 0);
    // an HnswGraph: every layer's population is the nodes at or above it
    const uint64_t n = 400, d = 8;
    std::vector<float> rows(n * d);
    for (auto& x : rows) x = u(rng);
    isl_hnsw_config hc;
    isl_hnsw_config_default(&hc);
    hc.m = 4; hc.m0 = 8; hc.ef_construction = 40;
    HnswGraph h = HnswGraph::build(rows, d, &hc, {}, 11);
    uint64_t pop0 = h.reachability(0).report.nodes;
    EXPECT(pop0 == n);
    const Reachability top = h.reachability(1, {}, true, true);
    uint64_t absent = 0;
    for (uint32_t x : top.depth) absent += x == ISL_DEPTH_ABSENT;
    EXPECT(top.report.nodes + absent == n && top.report.nodes < n && top.report.reached <= top.report.nodes);
    EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { h.reachability(40); }));
  }
  std::printf("%s: %d failure(s)\n", gpu ? "gpu" : "cpu", failures);
  return failures ? 1 : 0;
}
