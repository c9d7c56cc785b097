// C++ checks of HnswGraph::remove (include/islands_amd.hpp over isl_hnsw_remove).
// `test_hnsw_remove cpu`: what needs no device; `test_hnsw_remove gpu` adds removals on the device where the
// definition says what is left without measuring anything: nodes that no list names leave every other list as it
// was (through the remap), and a graph emptied and filled again is the graph a second build makes.
#include <cstdio>
#include <cstring>
#include <random>
#include <set>

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

int main(int argc, char** argv) {
  const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
  isl_hnsw_config cfg;
  isl_hnsw_config_default(&cfg);
  cfg.m = 8; cfg.m0 = 16; cfg.ef_construction = 64;
  {
    HnswGraph g = HnswGraph::build({}, 0, &cfg);
    const std::vector<uint8_t> b = g.to_bytes();
    EXPECT(g.remove({}).empty() && g.is_empty() && g.to_bytes() == b);  // no ids: nothing changes
    EXPECT(throws(ISL_ERR_NODE_NOT_FOUND, [&] { g.remove({4, 0}); }, 4));
    isl_build_options o = LeannIndex::build_options();
    o.select_rule = 7;
    EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { g.remove({0}, o); }));
    o.select_rule = ISL_SELECT_DIVERSE;
    o.alpha = 0.5f;
    EXPECT(throws(ISL_ERR_INVALID_CONFIG, [&] { g.remove({}, o); }));  // the options before "no ids"
    EXPECT(isl_hnsw_remove(nullptr, nullptr, nullptr, 0, nullptr, nullptr) == ISL_ERR_INVALID_ARGUMENT);
    EXPECT(g.is_empty() && g.to_bytes() == b);
  }
  if (gpu) {
    const uint64_t n = 300, d = 16;
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    std::vector<float> v(n * d);
    for (auto& x : v) x = u(rng);
    std::vector<uint64_t> lv(n);
    EXPECT(isl_hnsw_random_levels(3, n, cfg.ml, cfg.max_layers, lv.data()) == ISL_OK);
    for (uint32_t rule : {ISL_SELECT_REFERENCE, ISL_SELECT_DIVERSE}) {
      isl_build_options o = LeannIndex::build_options();
      o.select_rule = rule;
      HnswGraph g = HnswGraph::build(v, d, &cfg, lv, 0, &o);
      const std::vector<uint8_t> before = g.to_bytes();
      EXPECT(throws(ISL_ERR_NODE_NOT_FOUND, [&] { g.remove({5, n}, o); }, n));
      EXPECT(g.len() == n && g.to_bytes() == before);
      // every list of the graph, and the level-0 nodes that none of them names
      std::vector<std::vector<std::vector<uint64_t>>> lists(n);
      std::vector<bool> named(n, false);
      for (uint64_t i = 0; i < n; ++i)
        for (uint64_t L = 0; L <= lv[i]; ++L) {
          lists[i].push_back(g.neighbors(i, L));
          for (uint64_t x : lists[i].back()) named[x] = true;
        }
      std::set<uint64_t> gone;
      for (uint64_t i = n; i-- > 0 && gone.size() < 40;)
        if (!named[i] && lv[i] == 0) gone.insert(i);
      if (rule == ISL_SELECT_REFERENCE) EXPECT(gone.size() == 40);  // past m0 nodes no later node gets an inbound edge
      if (gone.empty()) gone.insert(n - 1);  // (the diverse rule leaves few such nodes: then any node will do)
      const bool unnamed = !named[*gone.begin()];
      const std::vector<uint64_t> remap = g.remove(std::vector<uint64_t>(gone.begin(), gone.end()), o);
      EXPECT(remap.size() == n && g.len() == n - gone.size());
      uint64_t next = 0;
      for (uint64_t i = 0; i < n; ++i) {
        if (gone.count(i)) { EXPECT(remap[i] == ISL_REMOVED); continue; }
        EXPECT(remap[i] == next++);
        for (uint64_t L = 0; L <= lv[i]; ++L) {
          const std::vector<uint64_t> now = g.neighbors(remap[i], L);
          if (unnamed) {  // no list lost a neighbour: each is the old one through the remap
            std::vector<uint64_t> want;
            for (uint64_t x : lists[i][L]) want.push_back(remap[x]);
            EXPECT(now == want);
          }
          for (uint64_t x : now) EXPECT(x < g.len() && x != remap[i]);
          EXPECT(now.size() <= (L ? cfg.m : cfg.m0));
        }
      }
      const auto row = g.get_vector(remap[8]);
      EXPECT(row && std::memcmp(row->data(), v.data() + 8 * d, d * 4) == 0);
      const auto r = g.search(std::vector<float>(v.begin() + 8 * d, v.begin() + 9 * d), 1, 64);
      EXPECT(r.size() == 1 && r[0].first == remap[8]);
      // emptied and filled again: the graph a second build makes
      std::vector<uint64_t> all(g.len());
      for (uint64_t i = 0; i < all.size(); ++i) all[i] = i;
      const std::vector<uint64_t> none = g.remove(all, o);
      EXPECT(g.is_empty() && none.size() == all.size() && none[0] == ISL_REMOVED);
      EXPECT(g.insert(v, d, lv, 0, &o) == 0 && g.len() == n);
      EXPECT(g.to_bytes() == before);
      EXPECT(g.to_bytes() == HnswGraph::build(v, d, &cfg, lv, 0, &o).to_bytes());
    }
  }
  std::printf("%s: %d failure(s)\n", gpu ? "gpu" : "cpu", failures);
  return failures ? 1 : 0;
}
