// C++ checks of HnswGraph::build / to_bytes / neighbors (include/islands_amd.hpp over isl_hnsw_build).
// `test_hnsw_build cpu`: what needs no device; `test_hnsw_build gpu` adds a small build on the device.
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
static bool throws(isl_status st, F f) {
  try { f(); } catch (const CoreError& e) { return e.status == st; }
  return false;
}

int main(int argc, char** argv) {
  const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
  isl_hnsw_config cfg;
  isl_hnsw_config_default(&cfg);
  EXPECT(cfg.m == 16 && cfg.m0 == 32 && cfg.ef_construction == 200 && cfg.max_layers == 16 && cfg.metric == 0);
  {
    HnswGraph g = HnswGraph::build({}, 0, &cfg);  // no rows: an empty graph, no device
    EXPECT(g.is_empty());
    const std::vector<uint8_t> b = g.to_bytes();
    EXPECT(b.size() == 8 * 3 + 8 + 4 + 8 + 8 + 1 + 8 + 1 + 8);  // config, 0 nodes, None, 0, None, next_id 0
    HnswGraph back = HnswGraph::from_bytes(b);
    EXPECT(back.to_bytes() == b);
    EXPECT(throws(ISL_ERR_NODE_NOT_FOUND, [&] { g.neighbors(0, 0); }));
  }
  isl_hnsw_config bad = cfg;
  bad.m0 = 8;
  EXPECT(throws(ISL_ERR_INVALID_CONFIG, [&] { HnswGraph::build(std::vector<float>(32, 1.f), 4, &bad); }));
  EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { HnswGraph::build(std::vector<float>(8, 1.f), 4, &cfg, {0, 16}); }));
  if (gpu) {
    const uint64_t n = 300, d = 16;
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    std::vector<float> v(n * d);
    for (auto& x : v) x = u(rng);
    cfg.m = 8; cfg.m0 = 16; cfg.ef_construction = 64;
    isl_build_options o;
    isl_build_options_default(&o);
    o.select_rule = ISL_SELECT_DIVERSE;
    HnswGraph g = HnswGraph::build(v, d, &cfg, {}, 3, &o);
    EXPECT(g.len() == n);
    std::vector<uint64_t> lv(n);
    check(isl_hnsw_random_levels(3, n, cfg.ml, cfg.max_layers, lv.data()));
    std::vector<bool> named(n, false);
    for (uint64_t i = 0; i < n; i++) {
      const auto row = g.neighbors(i, 0);
      EXPECT(row.size() <= cfg.m0);
      for (uint64_t x : row) { EXPECT(x < n && x != i); named[x] = true; }
      EXPECT(g.neighbors(i, lv[i] + 1).empty());
    }
    uint64_t lost = 0;
    for (uint64_t i = 0; i < n; i++) lost += !named[i];
    EXPECT(lost == 0);
    const auto r = g.search(std::vector<float>(v.begin() + 7 * d, v.begin() + 8 * d), 1, 64);
    EXPECT(r.size() == 1 && r[0].first == 7);
    const auto row7 = g.get_vector(7);
    EXPECT(row7 && std::memcmp(row7->data(), v.data() + 7 * d, d * 4) == 0);
    HnswGraph back = HnswGraph::from_bytes(g.to_bytes());
    EXPECT(back.to_bytes() == g.to_bytes());
    EXPECT(back.neighbors(7, 0) == g.neighbors(7, 0));
  }
  std::printf("%s: %d failure(s)\n", gpu ? "gpu" : "cpu", failures);
  return failures ? 1 : 0;
}
