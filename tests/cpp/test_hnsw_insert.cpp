// C++ checks of HnswGraph::insert (include/islands_amd.hpp over isl_hnsw_insert).
// `test_hnsw_insert cpu`: what needs no device; `test_hnsw_insert gpu` adds a split build on the device.
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
  cfg.m = 8; cfg.m0 = 16; cfg.ef_construction = 64;
  {
    HnswGraph g = HnswGraph::build({}, 0, &cfg);
    const std::vector<uint8_t> b = g.to_bytes();
    EXPECT(g.insert({}, 4) == 0 && g.is_empty() && g.to_bytes() == b);  // no rows: nothing changes
    EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { g.insert(std::vector<float>(8, 1.f), 4, {0, 16}); }));
    isl_build_options o;
    isl_build_options_default(&o);
    o.select_rule = 7;
    EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { g.insert(std::vector<float>(8, 1.f), 4, {}, 0, &o); }));
    EXPECT(isl_hnsw_insert(nullptr, nullptr, nullptr, 0, 0, nullptr, 0, ISL_MEM_HOST, nullptr) == ISL_ERR_INVALID_ARGUMENT);
    EXPECT(g.is_empty() && g.to_bytes() == b);
  }
  if (gpu) {
    const uint64_t n = 300, n0 = 180, d = 16;
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    std::vector<float> v(n * d);
    for (auto& x : v) x = u(rng);
    const std::vector<float> head(v.begin(), v.begin() + n0 * d), tail(v.begin() + n0 * d, v.end());
    for (uint32_t rule : {ISL_SELECT_REFERENCE, ISL_SELECT_DIVERSE}) {
      isl_build_options o;
      isl_build_options_default(&o);
      o.select_rule = rule;
      HnswGraph whole = HnswGraph::build(v, d, &cfg, {}, 3, &o);
      HnswGraph g = HnswGraph::build(head, d, &cfg, {}, 3, &o);
      EXPECT(throws(ISL_ERR_DIMENSION_MISMATCH, [&] { g.insert(std::vector<float>(24, 1.f), 12, {}, 3, &o); }));
      EXPECT(g.len() == n0);
      EXPECT(g.insert(tail, d, {}, 3, &o) == n0);  // the seed's stream continues at position len
      EXPECT(g.len() == n);
      EXPECT(g.to_bytes() == whole.to_bytes());
      EXPECT(g.neighbors(n - 1, 0) == whole.neighbors(n - 1, 0));
      const auto row = g.get_vector(n - 1);
      EXPECT(row && std::memcmp(row->data(), v.data() + (n - 1) * d, d * 4) == 0);
      const auto r = g.search(std::vector<float>(v.begin() + 7 * d, v.begin() + 8 * d), 1, 64);
      const auto w = whole.search(std::vector<float>(v.begin() + 7 * d, v.begin() + 8 * d), 1, 64);
      EXPECT(r == w && r.size() == 1);
    }
  }
  std::printf("%s: %d failure(s)\n", gpu ? "gpu" : "cpu", failures);
  return failures ? 1 : 0;
}
