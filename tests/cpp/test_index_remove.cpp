// C++ checks of LeannIndex::remove (include/islands_amd.hpp over isl_index_remove).
// `test_index_remove cpu`: what needs no device; `test_index_remove gpu` adds removals on the device for both
// stored types and both rules.
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

static uint16_t bf16_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// what every shrunk index must satisfy, whatever the rule: the remap, and lists of survivors alone
static void check_shape(const LeannIndex& idx, const std::vector<uint64_t>& remap, const std::set<uint64_t>& gone,
                        uint64_t n, uint64_t m0) {
  uint64_t next = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (gone.count(i)) EXPECT(remap[i] == ISL_REMOVED);
    else EXPECT(remap[i] == next++);
  }
  EXPECT(idx.len() == next && remap.size() == n);
  for (uint64_t p = 0; p < next; ++p) {
    const uint64_t* nb = nullptr;
    size_t cnt = 0;
    EXPECT(isl_index_get_neighbors(idx.handle(), p, &nb, &cnt) == 1);
    std::set<uint64_t> seen;
    for (size_t i = 0; i < cnt; ++i) EXPECT(nb[i] < next && nb[i] != p && seen.insert(nb[i]).second);
    EXPECT(seen.size() <= m0);
  }
  const uint64_t* none = nullptr;
  size_t cnt = 0;
  EXPECT(isl_index_get_neighbors(idx.handle(), next, &none, &cnt) == 0);
}

int main(int argc, char** argv) {
  const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
  LeannConfig cfg;
  cfg.m = 4; cfg.m0 = 8; cfg.ef_construction = 40;
  {
    LeannIndex idx(cfg);
    const std::vector<uint8_t> b = idx.to_bytes();
    EXPECT(idx.remove({}).empty() && idx.is_empty() && idx.to_bytes() == b);  // no ids: nothing changes
    EXPECT(throws(ISL_ERR_NODE_NOT_FOUND, [&] { idx.remove({0}); }, 0));
    isl_build_options o = LeannIndex::build_options();
    o.select_rule = 7;
    EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { idx.remove({0}, o); }));
    EXPECT(isl_index_remove(nullptr, nullptr, nullptr, 0, nullptr, nullptr) == ISL_ERR_INVALID_ARGUMENT);
    CsrGraph g;
    g.num_nodes = 3;
    g.node_offsets = {0, 1, 2, 3};
    g.neighbors = {1, 2, 0};
    g.levels = {0, 0, 0};
    g.degree_counts = {1, 1, 1};
    g.entry_point = 0;
    LeannIndex ring = LeannIndex::from_csr(g, cfg, 16);
    const std::vector<uint8_t> rb = ring.to_bytes();
    EXPECT((ring.remove({}) == std::vector<uint64_t>{0, 1, 2}));
    EXPECT(throws(ISL_ERR_NODE_NOT_FOUND, [&] { ring.remove({1, 3}); }, 3));
    EXPECT(throws(ISL_ERR_UNSUPPORTED, [&] { ring.remove({1}); }));  // no rows resident
    EXPECT(ring.len() == 3 && ring.to_bytes() == rb && idx.to_bytes() == b);
  }
  if (gpu) {
    const uint64_t n = 300, d = 16;
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    std::vector<float> v(n * d);
    for (auto& x : v) x = u(rng);
    std::vector<uint16_t> hb(n * d);
    for (size_t i = 0; i < v.size(); ++i) hb[i] = bf16_bits(v[i]);
    std::vector<uint64_t> lv(n, 0);
    lv[7] = 2; lv[200] = 3;
    std::set<uint64_t> gone = {200, 7};  // the entry point and the runner-up
    while (gone.size() < 120) gone.insert(rng() % n);
    const std::vector<uint64_t> ids(gone.begin(), gone.end());
    const std::vector<float> q(v.begin() + 8 * d, v.begin() + 9 * d);
    for (uint32_t rule : {ISL_SELECT_REFERENCE, ISL_SELECT_DIVERSE}) {
      isl_build_options o = LeannIndex::build_options();
      o.select_rule = rule;
      {
        LeannIndex idx = LeannIndex::build(v, n, d, cfg, o, lv.data());
        const std::vector<uint8_t> before = idx.to_bytes();
        EXPECT(throws(ISL_ERR_NODE_NOT_FOUND, [&] { idx.remove({5, n}, o); }, n));
        EXPECT(idx.len() == n && idx.to_bytes() == before);
        const std::vector<uint64_t> remap = idx.remove(ids, o);
        check_shape(idx, remap, gone, n, cfg.m0);
        EXPECT(idx.dimension() == std::optional<uint64_t>(d));
        // neither 7 nor 200 survives: every survivor has level 0 and the lowest new id takes over
        uint64_t entry = 77;
        EXPECT(isl_index_entry_point(idx.handle(), &entry) == 1 && entry == 0 && isl_index_max_level(idx.handle()) == 0);
        if (!gone.count(8)) {
          const auto r = idx.search_with_params(q, 5, 64);
          EXPECT(r.size() == 5 && r[0].first == remap[8]);
        }
        // a second removal and an insert into what is left
        const std::vector<uint64_t> again = idx.remove({0, 1, 2}, o);
        EXPECT(again.size() == n - gone.size() && idx.len() == n - gone.size() - 3);
        EXPECT(idx.insert(std::vector<float>(v.begin(), v.begin() + 4 * d), 4, d, o) == n - gone.size() - 3);
      }
      {
        LeannIndex idx = LeannIndex::build_bf16(hb, n, d, cfg, o, lv.data());
        const std::vector<uint64_t> remap = idx.remove(ids, o);
        check_shape(idx, remap, gone, n, cfg.m0);
        EXPECT(idx.insert_bf16(std::vector<uint16_t>(hb.begin(), hb.begin() + 4 * d), 4, d, o) == n - gone.size());
      }
    }
  }
  std::printf("%s: %d failure(s)\n", gpu ? "gpu" : "cpu", failures);
  return failures ? 1 : 0;
}
