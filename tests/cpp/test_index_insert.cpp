// C++ checks of LeannIndex::insert (include/islands_amd.hpp over isl_index_insert).
// `test_index_insert cpu`: what needs no device; `test_index_insert gpu` adds a split build on the device for
// both stored types.
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
static bool throws(isl_status st, F f, uint64_t expected = 0, uint64_t actual = 0) {
  try { f(); } catch (const CoreError& e) {
    return e.status == st && (st != ISL_ERR_DIMENSION_MISMATCH || (e.expected == expected && e.actual == actual));
  }
  return false;
}

static uint16_t bf16_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

int main(int argc, char** argv) {
  const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
  LeannConfig cfg;
  cfg.m = 8; cfg.m0 = 16; cfg.ef_construction = 40;
  {
    LeannIndex idx(cfg);
    const std::vector<uint8_t> b = idx.to_bytes();
    EXPECT(idx.insert({}, 0, 4) == 0 && idx.is_empty() && idx.to_bytes() == b);  // no rows: nothing changes
    EXPECT(idx.insert_bf16({}, 0, 4) == 0 && idx.to_bytes() == b);
    isl_build_options o = LeannIndex::build_options();
    o.select_rule = 7;
    EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { idx.insert(std::vector<float>(8, 1.f), 2, 4, o); }));
    EXPECT(throws(ISL_ERR_EMPTY_COLLECTION, [&] { idx.insert(std::vector<float>(8, 1.f), 2, 0); }));
    EXPECT(isl_index_insert(nullptr, nullptr, nullptr, ISL_DTYPE_F32, 0, 0, nullptr, ISL_MEM_HOST, nullptr) ==
           ISL_ERR_INVALID_ARGUMENT);
    // a non-empty index that needs no device: the dimension is compared first, with the payload
    CsrGraph g;
    g.num_nodes = 3;
    g.node_offsets = {0, 1, 2, 3};
    g.neighbors = {1, 2, 0};
    g.levels = {0, 0, 0};
    g.degree_counts = {1, 1, 1};
    g.entry_point = 0;
    LeannIndex ring = LeannIndex::from_csr(g, cfg, 16);
    EXPECT(throws(ISL_ERR_DIMENSION_MISMATCH, [&] { ring.insert(std::vector<float>(24, 1.f), 2, 12); }, 16, 12));
    EXPECT(throws(ISL_ERR_UNSUPPORTED, [&] { ring.insert(std::vector<float>(32, 1.f), 2, 16); }));  // no rows resident
    EXPECT(ring.len() == 3 && idx.is_empty() && idx.to_bytes() == b);
  }
  if (gpu) {
    const uint64_t n = 300, n0 = 180, d = 16;
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    std::vector<float> v(n * d);
    for (auto& x : v) x = u(rng);
    std::vector<uint16_t> hb(n * d);
    for (size_t i = 0; i < v.size(); ++i) hb[i] = bf16_bits(v[i]);
    std::vector<uint64_t> lv(n, 0);
    lv[7] = 2; lv[200] = 3;
    const std::vector<float> head(v.begin(), v.begin() + n0 * d), tail(v.begin() + n0 * d, v.end());
    const std::vector<uint16_t> head16(hb.begin(), hb.begin() + n0 * d), tail16(hb.begin() + n0 * d, hb.end());
    const std::vector<float> q(v.begin() + 7 * d, v.begin() + 8 * d);
    for (uint32_t rule : {ISL_SELECT_REFERENCE, ISL_SELECT_DIVERSE}) {
      isl_build_options o = LeannIndex::build_options();
      o.select_rule = rule;
      {
        LeannIndex whole = LeannIndex::build(v, n, d, cfg, o, lv.data());
        LeannIndex idx = LeannIndex::build(head, n0, d, cfg, o, lv.data());
        EXPECT(throws(ISL_ERR_DIMENSION_MISMATCH, [&] { idx.insert(std::vector<float>(24, 1.f), 2, 12, o); }, d, 12));
        EXPECT(throws(ISL_ERR_UNSUPPORTED, [&] { idx.insert_bf16(tail16, n - n0, d, o); }));  // the stored type
        EXPECT(idx.len() == n0);
        EXPECT(idx.insert(tail, n - n0, d, o, lv.data() + n0) == n0);
        EXPECT(idx.len() == n && idx.dimension() == std::optional<uint64_t>(d));
        EXPECT(idx.to_bytes() == whole.to_bytes());
        const auto r = idx.search_with_params(q, 5, 64), w = whole.search_with_params(q, 5, 64);
        EXPECT(r == w && r.size() == 5 && r[0].first == 7);
      }
      {
        LeannIndex whole = LeannIndex::build_bf16(hb, n, d, cfg, o, lv.data());
        LeannIndex idx = LeannIndex::build_bf16(head16, n0, d, cfg, o, lv.data());
        EXPECT(throws(ISL_ERR_UNSUPPORTED, [&] { idx.insert(tail, n - n0, d, o); }));
        EXPECT(idx.insert_bf16(tail16, n - n0, d, o, lv.data() + n0) == n0);
        EXPECT(idx.len() == n && idx.to_bytes() == whole.to_bytes());
        EXPECT(idx.search_with_params(q, 5, 64) == whole.search_with_params(q, 5, 64));
      }
    }
  }
  std::printf("%s: %d failure(s)\n", gpu ? "gpu" : "cpu", failures);
  return failures ? 1 : 0;
}
