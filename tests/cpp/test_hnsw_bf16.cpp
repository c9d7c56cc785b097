// C++ checks of an HnswGraph over bf16 rows (include/islands_amd.hpp over isl_hnsw_build_rows,
// isl_hnsw_insert_rows, isl_hnsw_row_storage).
// `test_hnsw_bf16 cpu`: the mirror's argument checks and the empty graph, which need no device;
// `test_hnsw_bf16 gpu` adds a build, a split build plus insert, and a removal on the device.
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

// round to nearest even, as the tests' to_bf16_bits
static uint16_t to_bf16(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
static float widen(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float x;
  std::memcpy(&x, &u, 4);
  return x;
}

int main(int argc, char** argv) {
  const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
  isl_hnsw_config cfg;
  isl_hnsw_config_default(&cfg);
  cfg.m = 8; cfg.m0 = 16; cfg.ef_construction = 64;
  {
    // no rows: the empty graph, the f32 one's bytes, nothing stored
    HnswGraph g = HnswGraph::build_bf16({}, 0, &cfg);
    const std::vector<uint8_t> b = g.to_bytes();
    EXPECT(g.is_empty() && b == HnswGraph::build({}, 0, &cfg).to_bytes());
    EXPECT(g.row_storage().dtype == ISL_DTYPE_F32 && g.row_storage().block_bytes == 0);
    EXPECT(g.insert_bf16({}, 4) == 0 && g.is_empty() && g.to_bytes() == b);
    // a level at max_layers, an unknown rule, d == 0: refused before any device call
    EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { g.insert_bf16(std::vector<uint16_t>(8, 0x3F80), 4, {0, 16}); }));
    EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { HnswGraph::build_bf16(std::vector<uint16_t>(8, 0x3F80), 4, &cfg, {0, 16}); }));
    isl_build_options o;
    isl_build_options_default(&o);
    o.select_rule = 7;
    EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { g.insert_bf16(std::vector<uint16_t>(8, 0x3F80), 4, {}, 0, &o); }));
    EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { HnswGraph::build_bf16(std::vector<uint16_t>(8, 0x3F80), 4, &cfg, {}, 0, &o); }));
    isl_hnsw_config bad = cfg;
    bad.m0 = 4;  // M0 < M
    EXPECT(throws(ISL_ERR_INVALID_CONFIG, [&] { HnswGraph::build_bf16(std::vector<uint16_t>(8, 0x3F80), 4, &bad); }));
    // the C calls themselves: NULL handles, the dtype
    const uint16_t one[4] = {0x3F80, 0, 0, 0};
    isl_hnsw* h = reinterpret_cast<isl_hnsw*>(0x1);
    EXPECT(isl_hnsw_build_rows(&cfg, nullptr, one, 7, 1, 4, nullptr, 0, ISL_MEM_HOST, 0, &h) == ISL_ERR_INVALID_ARGUMENT);
    EXPECT(isl_hnsw_build_rows(&cfg, nullptr, one, ISL_DTYPE_FP8_E4M3, 1, 4, nullptr, 0, ISL_MEM_HOST, 0, &h) ==
           ISL_ERR_UNSUPPORTED);
    EXPECT(h == reinterpret_cast<isl_hnsw*>(0x1));
    EXPECT(isl_hnsw_insert_rows(nullptr, nullptr, nullptr, ISL_DTYPE_BF16, 0, 0, nullptr, 0, ISL_MEM_HOST, nullptr) ==
           ISL_ERR_INVALID_ARGUMENT);
    EXPECT(isl_hnsw_row_storage(nullptr, nullptr, nullptr) == ISL_ERR_INVALID_ARGUMENT);
    EXPECT(g.is_empty() && g.to_bytes() == b);
  }
  if (gpu) {
    const uint64_t n = 300, n0 = 180, d = 16;
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    std::vector<uint16_t> bits(n * d);
    std::vector<float> wide(n * d);
    for (uint64_t i = 0; i < n * d; ++i) { bits[i] = to_bf16(u(rng)); wide[i] = widen(bits[i]); }
    const std::vector<uint16_t> head(bits.begin(), bits.begin() + n0 * d), tail(bits.begin() + n0 * d, bits.end());
    for (uint32_t rule : {ISL_SELECT_REFERENCE, ISL_SELECT_DIVERSE}) {
      isl_build_options o;
      isl_build_options_default(&o);
      o.select_rule = rule;
      HnswGraph whole = HnswGraph::build_bf16(bits, d, &cfg, {}, 3, &o);
      // the graph of the widened rows, and half its row bytes
      HnswGraph f32 = HnswGraph::build(wide, d, &cfg, {}, 3, &o);
      EXPECT(whole.to_bytes() == f32.to_bytes());
      EXPECT(whole.row_storage().dtype == ISL_DTYPE_BF16 && f32.row_storage().dtype == ISL_DTYPE_F32);
      EXPECT(whole.row_storage().block_bytes * 2 <= f32.row_storage().block_bytes + 4096);
      HnswGraph g = HnswGraph::build_bf16(head, d, &cfg, {}, 3, &o);
      const std::vector<uint8_t> before = g.to_bytes();
      // f32 rows into a bf16 graph: refused, nothing changed
      EXPECT(throws(ISL_ERR_UNSUPPORTED, [&] { g.insert(std::vector<float>(wide.begin() + n0 * d, wide.end()), d, {}, 3, &o); }));
      EXPECT(throws(ISL_ERR_UNSUPPORTED, [&] { f32.insert_bf16(tail, d, {}, 3, &o); }));
      EXPECT(g.len() == n0 && g.to_bytes() == before);
      EXPECT(g.insert_bf16(tail, d, {}, 3, &o) == n0);  // the seed's stream continues at position len
      EXPECT(g.len() == n && g.to_bytes() == whole.to_bytes());
      EXPECT(g.row_storage().dtype == ISL_DTYPE_BF16 && g.row_storage().block_bytes == whole.row_storage().block_bytes);
      const auto row = g.get_vector(n - 1);
      EXPECT(row && std::memcmp(row->data(), wide.data() + (n - 1) * d, d * 4) == 0);
      const std::vector<float> q(wide.begin() + 7 * d, wide.begin() + 8 * d);
      EXPECT(g.search(q, 5, 64) == f32.search(q, 5, 64));
      // remove: the three graphs shrink alike, and the bf16 ones stay bf16
      const std::vector<uint64_t> gone = {0, 7, 8, 120, 181, 299};
      isl_build_options ro = LeannIndex::build_options();
      ro.select_rule = rule;
      const auto r0 = whole.remove(gone, ro), r1 = g.remove(gone, ro), r2 = f32.remove(gone, ro);
      EXPECT(r0 == r1 && r0 == r2 && whole.len() == n - gone.size());
      EXPECT(whole.to_bytes() == g.to_bytes() && whole.to_bytes() == f32.to_bytes());
      EXPECT(whole.row_storage().dtype == ISL_DTYPE_BF16 && g.row_storage().dtype == ISL_DTYPE_BF16);
      const auto kept = whole.get_vector(0);  // old node 1
      EXPECT(kept && std::memcmp(kept->data(), wide.data() + d, d * 4) == 0);
      EXPECT(whole.search(q, 5, 64) == f32.search(q, 5, 64));
    }
  }
  std::printf("%s: %d failure(s)\n", gpu ? "gpu" : "cpu", failures);
  return failures ? 1 : 0;
}
