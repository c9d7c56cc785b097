// C++ checks of LeannIndex::build_bf16 (include/islands_amd.hpp over isl_index_build_rows).
// `test_build_bf16 cpu`: what needs no device.  `test_build_bf16 gpu <rows> <n> <d> <want>`: one build from the
// n x d bf16 bit patterns in file <rows> (m 8, m0 16, ef_construction 40, both rules); the reference rule's
// bytes are compared with file <want>, which tests/test_cpp_build_bf16.py makes from the oracle's graph.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>

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

static std::vector<uint8_t> read_file(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
  LeannConfig cfg;
  isl_leann_config_paper_default(&cfg);
  cfg.m = 8; cfg.m0 = 16; cfg.ef_construction = 40;
  {
    LeannIndex e = LeannIndex::build_bf16({}, 0, 0, cfg);
    EXPECT(e.is_empty() && e.len() == 0);
    EXPECT(e.to_bytes() == LeannIndex::build({}, 0, 0, cfg).to_bytes());
    const std::vector<uint16_t> rows(32, 0x3F80);
    isl_build_options o = LeannIndex::build_options();
    o.select_rule = 7;
    EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { LeannIndex::build_bf16(rows, 4, 8, cfg, o); }));
    o.select_rule = ISL_SELECT_DIVERSE;
    o.alpha = 0.5f;
    EXPECT(throws(ISL_ERR_INVALID_CONFIG, [&] { LeannIndex::build_bf16(rows, 4, 8, cfg, o); }));
    EXPECT(throws(ISL_ERR_EMPTY_COLLECTION, [&] { LeannIndex::build_bf16(rows, 4, 0, cfg); }));
    LeannConfig wide = cfg;
    wide.m = 64; wide.m0 = 129; wide.ef_construction = 200;
    EXPECT(throws(ISL_ERR_UNSUPPORTED, [&] { LeannIndex::build_bf16(rows, 4, 8, wide); }));
    isl_index* h = nullptr;
    EXPECT(isl_index_build_rows(&cfg, nullptr, rows.data(), 5, 4, 8, nullptr, ISL_MEM_HOST, 0, &h) == ISL_ERR_INVALID_ARGUMENT);
    EXPECT(h == nullptr);
    EXPECT(isl_index_build_rows(&cfg, nullptr, rows.data(), ISL_DTYPE_BF16, 4, 8, nullptr, ISL_MEM_HOST, 0, nullptr) ==
           ISL_ERR_INVALID_ARGUMENT);
  }
  if (gpu) {
    if (argc < 6) { std::printf("usage: test_build_bf16 gpu <rows> <n> <d> <want>\n"); return 2; }
    const uint64_t n = std::strtoull(argv[3], nullptr, 10), d = std::strtoull(argv[4], nullptr, 10);
    const std::vector<uint8_t> raw = read_file(argv[2]), want = read_file(argv[5]);
    EXPECT(raw.size() == n * d * 2 && !want.empty());
    std::vector<uint16_t> bits(n * d);
    std::memcpy(bits.data(), raw.data(), std::min(raw.size(), bits.size() * 2));
    std::vector<float> rows(n * d);
    for (size_t i = 0; i < rows.size(); ++i) {
      const uint32_t u = (uint32_t)bits[i] << 16;
      std::memcpy(&rows[i], &u, 4);
    }
    LeannIndex idx = LeannIndex::build_bf16(bits, n, d, cfg);
    EXPECT(idx.len() == n && idx.dimension() == d);
    EXPECT(idx.to_bytes() == want);
    EXPECT(LeannIndex::build(rows, n, d, cfg).to_bytes() == want);
    isl_build_options o = LeannIndex::build_options();
    o.select_rule = ISL_SELECT_DIVERSE;
    LeannIndex dv = LeannIndex::build_bf16(bits, n, d, cfg, o);
    EXPECT(dv.to_bytes() == LeannIndex::build(rows, n, d, cfg, o).to_bytes());
    EXPECT(throws(ISL_ERR_UNSUPPORTED, [&] { dv.select_neighbors(3, {1, 2}, 2); }));  // bf16 rows
  }
  std::printf("%s: %d failure(s)\n", gpu ? "gpu" : "cpu", failures);
  return failures ? 1 : 0;
}
