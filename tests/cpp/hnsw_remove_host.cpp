// isl_hnsw_remove's host-only half under AddressSanitizer (CPU build): the argument checks in their order over
// handles that need no device -- an empty graph from isl_hnsw_build, an empty image through isl_hnsw_from_bytes, and
// a graph with nodes and no resident rows put together here from isl_index_from_csr (isl_hnsw_from_layers would
// upload it) -- and the call that changes nothing.  Built from the library's own sources (host code instrumented,
// -fno-gpu-sanitize) by
//   make -C islands_amd/csrc ../lib/asan/hnsw_remove_host
// and linked without the search kernels' translation units: nothing called here reaches them without a device.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../islands_amd/csrc/common.hpp"

// search.hip is not part of this build; the one routine of it the call reaches before its first device call,
// restated (no lane of these handles is ever claimed)
namespace isl {
bool any_lane_busy(const isl_index* idx) {
  for (const auto& w : idx->ws)
    if (w.busy) return true;
  return false;
}
}  // namespace isl

static int failures = 0;
#define EXPECT(cond)                                                                        \
  do {                                                                                      \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)

static std::vector<uint8_t> bytes_of(const isl_hnsw* h) {
  uint8_t* p = nullptr;
  size_t n = 0;
  EXPECT(isl_hnsw_to_bytes(h, &p, &n) == ISL_OK && p);
  std::vector<uint8_t> out(p, p + (p ? n : 0));
  isl_free_bytes(p);
  return out;
}

int main() {
  isl_hnsw_config cfg;
  isl_hnsw_config_default(&cfg);
  cfg.m = 4; cfg.m0 = 8; cfg.ef_construction = 16;
  isl_build_options bad;
  isl_build_options_default(&bad);
  bad.select_rule = 7;
  isl_build_options low;
  isl_build_options_default(&low);
  low.select_rule = ISL_SELECT_DIVERSE;
  low.alpha = 0.5f;

  isl_hnsw *empty = nullptr, *image = nullptr;
  EXPECT(isl_hnsw_build(&cfg, nullptr, nullptr, 0, 0, nullptr, 0, ISL_MEM_HOST, 0, &empty) == ISL_OK);
  const std::vector<uint8_t> empty_bytes = bytes_of(empty);
  EXPECT(isl_hnsw_from_bytes(empty_bytes.data(), empty_bytes.size(), 0, &image) == ISL_OK);
  // twelve nodes in a ring on layer 0, no rows, no device
  const uint64_t n = 12, d = 16;
  std::vector<uint64_t> off(n + 1), nb(n), lv(n, 0);
  for (uint64_t i = 0; i <= n; ++i) off[i] = i;
  for (uint64_t i = 0; i < n; ++i) nb[i] = (i + 1) % n;
  isl_leann_config lcfg;
  isl_leann_config_paper_default(&lcfg);
  isl_hnsw ring;
  ring.m = 4; ring.m0 = 8; ring.ef_construction = 16; ring.dim = d;
  EXPECT(isl_index_from_csr(&lcfg, n, off.data(), nb.data(), lv.data(), nullptr, 1, 0, 0, 1, d, &ring.core) == ISL_OK);
  ring.core->is_hnsw = true;
  EXPECT(isl_hnsw_len(&ring) == n);

  const uint64_t some[3] = {3, 99, 5}, in_range[3] = {3, 5, 3};
  std::vector<uint64_t> remap(n, 77);
  uint64_t len = 77;
  auto untouched = [&] {
    for (uint64_t r : remap)
      if (r != 77) return false;
    return len == 77;
  };
  // 1. NULL h, NULL ids with n_ids > 0 -- before the options
  EXPECT(isl_hnsw_remove(nullptr, &bad, some, 3, remap.data(), &len) == ISL_ERR_INVALID_ARGUMENT);
  for (isl_hnsw* h : {empty, image, &ring}) {
    const bool has_nodes = h == &ring;
    EXPECT(isl_hnsw_remove(h, &bad, nullptr, 3, remap.data(), &len) == ISL_ERR_INVALID_ARGUMENT);
    EXPECT(std::strstr(isl_last_error_message(), "NULL") != nullptr);
    // 2. the options -- before n_ids == 0
    EXPECT(isl_hnsw_remove(h, &bad, nullptr, 0, remap.data(), &len) == ISL_ERR_INVALID_ARGUMENT);
    EXPECT(isl_hnsw_remove(h, &low, some, 3, remap.data(), &len) == ISL_ERR_INVALID_CONFIG);
    EXPECT(untouched());
    // 3. no ids: ISL_OK, the identity
    EXPECT(isl_hnsw_remove(h, nullptr, nullptr, 0, nullptr, nullptr) == ISL_OK);
    EXPECT(isl_hnsw_remove(h, nullptr, some, 0, remap.data(), &len) == ISL_OK);
    EXPECT(len == (has_nodes ? n : 0));
    for (uint64_t i = 0; i < n; ++i) EXPECT(remap[i] == (has_nodes ? i : 77));
    remap.assign(n, 77);
    len = 77;
    // 4. an id that is not below len, with the payload -- before the rows are missed
    EXPECT(isl_hnsw_remove(h, nullptr, some, 3, remap.data(), &len) == ISL_ERR_NODE_NOT_FOUND);
    EXPECT(isl_last_error_node() == (has_nodes ? 99 : 3));
    if (has_nodes) {
      // 5. no rows resident (and no device): refused before anything is allocated
      EXPECT(isl_hnsw_remove(h, nullptr, in_range, 3, remap.data(), &len) == ISL_ERR_UNSUPPORTED);
      EXPECT(std::strstr(isl_last_error_message(), "resident") != nullptr);
      EXPECT(isl_hnsw_len(h) == n);
    }
    EXPECT(untouched());
  }
  EXPECT(bytes_of(empty) == empty_bytes && bytes_of(image) == empty_bytes);
  isl_index_free(ring.core);
  isl_hnsw_free(empty);
  isl_hnsw_free(image);
  if (failures) { std::printf("hnsw remove host: %d failure(s)\n", failures); return 1; }
  std::printf("hnsw remove host: ok\n");
  return 0;
}
