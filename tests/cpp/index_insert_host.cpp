// isl_index_insert's host-only half under AddressSanitizer (CPU build): the argument checks in their order over
// handles that need no device -- an empty index, a ring from isl_index_from_csr, an image through
// isl_index_from_bytes -- the call that changes nothing, and, where no gfx950 is visible, the failure of a
// non-empty insert, after which the handle must serialise to the bytes it had.  Built from the library's own
// sources (host code instrumented, -fno-gpu-sanitize) by
//   make -C islands_amd/csrc ../lib/asan/index_insert_host
// and linked without the search kernels' translation units: nothing called here reaches them without a device.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../islands_amd/csrc/common.hpp"

// search.hip is not part of this build; the one routine of it the insert reaches before its first device call,
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

static std::vector<uint8_t> bytes_of(const isl_index* idx) {
  uint8_t* p = nullptr;
  size_t n = 0;
  EXPECT(isl_index_to_bytes(idx, &p, &n) == ISL_OK && p);
  std::vector<uint8_t> out(p, p + (p ? n : 0));
  isl_free_bytes(p);
  return out;
}

int main(int argc, char** argv) {
  const bool no_device = argc > 1 && std::strcmp(argv[1], "nodevice") == 0;
  isl_leann_config cfg;
  isl_leann_config_paper_default(&cfg);
  cfg.m = 8; cfg.m0 = 16; cfg.ef_construction = 40;
  const uint64_t n = 12, d = 16;
  std::vector<uint64_t> off(n + 1), nb(n), lv(n, 0);
  for (uint64_t i = 0; i <= n; ++i) off[i] = i;
  for (uint64_t i = 0; i < n; ++i) nb[i] = (i + 1) % n;
  std::vector<float> rows(8 * d, 0.25f);
  std::vector<uint64_t> levels(8, 1);
  isl_build_options bad;
  isl_build_options_default(&bad);
  bad.select_rule = 7;

  isl_index *empty = nullptr, *ring = nullptr, *image = nullptr;
  EXPECT(isl_index_new(&cfg, &empty) == ISL_OK);
  EXPECT(isl_index_from_csr(&cfg, n, off.data(), nb.data(), lv.data(), nullptr, 1, 0, 0, 1, d, &ring) == ISL_OK);
  const std::vector<uint8_t> empty_bytes = bytes_of(empty), ring_bytes = bytes_of(ring);
  EXPECT(isl_index_from_bytes(ring_bytes.data(), ring_bytes.size(), &image) == ISL_OK);

  uint64_t first = 77;
  EXPECT(isl_index_insert(nullptr, &bad, rows.data(), 9, 8, d, nullptr, ISL_MEM_HOST, &first) == ISL_ERR_INVALID_ARGUMENT);
  for (isl_index* idx : {empty, ring, image}) {
    const bool has_nodes = idx != empty;
    EXPECT(isl_index_insert(idx, &bad, nullptr, 9, 8, d, nullptr, ISL_MEM_HOST, &first) == ISL_ERR_INVALID_ARGUMENT);
    EXPECT(isl_index_insert(idx, &bad, rows.data(), 9, 0, d, nullptr, ISL_MEM_HOST, &first) == ISL_ERR_INVALID_ARGUMENT);
    EXPECT(isl_index_insert(idx, nullptr, rows.data(), 9, 0, d, nullptr, ISL_MEM_HOST, &first) == ISL_ERR_INVALID_ARGUMENT);
    EXPECT(first == 77);
    EXPECT(isl_index_insert(idx, nullptr, nullptr, ISL_DTYPE_BF16, 0, 3, nullptr, ISL_MEM_HOST, nullptr) == ISL_OK);
    EXPECT(isl_index_insert(idx, nullptr, nullptr, ISL_DTYPE_F32, 0, 3, nullptr, ISL_MEM_HOST, &first) == ISL_OK);
    EXPECT(first == (has_nodes ? n : 0));
    first = 77;
    if (has_nodes) {
      EXPECT(isl_index_insert(idx, nullptr, rows.data(), ISL_DTYPE_F32, 8, 12, nullptr, ISL_MEM_HOST, &first) ==
             ISL_ERR_DIMENSION_MISMATCH);
      EXPECT(isl_last_error_expected() == d && isl_last_error_actual() == 12);
      EXPECT(isl_index_insert(idx, nullptr, rows.data(), ISL_DTYPE_F32, 8, 0, nullptr, ISL_MEM_HOST, &first) ==
             ISL_ERR_DIMENSION_MISMATCH);
      // no rows resident (and no device): refused before anything is allocated
      EXPECT(isl_index_insert(idx, nullptr, rows.data(), ISL_DTYPE_F32, 8, d, levels.data(), ISL_MEM_HOST, &first) ==
             ISL_ERR_UNSUPPORTED);
      EXPECT(isl_index_insert(idx, nullptr, rows.data(), ISL_DTYPE_BF16, 8, d, levels.data(), ISL_MEM_HOST, &first) ==
             ISL_ERR_UNSUPPORTED);
    } else {
      EXPECT(isl_index_insert(idx, nullptr, rows.data(), ISL_DTYPE_F32, 8, 0, nullptr, ISL_MEM_HOST, &first) ==
             ISL_ERR_EMPTY_COLLECTION);
      // the empty handle takes the rows as a build would; where no gfx950 is visible (`nodevice`, as the caller
      // found: this program does not ask the runtime, whose start-up allocations LeakSanitizer would report) that
      // ends in Device at the first device call, the handle as it was.  Beside a device the call would go on into
      // the kernels' translation units, which this build leaves out: tests/test_gpu_index_insert.py covers it.
      if (no_device) {
        EXPECT(isl_index_insert(idx, nullptr, rows.data(), ISL_DTYPE_F32, 8, d, levels.data(), ISL_MEM_HOST, &first) ==
               ISL_ERR_DEVICE);
        EXPECT(first == 77 && isl_index_len(idx) == 0 && bytes_of(idx) == empty_bytes);
      }
      first = 77;
    }
    EXPECT(first == 77);
  }
  EXPECT(bytes_of(ring) == ring_bytes && bytes_of(image) == ring_bytes && isl_index_len(ring) == n);
  // the shape limits of the handle's config, before any device call
  cfg.m = 64; cfg.m0 = 129; cfg.ef_construction = 200;
  isl_index* wide = nullptr;
  EXPECT(isl_index_new(&cfg, &wide) == ISL_OK);
  EXPECT(isl_index_insert(wide, nullptr, rows.data(), ISL_DTYPE_F32, 8, d, nullptr, ISL_MEM_HOST, &first) == ISL_ERR_UNSUPPORTED);
  EXPECT(std::strstr(isl_last_error_message(), "m0 <= 128") != nullptr && first == 77);
  isl_index_free(wide);
  isl_index_free(empty);
  isl_index_free(ring);
  isl_index_free(image);
  if (failures) { std::printf("index insert host: %d failure(s)\n", failures); return 1; }
  std::printf("index insert host: ok\n");
  return 0;
}
