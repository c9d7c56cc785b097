// C++ checks of LeannIndex::convert_rows / read_rows (include/islands_amd.hpp over isl_index_convert_rows and
// isl_index_read_rows).  `test_convert_rows cpu`: what needs no device; `test_convert_rows gpu` adds the
// conversions of a built index on the device.
#include <cmath>
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

// narrow_bf16 of the header for a value that is not a NaN
static uint16_t bf16_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// e4m3(code) * 2^e from the format's definition
static float e4m3_image(uint8_t c, int e) {
  const int field = (c >> 3) & 15, m = c & 7;
  const float v = field == 0 ? std::ldexp((float)m, -9) : std::ldexp((float)(8 + m), field - 10);
  return std::ldexp(c & 0x80 ? -v : v, e);
}

template <typename T>
static std::vector<uint8_t> bytes_of(const std::vector<T>& v) {
  std::vector<uint8_t> b(v.size() * sizeof(T));
  if (!b.empty()) std::memcpy(b.data(), v.data(), b.size());
  return b;
}

int main(int argc, char** argv) {
  const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
  LeannConfig cfg;
  cfg.m = 4; cfg.m0 = 8; cfg.ef_construction = 40;
  {
    CsrGraph g;
    g.num_nodes = 3;
    g.node_offsets = {0, 1, 2, 3};
    g.neighbors = {1, 2, 0};
    g.levels = {0, 0, 0};
    g.degree_counts = {1, 1, 1};
    g.entry_point = 0;
    LeannIndex ring = LeannIndex::from_csr(g, cfg, 16);
    const std::vector<uint8_t> rb = ring.to_bytes();
    EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { ring.convert_rows(7); }));
    EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { ring.convert_rows(ISL_DTYPE_FP8_E4M3, 33); }));
    EXPECT(throws(ISL_ERR_UNSUPPORTED, [&] { ring.convert_rows(ISL_DTYPE_FP8_E4M3); }));  // no rows resident
    EXPECT(throws(ISL_ERR_UNSUPPORTED, [&] { ring.convert_rows(ISL_DTYPE_BF16, 33); }));  // (the exponent is fp8's)
    EXPECT(throws(ISL_ERR_UNSUPPORTED, [&] { ring.read_rows(0, 1); }));
    EXPECT(isl_index_convert_rows(nullptr, ISL_DTYPE_F32, 0) == ISL_ERR_INVALID_ARGUMENT);
    EXPECT(isl_index_read_rows(nullptr, 0, 0, nullptr, ISL_MEM_HOST) == ISL_ERR_INVALID_ARGUMENT);
    int32_t e = 77;
    EXPECT(isl_quantize_fp8_e4m3(nullptr, 0, 16, ISL_FP8_SCALE_AUTO, nullptr, &e, ISL_MEM_HOST, 0, nullptr) == ISL_OK && e == -32);
    EXPECT(isl_round_bf16(nullptr, 4, 4, nullptr, ISL_MEM_HOST, 0, nullptr) == ISL_ERR_INVALID_ARGUMENT);
    EXPECT(ring.len() == 3 && ring.to_bytes() == rb && ring.row_storage().block_bytes == 0);
  }
  if (gpu) {
    const uint64_t n = 300, d = 24;  // d = 24: fp8 rows at a padded pitch of 32
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    std::vector<float> v(n * d);
    for (auto& x : v) x = u(rng);
    v[17] = 1.0f;  // the top of the table: the automatic exponent is that of 1.0 = 448 * 2^-9 * 1.14..
    LeannIndex idx = LeannIndex::build(v, n, d, cfg);
    EXPECT(idx.row_storage().dtype == ISL_DTYPE_F32 && idx.read_rows(0, n) == bytes_of(v));
    EXPECT(throws(ISL_ERR_NODE_NOT_FOUND, [&] { idx.read_rows(n - 1, 2); }, n));
    // f32 -> bf16
    idx.convert_rows(ISL_DTYPE_BF16);
    std::vector<uint16_t> hb(n * d);
    for (size_t i = 0; i < v.size(); ++i) hb[i] = bf16_bits(v[i]);
    EXPECT(idx.row_storage().dtype == ISL_DTYPE_BF16 && idx.read_rows(0, n) == bytes_of(hb));
    EXPECT(idx.read_rows(7, 2) == bytes_of(std::vector<uint16_t>(hb.begin() + 7 * d, hb.begin() + 9 * d)));
    // bf16 -> fp8, automatic exponent: the smallest e with 1.0 <= 448 * 2^e
    idx.convert_rows(ISL_DTYPE_FP8_E4M3);
    const LeannIndex::RowStorage s = idx.row_storage();
    EXPECT(s.dtype == ISL_DTYPE_FP8_E4M3 && s.scale_exp == -8 && s.block_bytes == n * 32 + 1024);
    const std::vector<uint8_t> codes = idx.read_rows(0, n);
    EXPECT(codes.size() == n * d);
    idx.convert_rows(ISL_DTYPE_FP8_E4M3);               // the stored type: nothing happens
    idx.convert_rows(ISL_DTYPE_FP8_E4M3, s.scale_exp);  // ... under its own exponent as well
    EXPECT(throws(ISL_ERR_UNSUPPORTED, [&] { idx.convert_rows(ISL_DTYPE_FP8_E4M3, s.scale_exp + 1); }));
    EXPECT(idx.read_rows(0, n) == codes && idx.row_storage().scale_exp == s.scale_exp);
    EXPECT(throws(ISL_ERR_UNSUPPORTED, [&] { idx.insert(std::vector<float>(v.begin(), v.begin() + 2 * d), 2, d); }));
    // fp8 -> f32: the images, which every code's definition gives; the index takes rows again
    idx.convert_rows(ISL_DTYPE_F32);
    std::vector<float> images(n * d);
    bool near = true;
    for (size_t i = 0; i < images.size(); ++i) {
      images[i] = e4m3_image(codes[i], s.scale_exp);
      // bf16 moves v by 2^-9 |v| at the most, e4m3 by 2^-4 of that, or by half a subnormal step
      near = near && std::fabs(images[i] - v[i]) <= std::fabs(v[i]) * (0.0625f + 0.00390625f) + std::ldexp(1.f, s.scale_exp - 10);
    }
    EXPECT(near);
    EXPECT(idx.read_rows(0, n) == bytes_of(images));
    const std::vector<float> q(images.begin() + 8 * d, images.begin() + 9 * d);
    const auto r = idx.search_with_params(q, 5, 64);
    EXPECT(r.size() == 5 && r[0].first == 8);
    EXPECT(idx.insert(std::vector<float>(v.begin(), v.begin() + 4 * d), 4, d) == n && idx.len() == n + 4);
    // ... and narrows again under the same exponent: the old rows' codes are the old codes
    idx.convert_rows(ISL_DTYPE_FP8_E4M3, s.scale_exp);
    const std::vector<uint8_t> grown = idx.read_rows(0, n + 4);
    EXPECT(std::vector<uint8_t>(grown.begin(), grown.begin() + n * d) == codes);
    EXPECT(idx.search_with_params(q, 5, 64).size() == 5);
  }
  std::printf("%s: %d failure(s)\n", gpu ? "gpu" : "cpu", failures);
  return failures ? 1 : 0;
}
