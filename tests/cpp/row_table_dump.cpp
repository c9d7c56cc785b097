// Prints the answers of islands_amd/csrc/row_table_plan.hpp over a grid of shapes, one line per case; plain
// C++, no device.  tests/test_row_table_cpu.py compares the output with a Python restatement of the rule.
//   layout <dtype> <d> -> elem_size stride slack
//   alloc <dtype> <d> <n> -> elements of the block
//   norms <d> <n> -> rows per widened chunk, floats of the chunk buffer
//   cache <d> <slab> <nvec> -> bytes isl_index_recompute_cache_bytes reports
#include "../../islands_amd/csrc/row_table_plan.hpp"

#include <cstdio>
#include <vector>

int main() {
  using namespace isl_rows;
  std::vector<uint64_t> ds;
  for (uint64_t d = 1; d <= 70; ++d) ds.push_back(d);
  for (uint64_t d : {768ull, 4096ull, 65536ull}) ds.push_back(d);
  const uint64_t ns[] = {1, 1000, 10000000};
  for (int32_t dtype : {(int32_t)ISL_DTYPE_F32, (int32_t)ISL_DTYPE_BF16})
    for (uint64_t d : ds) {
      std::printf("layout %d %llu -> %llu %llu %llu\n", dtype, (unsigned long long)d, (unsigned long long)elem_size(dtype),
                  (unsigned long long)stride(dtype, d), (unsigned long long)slack(dtype));
      for (uint64_t n : ns)
        std::printf("alloc %d %llu %llu -> %llu\n", dtype, (unsigned long long)d, (unsigned long long)n,
                    (unsigned long long)alloc_elems(dtype, n, d));
    }
  for (uint64_t d : ds)
    for (uint64_t n : ns) {
      const uint64_t chunk = norm_chunk_rows(n, d);
      std::printf("norms %llu %llu -> %llu %llu\n", (unsigned long long)d, (unsigned long long)n, (unsigned long long)chunk,
                  (unsigned long long)norm_chunk_floats(chunk, d));
      for (uint64_t slab : {(uint64_t)0, n < 256 ? n : (uint64_t)256, n})
        std::printf("cache %llu %llu %llu -> %llu\n", (unsigned long long)d, (unsigned long long)slab, (unsigned long long)n,
                    (unsigned long long)recompute_cache_bytes(slab, d, n));
    }
  return 0;
}
