// Prints the layout of fp8 rows (ISL_DTYPE_FP8_E4M3) from islands_amd/csrc/row_table_plan.hpp, one line per
// case; plain C++, no device.  tests/test_fp8_rows_cpu.py compares the output with a Python restatement.
//   layout <dtype> <d> -> elem_size stride slack
//   alloc <dtype> <d> <n> -> elements of the block
#include "../../islands_amd/csrc/row_table_plan.hpp"

#include <cstdio>

int main() {
  using namespace isl_rows;
  const int32_t dtype = ISL_DTYPE_FP8_E4M3;
  for (uint64_t d : {1ull, 15ull, 16ull, 17ull, 768ull, 4096ull}) {
    std::printf("layout %d %llu -> %llu %llu %llu\n", dtype, (unsigned long long)d, (unsigned long long)elem_size(dtype),
                (unsigned long long)stride(dtype, d), (unsigned long long)slack(dtype));
    for (uint64_t n : {1ull, 1000ull, 10000000ull})
      std::printf("alloc %d %llu %llu -> %llu\n", dtype, (unsigned long long)d, (unsigned long long)n,
                  (unsigned long long)alloc_elems(dtype, n, d));
  }
  std::printf("scale_exp %d %d\n", kMinScaleExp, kMaxScaleExp);
  return 0;
}
