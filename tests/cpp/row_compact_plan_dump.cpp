// Prints the answers of islands_amd/csrc/row_compact_plan.hpp and of the capacity arithmetic of row_table_plan.hpp;
// plain C++, no device.  tests/test_row_compact_plan_cpu.py replays the plan on a numpy array and compares the
// arithmetic with a Python restatement.
// stdin: "<n> <stage_rows>" then the n ascending survivors.  stdout:
//   first <id>                           the first new id whose row moves (n: none)
//   move <first_new> <count> <staged>    one line per move, in order
//   stage <row_bytes> <n> <env or -> -> rows per staged move
//   alloc <dtype> <d> <capacity> -> elements of the block
//   tail <dtype> <d> <capacity> <first> -> elements from row `first` to the end of the block
//   fill <dtype> <capacity> <first> <count> -> elements of slack a fill of those rows clears
//   vacated <dtype> <d> <n> <n0> -> elements the compaction of n0 rows to n clears
#include "../../islands_amd/csrc/row_compact_plan.hpp"
#include "../../islands_amd/csrc/row_table_plan.hpp"

#include <cstdio>
#include <vector>

int main() {
  unsigned long long n = 0, stage = 0;
  if (std::scanf("%llu %llu", &n, &stage) != 2) return 2;
  std::vector<uint32_t> s(n);
  for (auto& x : s) {
    unsigned long long v = 0;
    if (std::scanf("%llu", &v) != 1) return 2;
    x = (uint32_t)v;
  }
  std::vector<isl_plan::RowMove> moves;
  isl_plan::plan_row_moves(s.data(), n, stage, moves);
  std::printf("first %llu\n", (unsigned long long)isl_plan::first_moved(s.data(), n));
  for (const isl_plan::RowMove& m : moves)
    std::printf("move %llu %llu %d\n", (unsigned long long)m.first_new, (unsigned long long)m.count, m.staged ? 1 : 0);
  const char* envs[] = {nullptr, "", "0", "-3", "1", "7", "1000000"};
  for (uint64_t row_bytes : {16ull, 3076ull, 1ull << 27})
    for (uint64_t rows : {0ull, 1ull, 300ull, 10000000ull})
      for (const char* e : envs)
        std::printf("stage %llu %llu %s -> %llu\n", (unsigned long long)row_bytes, (unsigned long long)rows,
                    !e ? "-" : *e ? e : "empty", (unsigned long long)isl_plan::compact_stage_rows(row_bytes, rows, e));
  using namespace isl_rows;
  for (int32_t dtype : {(int32_t)ISL_DTYPE_F32, (int32_t)ISL_DTYPE_BF16, (int32_t)ISL_DTYPE_FP8_E4M3})
    for (uint64_t d : {3ull, 100ull, 768ull})
      for (uint64_t cap : {1ull, 300ull, 512ull, 10000000ull}) {
        std::printf("alloc %d %llu %llu -> %llu\n", dtype, (unsigned long long)d, (unsigned long long)cap,
                    (unsigned long long)alloc_elems(dtype, cap, d));
        for (uint64_t first : {(uint64_t)0, (uint64_t)1, (uint64_t)299, cap})
          if (first <= cap) {
            std::printf("tail %d %llu %llu %llu -> %llu\n", dtype, (unsigned long long)d, (unsigned long long)cap,
                        (unsigned long long)first, (unsigned long long)tail_elems(dtype, cap, d, first));
            for (uint64_t count : {(uint64_t)0, (uint64_t)1, cap - first})
              if (first + count <= cap)
                std::printf("fill %d %llu %llu %llu -> %llu\n", dtype, (unsigned long long)cap, (unsigned long long)first,
                            (unsigned long long)count, (unsigned long long)fill_tail_elems(dtype, cap, first, count));
            std::printf("vacated %d %llu %llu %llu -> %llu\n", dtype, (unsigned long long)d, (unsigned long long)first,
                        (unsigned long long)cap, (unsigned long long)vacated_elems(dtype, d, first, cap));
          }
      }
  return 0;
}
