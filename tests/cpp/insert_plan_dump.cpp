// plan_steps_from of islands_amd/csrc/build_plan.hpp without a device or the library:
//   g++ -std=c++17 tests/cpp/insert_plan_dump.cpp -o insert_plan_dump
// stdin: batch, n0, max_level0, n, then n levels.  stdout: one line "step <first> <count> <top>" per step,
// then "order" followed by the n node ids in insertion order (tests/test_hnsw_insert_cpu.py).
#include <cstdio>

#include "../../islands_amd/csrc/build_plan.hpp"

int main() {
  unsigned long long batch = 0, n0 = 0, n = 0;
  unsigned max_level0 = 0;
  if (std::scanf("%llu %llu %u %llu", &batch, &n0, &max_level0, &n) != 4) return 2;
  std::vector<uint32_t> lv(n);
  for (auto& x : lv)
    if (std::scanf("%u", &x) != 1) return 2;
  std::vector<isl_plan::Step> steps;
  std::vector<uint32_t> order;
  isl_plan::plan_steps_from(lv, n0, max_level0, batch, steps, order);
  for (const isl_plan::Step& s : steps) std::printf("step %llu %u %u\n", (unsigned long long)s.first, s.count, s.top);
  std::printf("order");
  for (uint32_t id : order) std::printf(" %u", id);
  std::printf("\n");
  return 0;
}
