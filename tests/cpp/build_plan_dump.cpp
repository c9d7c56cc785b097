// The builders' step planner (islands_amd/csrc/build_plan.hpp) without a device or the library:
//   g++ -std=c++17 tests/cpp/build_plan_dump.cpp -o build_plan_dump
// stdin: batch, n, then n levels.  stdout: one line "step <first> <count> <top>" per step, then
// "order" followed by the n node ids in insertion order.  tests/test_hnsw_build_cpu.py compares the
// steps with the tests' own planner and checks the order inside every step.
#include <cstdio>

#include "../../islands_amd/csrc/build_plan.hpp"

int main() {
  unsigned long long batch = 0, n = 0;
  if (std::scanf("%llu %llu", &batch, &n) != 2) return 2;
  std::vector<uint32_t> lv(n);
  for (auto& x : lv)
    if (std::scanf("%u", &x) != 1) return 2;
  std::vector<isl_plan::Step> steps;
  std::vector<uint32_t> order;
  isl_plan::plan_steps(lv, batch, steps, order);
  for (const isl_plan::Step& s : steps) std::printf("step %llu %u %u\n", (unsigned long long)s.first, s.count, s.top);
  std::printf("order");
  for (uint32_t id : order) std::printf(" %u", id);
  std::printf("\nlargest %llu\n", (unsigned long long)isl_plan::largest_step(steps));
  return 0;
}
