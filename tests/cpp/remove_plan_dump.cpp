// islands_amd/csrc/remove_plan.hpp without a device or the library:
//   g++ -std=c++17 tests/cpp/remove_plan_dump.cpp -o remove_plan_dump
// stdin: n0, has_entry, entry, max_level, with_levels, n_ids, then n0 levels (if with_levels) and n_ids ids.
// stdout: "unknown <id>" and nothing else when an id is not below n0; otherwise "len", "remap" (-1 = removed),
// "survivors", "entry <has> <id> <max_level>", "levels", then the constants and LDS figures the kernels are
// launched with: "cap", "worst <m0> <ids>", "lds <f32|bf16> <d> <m0> <bytes>" (tests/test_index_remove_cpu.py).
#include <cstdio>

#include "../../islands_amd/csrc/remove_plan.hpp"

int main() {
  unsigned long long n0 = 0, entry = 0, max_level = 0, n_ids = 0;
  int has_entry = 0, with_levels = 0;
  if (std::scanf("%llu %d %llu %llu %d %llu", &n0, &has_entry, &entry, &max_level, &with_levels, &n_ids) != 6) return 2;
  std::vector<uint64_t> levels(with_levels ? n0 : 0), ids(n_ids);
  for (auto& x : levels) {
    unsigned long long t;
    if (std::scanf("%llu", &t) != 1) return 2;
    x = t;
  }
  for (auto& x : ids) {
    unsigned long long t;
    if (std::scanf("%llu", &t) != 1) return 2;
    x = t;
  }
  uint64_t bad = 0;
  if (isl_plan::first_unknown_id(ids.data(), ids.size(), n0, &bad)) {
    std::printf("unknown %llu\n", (unsigned long long)bad);
    return 0;
  }
  std::vector<uint32_t> remap, survivors;
  const uint64_t n = isl_plan::build_remap(n0, ids.data(), ids.size(), remap, survivors);
  std::printf("len %llu\nremap", (unsigned long long)n);
  for (uint32_t r : remap) std::printf(" %lld", r == isl_plan::kGone ? -1ll : (long long)r);
  std::printf("\nsurvivors");
  for (uint32_t s : survivors) std::printf(" %u", s);
  const isl_plan::Entry e = isl_plan::entry_after(levels, remap, survivors, has_entry != 0, entry, max_level);
  std::printf("\nentry %d %llu %llu\nlevels", e.has ? 1 : 0, (unsigned long long)e.id, (unsigned long long)e.max_level);
  for (uint64_t l : isl_plan::levels_after(levels, survivors)) std::printf(" %llu", (unsigned long long)l);
  std::printf("\ncap %u\n", isl_plan::kRemoveMaxCandidates);
  for (unsigned m0 : {8u, 64u, 96u, 128u}) std::printf("worst %u %llu\n", m0, (unsigned long long)isl_plan::worst_emission(m0));
  for (unsigned d : {3u, 16u, 100u, 768u})
    for (unsigned m0 : {8u, 128u}) {
      std::printf("lds f32 %u %u %zu\n", d, m0, isl_plan::repair_lds(16 * 80 * 4, d, m0));
      std::printf("lds bf16 %u %u %zu\n", d, m0, isl_plan::repair_lds_bf16(d, m0));
    }
  return 0;
}
