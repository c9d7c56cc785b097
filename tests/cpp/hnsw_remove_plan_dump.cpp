// islands_amd/csrc/hnsw_remove_plan.hpp without a device or the library:
//   g++ -std=c++17 tests/cpp/hnsw_remove_plan_dump.cpp -o hnsw_remove_plan_dump
// stdin: n0, has_entry, entry, max_level, n_ids, then n0 levels and n_ids ids (all below n0).
// stdout: "len", "entry <has> <id> <max_level>", "layers <before> <after>", "members" (survivors per old layer),
// "capacity" (the bound on the touched list), then "pair <layer> <node> <packed> <layer back> <node back>" for a few
// pairs, "cap <layer> <m> <m0> <M_L>" and "lds <d> <m> <m0> <bytes>" (tests/test_hnsw_remove_cpu.py).
#include <cstdio>

#include "../../islands_amd/csrc/hnsw_remove_plan.hpp"

int main() {
  unsigned long long n0 = 0, entry = 0, max_level = 0, n_ids = 0;
  int has_entry = 0;
  if (std::scanf("%llu %d %llu %llu %llu", &n0, &has_entry, &entry, &max_level, &n_ids) != 5) return 2;
  std::vector<uint64_t> levels(n0), ids(n_ids);
  for (auto* vec : {&levels, &ids})
    for (auto& x : *vec) {
      unsigned long long t;
      if (std::scanf("%llu", &t) != 1) return 2;
      x = t;
    }
  std::vector<uint32_t> remap, survivors;
  const uint64_t n = isl_plan::build_remap(n0, ids.data(), ids.size(), remap, survivors);
  const isl_plan::Entry e = isl_plan::entry_after(levels, remap, survivors, has_entry != 0, entry, max_level);
  std::printf("len %llu\nentry %d %llu %llu\n", (unsigned long long)n, e.has ? 1 : 0, (unsigned long long)e.id,
              (unsigned long long)e.max_level);
  std::printf("layers %llu %llu\nmembers", max_level + 1, (unsigned long long)isl_plan::layers_after(e));
  const std::vector<uint64_t> members = isl_plan::layer_members(levels, survivors, max_level + 1);
  for (uint64_t m : members) std::printf(" %llu", (unsigned long long)m);
  std::printf("\ncapacity %llu\n", (unsigned long long)isl_plan::touched_capacity(members));
  for (unsigned layer : {0u, 1u, 5u, 63u})
    for (unsigned node : {0u, 7u, 0x7FFFFFEFu}) {
      const uint64_t p = isl_plan::touched_pair(layer, node);
      std::printf("pair %u %u %llu %u %u\n", layer, node, (unsigned long long)p, isl_plan::pair_layer(p),
                  isl_plan::pair_node(p));
    }
  for (unsigned layer : {0u, 1u, 9u}) std::printf("cap %u 4 8 %u\n", layer, isl_plan::layer_cap(layer, 4, 8));
  for (unsigned d : {3u, 24u, 768u})
    for (unsigned m : {4u, 64u, 128u})
      for (unsigned m0 : {8u, 128u})
        std::printf("lds %u %u %u %zu\n", d, m, m0, isl_plan::hnsw_repair_lds(16 * 80 * 4, d, m, m0));
  std::printf("max_layers %llu\n", (unsigned long long)isl_plan::kMaxLayers);
  return 0;
}
