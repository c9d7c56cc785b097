// Prints the launch geometry of the search path over a grid of calls, one line per case; needs no
// device (an index whose device is -1 answers 256 compute units).  tests/test_search_geometry_cpu.py
// compares the output with tests/golden/search_geometry.txt, which was recorded from the code as it
// stood before the arithmetic moved into search_geometry.hpp.
#include "../../islands_amd/csrc/search_geometry.hpp"
#include <cstdio>

int main() {
  // ef straddles every threshold of the code: segments (64, 128, 256), visited-table bits (64, 160,
  // 320), the fast kernel's limit (512) and the device limit (4096)
  const uint32_t efs[] = {1, 10, 64, 65, 128, 160, 161, 256, 320, 321, 512, 513, 4096};
  // evaluations per query: unknown, below and above the default tables, the measured ones of the
  // comments in fast_geometry (1226, 3100-3400), one past the 4x cap
  const uint32_t hints[] = {0, 500, 1226, 3100, 3400, 9000, 40000};
  for (uint32_t ef : efs)
    for (uint32_t d : {100u, 128u, 768u, 4096u})
      for (uint32_t qb : {4u, 2u})
        for (uint32_t h : hints) {
          const FastGeom g = fast_geometry(ef, d, qb, h);
          printf("fast %u %u %u %u -> %u %zu %u\n", ef, d, qb, h, g.hbits, g.lds, g.hcap);
        }
  for (uint32_t ef : efs)
    for (uint32_t d : {8u, 100u, 128u, 384u, 768u, 1024u, 4096u}) {
      printf("aux %u %u -> %zu %u", ef, d, exact_lds(ef, d), push_log_cap(ef));
      for (uint32_t hbits : {9u, 13u})
        for (uint32_t wcap : {256u, 2624u})
          for (uint32_t qb : {4u, 2u}) printf(" %zu", two_level_lds(hbits, wcap, ef, d, qb));
      printf("\n");
    }
  isl_index* idx = new isl_index();
  idx->device = -1;
  idx->ncodes = 1000000;
  // plain, bf16 rows with a recorded evaluation count, recompute provider, two-level, two-level
  // retry (window_scale 4) over the recompute provider
  struct Variant { const char* name; int tl; bool bf16, recompute; };
  const Variant variants[] = {{"f32", 0, false, false}, {"bf16", 0, true, false}, {"rec", 0, false, true},
                              {"tl", 1, false, false}, {"tl4rec", 2, false, true}};
  for (uint32_t deg : {64u, 65u, 128u, 129u})
    for (uint32_t ef : efs)
      for (uint32_t d : {100u, 768u, 4096u})
        for (const Variant& v : variants) {
          idx->max_degree = deg;
          idx->rows.set_dtype(v.bf16 ? ISL_DTYPE_BF16 : ISL_DTYPE_F32);  // only the type matters: no block
          idx->recompute = v.recompute;
          idx->evals_hint.store(v.bf16 ? ((uint64_t)ef << 32) | 3100u : 0u);
          TwoLevelCall t{0.5f, v.tl == 2 ? 4u : 1u};
          CallGeometry cg;
          const isl_status st = call_geometry(idx, d, 10, ef, v.tl ? &t : nullptr, cg);
          printf("call %u %u %u %s -> %d", deg, ef, d, v.name, (int)st);
          if (st != ISL_OK) { printf("\n"); continue; }
          printf(" %u %d %u %u %zu %u %zu %u %u", cg.ef, (int)cg.use_fast, cg.slots, cg.tl_wcap, cg.tl_lds,
                 cg.tl_hbits_q, cg.tl_lds_q, cg.tl_slots_q, cg.plog_cap);
          printf(" | %u %u %zu %u", cg.vhint, cg.fg.hbits, cg.fg.lds, cg.fg.hcap);
          printf(" | %d %d %u %zu %u %u | %u %u %zu %zu\n", cg.segments, (int)cg.qh, cg.fgq.hbits, cg.fgq.lds,
                 cg.fgq.hcap, cg.slots_q, cg.state_words, cg.lane_slots, cg.exact_lds, cg.descent_lds);
        }
  return 0;
}
