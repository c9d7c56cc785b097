// Prints the answers of islands_amd/csrc/graph_reach_plan.hpp; plain C++, no device.  tests/test_graph_reach_cpu.py
// compares them with a Python restatement, once from a plain build and once from a stand-alone build under
// -fsanitize=address,undefined.
// stdin:
//   <len> <layer> <nlevels> then the levels, <count> then the sources
//   <table_count> then the table, <entry_point> <max_seeds> <cover_len> <steps>, <reached> after the walk from the
//     initial S, then per step "<found> <reached>": what the scan of the loop's next window answers (4294967295:
//     none in it) and how many nodes are reached after the walk that follows it (used only when the answer joins S)
// stdout:
//   sources <status> <bad> <distinct> [the list as u32]
//   expand <frontier> <cus> -> <blocks>      stream <elements> <cus> -> <blocks>
//   cover start <initial> wants <0|1>
//   window <first> <count>                   take <0|1> cursor <cursor> seeds <|S|> wants <0|1>
//   cover end added <k> installs <0|1> unreached <u> scans <s> seeds <ids...>
#include "../../islands_amd/csrc/graph_reach_plan.hpp"

#include <cstdio>
#include <vector>

static bool read_u64(unsigned long long* v) { return std::scanf("%llu", v) == 1; }

int main() {
  unsigned long long len = 0, layer = 0, nlevels = 0, count = 0, v = 0;
  if (!read_u64(&len) || !read_u64(&layer) || !read_u64(&nlevels)) return 2;
  std::vector<uint64_t> levels(nlevels);
  for (auto& x : levels) {
    if (!read_u64(&v)) return 2;
    x = v;
  }
  if (!read_u64(&count)) return 2;
  std::vector<uint64_t> src(count);
  for (auto& x : src) {
    if (!read_u64(&v)) return 2;
    x = v;
  }
  uint64_t bad = 0, distinct = 0;
  std::vector<uint32_t> out32;
  const isl_status st = isl_reach::check_sources(src.data(), count, len, nlevels ? levels.data() : nullptr, nlevels,
                                                 layer, &bad, &distinct, &out32);
  std::printf("sources %d %llu %llu", (int)st, (unsigned long long)bad, (unsigned long long)distinct);
  for (uint32_t s : out32) std::printf(" %u", s);
  std::printf("\n");

  for (uint32_t cus : {0u, 1u, 64u, 256u})
    for (uint64_t f : {0ull, 1ull, 3ull, 4ull, 5ull, 2047ull, 8192ull, 8193ull, 1000000ull, 1ull << 31}) {
      std::printf("expand %llu %u -> %u\n", (unsigned long long)f, cus, isl_reach::expand_blocks(f, cus));
      std::printf("stream %llu %u -> %u\n", (unsigned long long)f, cus, isl_reach::stream_blocks(f, cus));
    }

  unsigned long long tcount = 0, entry = 0, max_seeds = 0, clen = 0, steps = 0;
  if (!read_u64(&tcount)) return 2;
  std::vector<uint64_t> table(tcount);
  for (auto& x : table) {
    if (!read_u64(&v)) return 2;
    x = v;
  }
  if (!read_u64(&entry) || !read_u64(&max_seeds) || !read_u64(&clen) || !read_u64(&steps)) return 2;
  unsigned long long reached = 0;
  if (!read_u64(&reached)) return 2;  // after the walk from the initial S
  isl_reach::CoverLoop loop;
  loop.start(table.data(), tcount, entry, max_seeds, clen);
  std::printf("cover start %llu wants %d\n", (unsigned long long)loop.initial, loop.wants_seed(reached) ? 1 : 0);
  for (unsigned long long i = 0; i < steps && loop.wants_seed(reached); ++i) {
    unsigned long long found = 0, after = 0;
    if (!read_u64(&found) || !read_u64(&after)) return 2;
    uint64_t first = 0, cnt = 0;
    loop.next_window(&first, &cnt);
    std::printf("window %llu %llu\n", (unsigned long long)first, (unsigned long long)cnt);
    if (!cnt) break;
    const bool took = loop.take_scan((uint32_t)found);
    if (took) reached = after;
    std::printf("take %d cursor %llu seeds %llu wants %d\n", took ? 1 : 0, (unsigned long long)loop.cursor,
                (unsigned long long)loop.seeds.size(), loop.wants_seed(reached) ? 1 : 0);
  }
  std::printf("cover end added %llu installs %d unreached %llu scans %llu seeds", (unsigned long long)loop.added(),
              loop.installs() ? 1 : 0, (unsigned long long)loop.unreached(reached), (unsigned long long)loop.scans);
  for (uint64_t s : loop.seeds) std::printf(" %llu", (unsigned long long)s);
  std::printf("\n");
  return 0;
}
