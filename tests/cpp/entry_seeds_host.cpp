// islands_amd/csrc/entry_seeds_plan.hpp on the host, under AddressSanitizer: the ISL_ENTRY_SEEDS variable,
// the check of a caller's seed list (exactly-sized heap arrays, so that a read past `count` is reported) and
// the grid of one pick launch over a sweep of call shapes (every seed tile covered once, no empty range).
// Built by `make -C islands_amd/csrc ../lib/asan/entry_seeds_host`; stand-alone, no device is touched.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../islands_amd/csrc/entry_seeds_plan.hpp"

static int failures = 0;
#define EXPECT(c)                                                   \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      ++failures;                                                   \
    }                                                               \
  } while (0)

int main() {
  using namespace isl_seeds;
  uint64_t n = 99;
  EXPECT(parse_seed_env(nullptr, &n) == ISL_OK && n == 0);
  EXPECT(parse_seed_env("", &n) == ISL_OK && n == 0);
  EXPECT(parse_seed_env("0", &n) == ISL_OK && n == 0);
  EXPECT(parse_seed_env("000", &n) == ISL_OK && n == 0);
  EXPECT(parse_seed_env("16", &n) == ISL_OK && n == 16);
  EXPECT(parse_seed_env("65536", &n) == ISL_OK && n == 65536);
  EXPECT(parse_seed_env("65537", &n) == ISL_ERR_UNSUPPORTED && n == 0);
  EXPECT(parse_seed_env("99999999999999999999999999999999", &n) == ISL_ERR_UNSUPPORTED && n == 0);
  for (const char* bad : {"-1", "+4", " 4", "4 ", "1e3", "0x10", "four", "4,5"})
    EXPECT(parse_seed_env(bad, &n) == ISL_ERR_INVALID_ARGUMENT && n == 0);
  {
    // a heap copy without the terminator's neighbour: the parser must stop at the NUL
    std::string s = "1024";
    char* heap = static_cast<char*>(std::malloc(s.size() + 1));
    for (size_t i = 0; i <= s.size(); ++i) heap[i] = s.c_str()[i];
    EXPECT(parse_seed_env(heap, &n) == ISL_OK && n == 1024);
    std::free(heap);
  }

  uint64_t bad = 7;
  EXPECT(check_seed_ids(nullptr, 0, 10, 10, &bad) == ISL_OK);
  EXPECT(check_seed_ids(nullptr, 3, 10, 10, &bad) == ISL_ERR_INVALID_ARGUMENT);
  EXPECT(check_seed_ids(nullptr, ISL_MAX_ENTRY_SEEDS + 1, 10, 10, &bad) == ISL_ERR_UNSUPPORTED);
  for (uint64_t count : {1ull, 2ull, 17ull, 1000ull}) {
    std::vector<uint64_t> ids(count);
    for (uint64_t i = 0; i < count; ++i) ids[i] = (i * 7) % 10;  // repeats are fine
    EXPECT(check_seed_ids(ids.data(), count, 10, 10, &bad) == ISL_OK && bad == 0);
    ids[count - 1] = 10;
    EXPECT(check_seed_ids(ids.data(), count, 10, 10, &bad) == ISL_ERR_NODE_NOT_FOUND && bad == 10);
    ids[count - 1] = 8;  // a node of the graph without a row
    EXPECT(check_seed_ids(ids.data(), count, 10, 8, &bad) == ISL_ERR_NODE_NOT_FOUND && bad == 8);
    ids[0] = ~0ull;
    EXPECT(check_seed_ids(ids.data(), count, 10, 10, &bad) == ISL_ERR_NODE_NOT_FOUND && bad == ~0ull);
  }
  {
    std::vector<uint64_t> full(ISL_MAX_ENTRY_SEEDS, 3);
    EXPECT(check_seed_ids(full.data(), full.size(), 4, 4, &bad) == ISL_OK);
  }

  for (uint64_t nq : {1ull, 17ull, 32ull, 33ull, 257ull, 1024ull, 100000ull, 0x7FFFFFFFull})
    for (uint64_t seeds : {1ull, 15ull, 17ull, 32ull, 33ull, 65ull, 257ull, 1024ull, 4096ull, 65536ull})
      for (uint32_t cus : {0u, 1u, 64u, 256u, 304u}) {
        const PickGrid g = pick_grid(nq, seeds, cus);
        const uint64_t stiles = (seeds + PST - 1) / PST;
        EXPECT(g.qtiles == (nq + PQT - 1) / PQT);
        EXPECT(g.splits >= 1 && g.splits <= 65535 && g.tiles_per_split >= 1);
        EXPECT((uint64_t)g.splits * g.tiles_per_split >= stiles);                  // every tile is in a range
        EXPECT((uint64_t)(g.splits - 1) * g.tiles_per_split < stiles);             // and no range is empty
      }
  EXPECT(PLD % 4 == 0 && PLD > PDC);

  if (failures) return 1;
  std::printf("entry seeds host: ok\n");
  return 0;
}
