// Host-only arithmetic of the reachability report and the covering entry seeds (graph_reach.hip): the check of a
// caller's source list, how one level of the walk is cut into workgroups, and the bookkeeping of the cover loop.
// Plain C++ without a device header, in the manner of entry_seeds_plan.hpp: tests/cpp/graph_reach_plan_dump.cpp
// prints it with g++ alone (tests/test_graph_reach_cpu.py compares with a Python restatement).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/islands_amd.h"

namespace isl_reach {

// ---- sources
// the level of node v where `levels` holds nlevels of them (a handle without levels: every node on layer 0 only)
inline uint64_t level_of(const uint64_t* levels, uint64_t nlevels, uint64_t v) { return v < nlevels ? levels[v] : 0; }

// A caller's source list against a graph of `len` nodes whose population is the nodes of level >= layer: ISL_OK, or
// ISL_ERR_NODE_NOT_FOUND with *bad = the first id that is >= len or not on the layer.  *distinct = the number of
// different ids (repeats are accepted); out32 (may be NULL) receives the list as the device reads it.
inline isl_status check_sources(const uint64_t* src, uint64_t count, uint64_t len, const uint64_t* levels,
                                uint64_t nlevels, uint64_t layer, uint64_t* bad, uint64_t* distinct,
                                std::vector<uint32_t>* out32) {
  *bad = 0;
  *distinct = 0;
  if (out32) out32->clear();
  for (uint64_t i = 0; i < count; ++i)
    if (src[i] >= len || level_of(levels, nlevels, src[i]) < layer) {
      *bad = src[i];
      return ISL_ERR_NODE_NOT_FOUND;
    }
  std::vector<uint64_t> s(src, src + count);
  std::sort(s.begin(), s.end());
  *distinct = (uint64_t)(std::unique(s.begin(), s.end()) - s.begin());
  if (out32) out32->assign(src, src + count);  // (ids < len < 2^31: checked above)
  return ISL_OK;
}

// ---- launch geometry
constexpr uint32_t kBlock = 256;          // four waves
constexpr uint32_t kWavesPerBlock = kBlock / 64;
constexpr uint32_t kBlocksPerCu = 8;      // 32 waves per CU: the walk waits on memory, not on registers
constexpr uint64_t kScanWindow = 1ull << 20;  // ids one "smallest unreached id" launch looks at

// Workgroups of the expand kernel for a frontier of `frontier` nodes: a wave per node until the card is full,
// then every wave strides over the frontier.
inline uint32_t expand_blocks(uint64_t frontier, uint32_t cus) {
  const uint64_t want = (frontier + kWavesPerBlock - 1) / kWavesPerBlock;
  const uint64_t cap = (uint64_t)(cus ? cus : 1u) * kBlocksPerCu;
  return (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
}
// ... and of the kernels with one thread per element (init, in-degree, reduction, scan): grid-striding
inline uint32_t stream_blocks(uint64_t elements, uint32_t cus) {
  const uint64_t want = (elements + kBlock - 1) / kBlock;
  const uint64_t cap = (uint64_t)(cus ? cus : 1u) * kBlocksPerCu;
  return (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
}

// ---- the cover loop (isl_index_cover_entry_seeds)
//   S = the current table, or [entry_point];  R = reachable from S
//   while R != all nodes and |S| < max_seeds:  j = the smallest id not in R;  S += [j];  R |= reachable from j
// The device does the walks and finds j; this keeps S, the cursor and the decisions.
struct CoverLoop {
  std::vector<uint64_t> seeds;  // S
  uint64_t initial = 0;         // |S| before the loop
  uint64_t max_seeds = 0, len = 0;
  uint64_t cursor = 0;          // every id below it is reached: j is looked for at or after it, it only moves forward
  uint64_t scans = 0;           // "smallest unreached id" launches so far

  void start(const uint64_t* table, uint64_t table_count, uint64_t entry_point, uint64_t max_seeds_, uint64_t len_) {
    seeds.assign(table, table + table_count);
    if (seeds.empty()) seeds.push_back(entry_point);
    initial = seeds.size();
    max_seeds = max_seeds_;
    len = len_;
    cursor = 0;
    scans = 0;
  }
  // after a walk that left `reached` nodes reached: is another seed to be looked for?
  bool wants_seed(uint64_t reached) const { return reached < len && seeds.size() < max_seeds; }
  // the window [first, first + count) the next scan looks at (count 0: nothing left to look at)
  void next_window(uint64_t* first, uint64_t* count) const {
    *first = cursor;
    *count = cursor < len ? std::min(kScanWindow, len - cursor) : 0;
  }
  // what the scan of that window answered (found == 0xFFFFFFFF: none in it).  true: `found` joins S and is walked
  // from; false: the window held none, look at the next one.
  bool take_scan(uint32_t found) {
    ++scans;
    uint64_t first, count;
    next_window(&first, &count);
    if (found == 0xFFFFFFFFu || found < first || found >= first + count) {
      cursor = first + count;
      return false;
    }
    seeds.push_back(found);
    cursor = (uint64_t)found + 1;
    return true;
  }
  uint64_t added() const { return seeds.size() - initial; }
  // the table is installed only when the loop added an id: an index without a table that needs none keeps none
  bool installs() const { return added() > 0; }
  uint64_t unreached(uint64_t reached) const { return len - reached; }
};

}  // namespace isl_reach
