// Host-only arithmetic of isl_index_remove (build.hip): the remap of the surviving ids, the entry-point rule,
// the bound on a candidate list and the LDS of the repair kernel.  Plain C++ without a device header, in the
// manner of build_plan.hpp: tests/cpp/remove_plan_dump.cpp prints it with g++ alone
// (tests/test_index_remove_cpu.py).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "build_plan.hpp"

namespace isl_plan {

// ISL_REMOVE_MAX_CANDIDATES: C(p) is cut after this many distinct ids -- the builder's bound on a candidate
// list, whose lists live in LDS
constexpr uint32_t kRemoveMaxCandidates = (uint32_t)kMaxEfConstruction;
// a removed id in the 32-bit remap the kernels read (ids stay below kMaxNodes)
constexpr uint32_t kGone = 0xFFFFFFFFu;

// the most ids the walk of one list can emit before C(p) is deduplicated: its own m0 ids, or the m0 ids of each
constexpr uint64_t worst_emission(uint64_t m0) { return m0 + m0 * m0; }

// the first id of `ids` that is not below n0 (false: there is none)
inline bool first_unknown_id(const uint64_t* ids, uint64_t n_ids, uint64_t n0, uint64_t* bad) {
  for (uint64_t i = 0; i < n_ids; ++i)
    if (ids[i] >= n0) { *bad = ids[i]; return true; }
  return false;
}

// remap[old] = the new id (old minus the removed ids below it) or kGone; survivors[new] = old.  Every id of
// `ids` is below n0; repeated ids count once.  Returns the new len.
inline uint64_t build_remap(uint64_t n0, const uint64_t* ids, uint64_t n_ids, std::vector<uint32_t>& remap,
                            std::vector<uint32_t>& survivors) {
  remap.assign(n0, 0u);
  for (uint64_t i = 0; i < n_ids; ++i) remap[ids[i]] = kGone;
  survivors.clear();
  for (uint64_t p = 0; p < n0; ++p)
    if (remap[p] != kGone) {
      remap[p] = (uint32_t)survivors.size();
      survivors.push_back((uint32_t)p);
    }
  return survivors.size();
}

// Entry point of the shrunk graph.  A surviving entry point is kept (remapped) and max_level stays; otherwise
// the lowest new id among the survivors of the highest level takes over and max_level is that level -- what
// LeannIndex::build leaves for those nodes (leann.rs:610-613: a later node replaces the entry point only with a
// HIGHER level).  `levels`: of all old nodes, or empty (all 0).  No survivor, or an index without entry point:
// none.
struct Entry {
  bool has;
  uint64_t id, max_level;
};
inline Entry entry_after(const std::vector<uint64_t>& levels, const std::vector<uint32_t>& remap,
                         const std::vector<uint32_t>& survivors, bool has_entry, uint64_t entry, uint64_t max_level) {
  if (!has_entry || survivors.empty()) return Entry{false, 0, survivors.empty() ? 0 : max_level};
  if (entry < remap.size() && remap[entry] != kGone) return Entry{true, remap[entry], max_level};
  Entry e{true, 0, levels.empty() ? 0 : levels[survivors[0]]};
  for (uint64_t i = 1; i < survivors.size(); ++i) {
    const uint64_t lv = levels.empty() ? 0 : levels[survivors[i]];
    if (lv > e.max_level) { e.id = i; e.max_level = lv; }
  }
  return e;
}

// levels of the survivors in their order (`levels` of all old nodes, or empty = all 0)
inline std::vector<uint64_t> levels_after(const std::vector<uint64_t>& levels, const std::vector<uint32_t>& survivors) {
  std::vector<uint64_t> out(survivors.size(), 0);
  if (!levels.empty())
    for (uint64_t i = 0; i < survivors.size(); ++i) out[i] = levels[survivors[i]];
  return out;
}

// LDS of the repair kernel: a selection over up to kRemoveMaxCandidates candidates into a row of m0 (the raw
// ids and distances wait in the two lists the selection initialises itself, as in isl_select_neighbors)
constexpr size_t repair_lds(size_t tile_bytes, uint32_t d, uint32_t m0) {
  return select_lds(tile_bytes, d, kRemoveMaxCandidates, m0);
}
constexpr size_t repair_lds_bf16(uint32_t d, uint32_t m0) { return select_lds_bf16(d, kRemoveMaxCandidates, m0); }

}  // namespace isl_plan
