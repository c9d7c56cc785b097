// Host-only arithmetic of the in-place row compaction of isl_index_remove on a reserved index (build.hip): the
// order in which the survivors' rows move down inside the one block that holds them.  Plain C++ without a device
// header, in the manner of remove_plan.hpp: tests/cpp/row_compact_plan_dump.cpp prints it with g++ alone
// (tests/test_row_compact_plan_cpu.py replays the plan on a numpy array).
//
// New row j takes old row s[j], s the ascending survivor list, so s[j] >= j and j - s[j] never grows.  Slot j is
// the source of an earlier new row j' <= j: a destination may only be written once the row that lives there has
// been read.  The plan is a list of moves over ascending new ids, each one or two stream-ordered launches:
//   direct   s[first_new] >= first_new + count: every source of the move lies behind every destination of it, one
//            launch copies block -> block;
//   staged   the sources are gathered into a staging buffer, then written to their destinations.
// A move never needs a later move's destinations (later sources are >= their own new id, which is >= every earlier
// destination), and a later move's sources are not written by an earlier one (they lie at or behind its own first
// new id).  Rows below the first removed id do not move and are in no move.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace isl_plan {

constexpr uint64_t kCompactStageBytes = 64ull << 20;  // the staging buffer, at least one row

struct RowMove {
  uint64_t first_new, count;  // new rows [first_new, first_new + count)
  bool staged;
};

// Rows per staged move for rows of `row_bytes` (the stride in bytes plus the norm): the default buffer, or what
// ISL_COMPACT_STAGE_ROWS says (tests reach the chunk edges at small n with it); never more than the n rows there are.
inline uint64_t compact_stage_rows(uint64_t row_bytes, uint64_t n, const char* env) {
  uint64_t rows = std::max<uint64_t>(1, kCompactStageBytes / std::max<uint64_t>(1, row_bytes));
  if (env && *env) {
    const long long v = atoll(env);
    if (v > 0) rows = (uint64_t)v;
  }
  return std::max<uint64_t>(1, std::min(rows, std::max<uint64_t>(1, n)));
}

// the first new id whose row moves (n: none does)
inline uint64_t first_moved(const uint32_t* s, uint64_t n) {
  uint64_t j = 0;
  while (j < n && s[j] == j) ++j;
  return j;
}

// The moves of survivors s[0 .. n), stage_rows >= 1.  A direct move takes the whole gap s[j] - j; it is chosen where
// that is at least what a staged move would take, so that a small gap near the start of a large table costs two
// launches per stage_rows rows and not one per row.
inline void plan_row_moves(const uint32_t* s, uint64_t n, uint64_t stage_rows, std::vector<RowMove>& out) {
  out.clear();
  stage_rows = std::max<uint64_t>(1, stage_rows);
  for (uint64_t j = first_moved(s, n); j < n;) {
    const uint64_t left = n - j, direct = std::min<uint64_t>((uint64_t)s[j] - j, left);
    const uint64_t staged = std::min(stage_rows, left);
    const bool is_direct = direct >= staged;
    const uint64_t count = is_direct ? direct : staged;
    out.push_back(RowMove{j, count, !is_direct});
    j += count;
  }
}

}  // namespace isl_plan
