// Host-only bookkeeping of the recompute provider's rounds (search_recompute.hip): how many queries are in
// flight at a time, which queries a round lists for the traversal kernel and which for the heap-exact kernel's
// queue, how fresh queries top a round up, when the batch is over.  Plain C++ without a device header, in the
// manner of build_plan.hpp: tests/cpp/recompute_plan_dump.cpp drives the scheduler over scripted statuses with
// g++ alone (tests/test_recompute_plan_cpu.py).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "query_status.hpp"

namespace isl_rounds __attribute__((visibility("hidden"))) {  // (inline code: not among the library's symbols)

// ---- the kind of a batch
// Searches park and resume: the wave-per-query traversal, the two-level search, and the heap-exact kernel
// (ef > 512, rows past 128 ids, tie hand-overs), whose parked queries keep their slot of the scratch pool
// across the rounds -- when the row cache is bounded.  With a row for every node nothing is ever evicted, a
// blocked query of that kernel simply starts over next round (all of them advance in parallel, where parked
// ones would advance 32 at a time: the pool's slots).
enum class Kind {
  RERUN,        // an ordinary launch over all queries every round, blocked queries start over
  PARK,         // the round's queries park in the traversal kernel (the two-level search included)
  EXACT_QUEUE,  // no traversal kernel in front: the round's queries are the heap-exact kernel's queue
};
// exact_parks: this call's queries park in the heap-exact kernel (not the two-level search; bounded row cache)
inline Kind batch_kind(bool two_level, bool use_fast, bool exact_parks) {
  return two_level || use_fast ? Kind::PARK : exact_parks ? Kind::EXACT_QUEUE : Kind::RERUN;
}

// ---- the caps
// Queries in flight at a time: each may hold one hop (<= 128 rows) waiting for its last rows, and
// those rows are exempt from eviction -- half the slab stays free for the rows being encoded, so
// every round serves every miss and every query in flight advances by a hop per round.  (2^20
// rows: 4096 queries; a smaller cache works through the batch a few queries at a time.)
// (A slab with a row for every node never evicts: no limit.)
// (a hop parked in the heap-exact kernel may hold a whole adjacency row of any length)
inline uint64_t hop_rows(bool two_level, uint64_t max_degree) {
  return 2 * std::max<uint64_t>(128, two_level ? 128 : max_degree);
}
inline uint32_t max_in_flight(uint64_t nq, uint64_t slab_rows, uint64_t nvec, bool two_level, uint64_t max_degree) {
  return slab_rows < nvec ? (uint32_t)std::max<uint64_t>(1, slab_rows / hop_rows(two_level, max_degree)) : (uint32_t)nq;
}
// Every query in flight advances by at least one hop per round, and a query makes at most a few
// times ef hops with new rows: the cap scales with the number of groups the batch is worked
// through in, so a 256-row cache (one query at a time) is not cut short and a bug still ends.
inline uint64_t max_rounds(uint64_t nq, uint32_t in_flight, uint64_t ef) {
  return 64 + ((nq + in_flight - 1) / in_flight) * ((uint64_t)64 * ef + 4096);
}
// ids a round may report missing: a hop keeps up to 128 rows
inline uint64_t miss_capacity(uint64_t nq) { return std::min<uint64_t>(nq * 128 + 64, 0xFFFFFFF0ull); }
// ... + the ids parked two-level queries expect to promote next (behind miss[miss_capacity])
inline uint64_t prefetch_capacity(uint64_t nq) { return nq * 8 + 64; }
// Rounds in a row that place no row although rows are missing (every slot is held by a hop of the round)
// before the batch fails.  A batch that parks cannot get there (half the slab stays free by construction); a
// batch that re-runs its blocked queries from their start needs their whole traversal resident and never
// will be.
inline uint32_t stall_limit(Kind kind) { return kind == Kind::RERUN ? 1u : 3u; }

// ---- the window step of the two-level search
// A query whose approximate queue outgrew the LDS window is never answered differently: the queries it
// happened to are run again with a window four times the size, up to 64 times the first.
inline bool grow_window(uint32_t& window_scale) {
  if (window_scale >= 64) return false;
  window_scale *= 4;
  return true;
}

// ---- the rounds
enum class Verdict {
  LAUNCH,         // run the round: active() queries of qlist, exact() queries of xlist
  FINAL,          // nothing listed: the statuses are final
  SHORT_WINDOWS,  // two-level search, nothing parked: hand the short-window queries over (restart_short)
};

// Which queries each round of a batch of nq runs, at most `in_flight` of them.  The lists are written into
// the caller's arrays of nq words each (the lane's pinned host lists).
class RoundScheduler {
 public:
  RoundScheduler(Kind kind, bool two_level, uint32_t nq, uint32_t in_flight, uint32_t* qlist, uint32_t* xlist)
      : kind_(kind), two_level_(two_level), nq_(nq), cap_(in_flight), qlist_(qlist), xlist_(xlist) {}

  uint32_t active() const { return active_; }  // queries of qlist for the traversal kernel
  uint32_t exact() const { return nxl_; }      // queries of xlist that go straight to the heap-exact kernel's queue
  bool listed() const { return listed_; }      // false: the round runs queries [0, active()) and reads no list

  // the first round (always launched)
  void first() {
    active_ = std::min(nq_, cap_);
    next_fresh_ = active_;
    nxl_ = 0;
    listed_ = active_ < nq_;
    if (kind_ == Kind::RERUN) {
      active_ = 0;  // an ordinary launch over all queries every round
      listed_ = false;
    } else if (kind_ == Kind::EXACT_QUEUE) {
      for (uint32_t i = 0; i < active_; ++i) xlist_[i] = i;
      nxl_ = active_;
      active_ = 0;
      listed_ = true;
    } else if (listed_) {
      for (uint32_t i = 0; i < active_; ++i) qlist_[i] = i;
    }
  }

  // The next round, from the statuses of the finished one (status[i] of every query started so far; `misses` ids
  // were reported missing): the queries that are waiting for rows, topped up with fresh ones.  A batch that
  // re-runs goes by the misses alone.
  Verdict next(const uint32_t* status, uint32_t misses) {
    if (kind_ == Kind::RERUN) return misses ? Verdict::LAUNCH : Verdict::FINAL;
    const bool to_queue = kind_ == Kind::EXACT_QUEUE;
    uint32_t na = 0;
    nxl_ = 0;
    // queries parked in the heap-exact kernel go straight back to its queue (in front: they hold slots);
    // the others that wait for rows go through the traversal kernel again -- or, when there is none in
    // front (ef > 512, long rows), to that queue as well
    for (uint32_t i = 0; i < next_fresh_; ++i)
      if (status[i] == QS_BLOCKED_X) xlist_[nxl_++] = i;
    for (uint32_t i = 0; i < next_fresh_; ++i)
      if (status[i] == QS_BLOCKED) {
        if (to_queue) xlist_[nxl_++] = i;
        else qlist_[na++] = i;
      }
    while (na + nxl_ < cap_ && !again_.empty()) { qlist_[na++] = again_.back(); again_.pop_back(); }
    while (na + nxl_ < cap_ && next_fresh_ < nq_) {
      if (to_queue) xlist_[nxl_++] = next_fresh_++;
      else qlist_[na++] = next_fresh_++;
    }
    active_ = na;
    listed_ = true;
    if (!na && two_level_) return Verdict::SHORT_WINDOWS;
    return na || nxl_ ? Verdict::LAUNCH : Verdict::FINAL;
  }

  // After SHORT_WINDOWS: every query has run to its end; the `nshort` of qlist[0, nshort) whose queue window
  // was too small start over -- alone, nothing is parked now (0: none, or the window cannot grow).
  Verdict restart_short(uint32_t nshort) {
    again_.assign(qlist_, qlist_ + nshort);
    uint32_t na = 0;
    while (na < cap_ && !again_.empty()) { qlist_[na++] = again_.back(); again_.pop_back(); }
    active_ = na;
    return na || nxl_ ? Verdict::LAUNCH : Verdict::FINAL;
  }

 private:
  const Kind kind_;
  const bool two_level_;
  const uint32_t nq_, cap_;
  uint32_t* const qlist_;
  uint32_t* const xlist_;
  uint32_t active_ = 0;
  uint32_t nxl_ = 0;         // queries this round hands straight to the heap-exact kernel
  uint32_t next_fresh_ = 0;  // queries [next_fresh_, nq) have not been started
  bool listed_ = false;
  std::vector<uint32_t> again_;  // two-level search: queries to start over with a larger queue window
};

}  // namespace isl_rounds
