// What the host units of the search path share: search.hip (lanes, parameter fill, the one loop that issues
// launches, entry points), search_group.hip (grouped launches) and search_recompute.hip (the recompute provider's
// row cache, rounds and coalescer).  Declarations only; the symbols stay inside the library.
// What one enqueue launches -- which kernels, in what order, with what grid, LDS, instantiation and told nq, for a
// SearchCall, a RoundPlan and the warm flag -- is decided in search_launch_plan.hpp (plan_launches), not here and
// not in search.hip.
#pragma once

#include "common.hpp"

namespace isl_lane __attribute__((visibility("hidden"))) {

// Stream a call runs on.  OWN: the lane's non-blocking stream (host-pointer entry point).
// USER: the caller's stream (NULL = legacy default stream, ordered after the caller's earlier
// work on it, e.g. torch kernels that produced the queries).  OWN_AFTER_USER: the lane's stream,
// made to wait for everything already enqueued on the caller's stream -- lets several searches
// overlap (asynchronous entry point).  OWN_AFTER_EVENT: the same, with the lane's ev_in already recorded on the
// caller's stream (a call the group path held back: ordered after the caller's stream as of its arrival).
enum class StreamMode { OWN, USER, OWN_AFTER_USER, OWN_AFTER_EVENT };

// One search as its entry point received it; every pointer is a device pointer.
struct SearchCall {
  const float* queries = nullptr;
  uint64_t nq = 0, d = 0, k = 0, ef = 0;
  uint64_t* ids = nullptr;
  float* dist = nullptr;
  uint32_t* count = nullptr;
  hipStream_t user_stream = nullptr;
  StreamMode mode = StreamMode::OWN;
  bool two_level = false;  // the two-level search with a PQ filter, re-ranking `ratio` of the approximate queue
  float ratio = 0.0f;
};
inline hipStream_t call_stream(const isl::SearchWorkspace& ws, const SearchCall& c) {
  return c.mode == StreamMode::USER ? c.user_stream : ws.stream;
}

// What search_sync asks of one enqueue beyond the call itself; the default is an ordinary launch
// over all queries (asynchronous entry points, warm launches).
struct RoundPlan {
  // a round of the recompute provider: the RESUME kernel over `active` queries, listed in ws.qlist
  // unless it is the first round (`listed`); `exact` queries of ws.h_xlist go straight to the
  // heap-exact kernel's queue
  uint32_t active = 0;
  uint32_t exact = 0;
  bool exact_parks = false;   // this call's queries park in the heap-exact kernel (bounded row cache)
  bool listed = false;
  uint32_t prefetch = 0;      // two-level search: ids a parked query names beyond its misses (0 = none)
  // two-level search: `retry` queries (listed in ws.qlist) re-run alone with a queue window grown
  // by `window_scale`; the PQ distance tables of the call's first launch stay
  uint32_t retry = 0;
  uint32_t window_scale = 1;
  bool tables_built = false;
};

// ---- search.hip
isl_status ensure_lane_stream(const isl_index* idx, isl::SearchWorkspace& ws);
isl_status ensure_pool(const isl_index* idx, isl::SearchWorkspace& ws);  // (under idx->mu)
// dst[0, n) = src[0, n) on `st` (copy_u32_kernel on grid x block threads; either side may be pinned host memory)
void copy_words(const uint32_t* src, uint32_t* dst, uint64_t n, uint32_t grid, uint32_t block, hipStream_t st);
// streams, events, per-query arrays, overflow table and push log of one workspace, for nq queries on `slots` waves
isl_status prepare_workspace(const isl_index* idx, isl::SearchWorkspace& ws, uint32_t nq, uint32_t slots,
                             uint32_t plog_cap);
isl_status search_enqueue(const isl_index* idx, isl::SearchWorkspace& ws, const SearchCall& c,
                          const RoundPlan& plan = RoundPlan{}, bool warm = false);
isl_status search_finish(const isl_index* idx, isl::SearchWorkspace& ws, uint32_t* misses = nullptr,
                         bool defer_statuses = false);
isl_status search_statuses(isl::SearchWorkspace& ws, uint64_t nq);
isl_status search_sync(const isl_index* idx, isl::SearchWorkspace& ws, const SearchCall& c);

// ---- search_recompute.hip
isl_status prepare_recompute(isl::SearchWorkspace& ws, uint64_t nq, uint64_t state_words_per_query);
isl_status tl_retry_short(isl::SearchWorkspace& ws, uint64_t nq, uint32_t& window_scale, uint32_t* nshort);
isl_status recompute_rounds(const isl_index* idx, isl::SearchWorkspace& ws, const SearchCall& c);
isl_status recompute_coalesced(const isl_index* idx, isl::SearchWorkspace& ws, const SearchCall& c);

// ---- search_group.hip: asynchronous device-pointer calls that find the chip full share one launch
// (rules: search_group_plan.hpp).  A call the group path takes keeps its lane and its token; its kernels are
// enqueued now or at a later entry into the library, alone on its lane or as a member of a group launch.
bool group_takes(const isl_index* idx, const SearchCall& c);
// the call (lane claimed, device selected) joins the held set; whatever the rules release is submitted.  An
// error is this call's own (its launch could not be enqueued): the caller releases the lane.
isl_status group_arrive(const isl_index* idx, isl::SearchWorkspace& ws, const SearchCall& c);
// a pump: submits what the rules release now (no-op for an index without group state)
void group_pump(const isl_index* idx);
// the call of lane `ws` is about to be waited for (by the host or by a stream): it is submitted if it is still
// held.  Returns the status of its enqueue.
isl_status group_before_wait(const isl_index* idx, isl::SearchWorkspace& ws);
// ... and its wait is over: the launch counts as complete, its workspace is free once every member's is
void group_after_wait(const isl_index* idx, isl::SearchWorkspace& ws);
// isl_index_prepare: the group workspaces beside `lanes` lanes of max_nq queries, their kernels warmed
// (ovf_waves = the most resident waves of any launch on the device)
isl_status group_prepare(const isl_index* idx, uint64_t max_nq, uint64_t max_ef, uint64_t max_k, int32_t lanes,
                         uint32_t ovf_waves, uint32_t plog_cap);

}  // namespace isl_lane
