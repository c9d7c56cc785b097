// What one enqueue launches: the kernels of a search call, in stream order, each with its grid, LDS,
// instantiation and the per-launch values of SearchParams, plus the call-level facts the parameter fill
// and the lane bookkeeping need.  Host-only, in the manner of search_geometry.hpp: no HIP call, no
// isl_index.  search.hip fills LaunchFacts from the index, asks plan_launches and issues the steps in one
// loop; tests/cpp/launch_plan_dump.cpp prints the plans of a grid of calls without a device
// (tests/test_search_launch_plan_cpu.py).
#pragma once

#include "search_geometry.hpp"
#include "search_internal.hpp"

namespace {

// what the decision reads from the index beyond CallGeometry
struct LaunchFacts {
  int dtype = ISL_DTYPE_F32;  // rows as stored (ISL_DTYPE_*)
  int metric = 0;
  bool is_hnsw = false;
  uint32_t max_level = 0;
  bool recompute = false;  // the recompute provider
  uint64_t max_degree = 0;
  bool seeds = false;          // entry seeds are set
  bool build_q_entry = false;  // a construction search of the HnswGraph builder
  uint32_t pool_slots = 0;     // slots of the heap-exact kernel's scratch pool
};

struct CallShape {
  uint64_t nq = 0;
  bool two_level = false;
};

enum class StepKind : uint8_t {
  SeedRedo,     // the queries parked in the heap-exact kernel go back to its queue (nq of the lane's xlist)
  PqTables,     // the PQ distance tables of the call's nq queries
  Classify,     // splits the queries into bf16-valued ones (qsel_h) and the others (qsel)
  TwoLevel,
  Descent,      // HnswGraph: greedy descent through the upper layers into q_entry
  EntryPick,    // entry seeds: the nearest seed of each of nq queries into q_entry
  Fast,
  FillRedoAll,  // no traversal kernel in front: the host queues [0, nq) for the heap-exact kernel and
                // synchronises the stream
  Exact,
};

// One unit of device work.  nq, hbits, hcap and qsel_mode are what the kernel is told (applied to a copy
// of the call's SearchParams); the rest selects the instantiation.
struct LaunchStep {
  StepKind kind;
  uint32_t grid = 0;
  size_t lds = 0;
  uint32_t nq = 0;
  uint32_t hbits = 0, hcap = 0;
  uint32_t qsel_mode = 0;  // 1: list mode over the queries the bf16-query launch in front passed on
  int S = 1, metric = 0, dtype = ISL_DTYPE_F32;
  bool wide = false, resume = false, qh = false, bf16 = false, hnsw = false;
};

enum class QlistUse : uint8_t { None, ListedRound, Retry };

struct LaunchPlan {
  static constexpr uint32_t kMaxSteps = 6;  // (the longest: Descent, Classify, Fast, Fast, Exact)
  LaunchStep steps[kMaxSteps];
  uint32_t count = 0;

  bool two_level = false;
  bool use_fast = false;
  bool resume = false;       // a round of the recompute provider: parked-query state is handed to the kernels
  bool seeded = false;
  bool prepare_lane = false; // the lane's per-query arrays are sized for this call, on lane_slots waves
  uint32_t lane_slots = 0;
  bool wants_ell = false;    // the launch reads the padded adjacency
  bool measures = false;     // the call may carry the ISL_DEBUG / ISL_TIMELINE buffers
  uint32_t nq = 0;           // what a kernel is told unless its step says otherwise
  uint32_t max_level = 0;
  bool construction = false; // q_entry / q_evals are the builder's and status is zeroed ahead of the launches
  uint64_t q_entry_words = 0;  // words of the lane's q_entry this call needs (0: it is not used)
  bool entry_given = false;
  bool exact_park_fields = false;  // the heap-exact kernel parks and resumes too
  QlistUse qlist = QlistUse::None;
  bool qsel = false;         // a Classify step fills the lane's two selections
  uint32_t tl_prefetch = 0;
  bool publishes = false;    // the call completes: publish, ev_done, in-flight bookkeeping
};

inline LaunchPlan plan_launches(const LaunchFacts& f, const CallShape& c, const isl_lane::RoundPlan& rp, bool warm,
                                const CallGeometry& cg) {
  const uint64_t nq = c.nq;
  const bool tl = c.two_level, use_fast = cg.use_fast, bf16 = f.dtype == ISL_DTYPE_BF16;
  // searches over the recompute provider park and resume on the fast kernel (f32 rows; the two-level
  // and heap-exact kernels re-run a blocked query from its start instead)
  const bool resume = !warm && (rp.active != 0 || rp.exact != 0);
  // two-level search over bf16 rows: first the instantiation that keeps a bf16-valued query as bf16 in
  // LDS, then the float32-query one over the queries it passed on.  tl_qh is dropped for retries (their
  // list mode), resumes and warm launches.
  const bool tl_qh = tl && !warm && !resume && bf16 && rp.retry == 0 && cg.tl_hbits_q == cg.fg.hbits;
  // the fast kernel's bf16-query instantiation in front; qh is dropped for resumed rounds
  const bool qh = cg.qh && !resume;
  // A warm launch runs on a grid of one workgroup (it has to exist) with nq = 0; it still launches the
  // qh pair, the descent and the exact kernel.
  const uint64_t nq_grid = warm ? 1 : nq;

  LaunchPlan lp;
  lp.two_level = tl;
  lp.use_fast = use_fast;
  lp.resume = resume;
  lp.prepare_lane = lp.measures = lp.publishes = !warm;
  // per-slot state is indexed by blockIdx.x < min(nq, slots) -- by the query when it can come back on
  // another wave
  lp.lane_slots = (uint32_t)(f.recompute ? nq : std::min<uint64_t>(nq, cg.lane_slots));
  lp.wants_ell = use_fast || (tl && f.max_degree <= 128);
  lp.nq = warm ? 0u : (uint32_t)nq;
  // The construction search starts every query at the builder's node on the layer in d_ell: max_level = 0,
  // so it never descends, and it is never seeded.
  lp.construction = f.build_q_entry && !warm;
  lp.max_level = f.is_hnsw && !lp.construction ? f.max_level : 0u;
  // entry seeds: a plain search over resident rows starts every query at the seed nearest to it; two-level
  // searches, the recompute provider and an HnswGraph (max_level stays as it is) keep entry_point
  lp.seeded = f.seeds && !tl && !f.recompute && !f.is_hnsw && !f.build_q_entry && !warm && !resume && nq != 0;
  const bool descends = !tl && use_fast && f.is_hnsw && lp.max_level > 0;
  lp.q_entry_words = lp.seeded ? nq * 4 : descends ? std::max<uint64_t>(nq, 1) * 2 : 0;
  lp.entry_given = lp.construction || lp.seeded;
  lp.exact_park_fields = resume && !tl && rp.exact_parks;
  lp.qlist = resume ? (rp.listed ? QlistUse::ListedRound : QlistUse::None)
                    : tl && rp.retry ? QlistUse::Retry : QlistUse::None;  // (a retry: the short-window queries, alone)
  lp.qsel = tl_qh || qh;
  lp.tl_prefetch = tl && resume ? rp.prefetch : 0u;

  // a step with the call's own values; the callers below change what differs
  auto add = [&](StepKind kind, uint64_t grid, size_t lds, uint32_t told) -> LaunchStep& {
    LaunchStep& s = lp.steps[lp.count++];
    s.kind = kind;
    s.grid = (uint32_t)grid;
    s.lds = lds;
    s.nq = told;
    s.hbits = cg.fg.hbits;
    s.hcap = cg.fg.hcap;
    s.S = cg.segments;
    s.metric = f.metric;
    s.dtype = f.dtype;
    s.wide = f.max_degree > 64;
    s.resume = resume;
    s.bf16 = bf16;
    s.hnsw = f.is_hnsw;
    return s;
  };
  // the classify grid is capped at 2048
  auto classify = [&](uint32_t told) { add(StepKind::Classify, std::min<uint64_t>(nq_grid, 2048), 0, told); };

  if (resume && !tl && rp.exact) add(StepKind::SeedRedo, 1, 0, rp.exact);
  if (tl) {
    // build_distance_tables for the whole batch (pq.rs:307-338; once per call: the rounds of the
    // recompute provider and a retry keep them), then one wave per query
    if (!warm && !rp.tables_built) add(StepKind::PqTables, 0, 0, (uint32_t)nq);
    const uint64_t n_run = resume ? rp.active : rp.retry ? rp.retry : nq_grid;
    const uint32_t told = warm ? 0u : (uint32_t)n_run;
    if (tl_qh) {
      classify(told);
      LaunchStep& h = add(StepKind::TwoLevel, std::min<uint64_t>(nq_grid, cg.tl_slots_q), cg.tl_lds_q, told);
      h.qh = true;
      add(StepKind::TwoLevel, std::min<uint64_t>(n_run, cg.slots), cg.tl_lds, told).qsel_mode = 1;  // the others
    } else {
      // the two-level warm launch on a recompute index uses the RESUME instantiation (what its rounds run)
      add(StepKind::TwoLevel, std::min<uint64_t>(n_run, cg.slots), cg.tl_lds, told).resume = resume || (warm && f.recompute);
    }
    return lp;  // (the two-level kernel hands nothing to the heap-exact kernel)
  }
  // HnswGraph::search: greedy descent through the upper layers first (its own kernel, so that the
  // traversal kernel keeps its register budget); the descent grid is capped at 8192
  if (descends) add(StepKind::Descent, std::min<uint64_t>(nq_grid, 8192), cg.descent_lds, lp.nq);
  // q_entry[q] = the nearest seed, q_evals[q] = 1, status[q] = QS_OK: ahead of the traversal that reads them
  if (lp.seeded) add(StepKind::EntryPick, 0, 0, (uint32_t)nq);
  if (use_fast) {
    // the traversal kernel is told nq = active in a round: it runs this round's queries
    const uint32_t told = resume ? rp.active : lp.nq;
    const uint64_t grid = std::min<uint64_t>(resume ? rp.active : nq_grid, cg.slots);
    if (qh) {
      classify(told);
      LaunchStep& h = add(StepKind::Fast, std::min<uint64_t>(nq_grid, cg.slots_q), cg.fgq.lds, told);  // the bf16-valued queries
      h.qh = true;
      h.hbits = cg.fgq.hbits;
      h.hcap = cg.fgq.hcap;
      add(StepKind::Fast, grid, cg.fg.lds, told).qsel_mode = 1;  // the others
    } else if (!(resume && rp.active == 0)) {
      // (a round with active == 0 and exact > 0 has only queries parked in the heap-exact kernel: it skips
      // the traversal but not SeedRedo or Exact)
      add(StepKind::Fast, grid, cg.fg.lds, told);
    }
  } else if (!warm && !resume) {
    add(StepKind::FillRedoAll, 0, 0, (uint32_t)nq);  // every query goes to the exact kernel: redo = [0, nq)
  }
  // the exact kernel is always told the call's nq (behind a fast kernel even when the launch is warm;
  // without one a warm launch tells it 0)
  add(StepKind::Exact, std::min<uint64_t>(nq_grid, f.pool_slots), cg.exact_lds, use_fast ? (uint32_t)nq : lp.nq);
  return lp;
}

}  // namespace
