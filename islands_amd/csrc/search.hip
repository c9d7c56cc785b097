// LEANN best-first search on gfx950: one 64-lane wavefront per query.
//
// Replaces LeannIndex::search_with_params / search_layer_recompute
// (src/core/leann.rs:868-988) over an EmbeddingProvider (in-memory rows, leann.rs:104-159, or the
// recompute provider) with DistanceMetric::calculate (src/core/distance.rs:37-122); the same
// kernels serve HnswGraph::search (src/core/hnsw.rs:458-504) and the graph builder's
// construction searches.
//
// Parity design:
//   * distances are computed in the reference's exact operation order: the strictly sequential
//     f32 chain of a row (separate multiply and add roundings, -ffp-contract=off), so every
//     distance is bit-identical to the Rust scalar loop and every traversal decision (strict
//     float compares at leann.rs:925,959) matches.  The four lanes of a quad own one row, load 16
//     of every 64 bytes of it straight from global memory into a register ring and exchange the
//     products with DPP (device_common.hip.h, direct_distances).
//   * fast kernel: the result set R (<= ef entries, key = (OrderedFloat d, id)) lives in registers
//     as a sorted array spread over the wave; the candidate heap is implicit (live candidates are
//     exactly the unexpanded entries of R); the pushes of a hop are merged into R at once.
//     Situations where the reference's BinaryHeap internals become observable (equal distances
//     inside the returned prefix, or between an evicted entry and the new worst) are replayed from
//     a push log or handed to the exact kernel.
//   * exact kernel: emulates Rust's BinaryHeap push/pop/into_iter byte for byte (candidates in
//     HBM scratch, results in LDS) for those queries, for ef > 512, for adjacency rows longer
//     than 64 and for NaN / -0.0 distances.
#include "search_launch_plan.hpp"

#include <cmath>

using namespace isl_lane;

namespace {

__global__ void fill_u32_kernel(uint32_t* p, uint64_t n, uint32_t v) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = v;
}

// The search path moves its small host<->device traffic with kernels that read / write the
// lane's pinned host buffers directly (they are mapped into the device's address space) instead
// of hipMemcpyAsync: a call is then kernels and two event records only.  (The runtime's async
// copies draw completion signals from pools that grow one concurrent copy at a time, several
// milliseconds each -- measured as 7 ms stalls inside the first dozens of pipelined calls.)
struct PublishParams {
  const uint32_t* src[6];
  uint32_t* dst[6];
  uint32_t words[6];
  uint32_t ticket_seg;  // that segment's source is zeroed once copied: the next call's work-queue heads
};
__global__ void publish_kernel(PublishParams pp) {
  const uint32_t seg = blockIdx.y;
  const uint32_t n = pp.words[seg];
  const uint32_t* __restrict__ src = pp.src[seg];
  uint32_t* __restrict__ dst = pp.dst[seg];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    dst[i] = src[i];
    if (seg == pp.ticket_seg) const_cast<uint32_t*>(src)[i] = 0u;
  }
}
__global__ void copy_u128_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    dst[i] = src[i];
}
__global__ void copy_u32_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    dst[i] = src[i];
}

// recompute provider: the queries parked in the heap-exact kernel go straight back to its queue
__global__ void seed_redo_kernel(const uint32_t* __restrict__ list, uint32_t n, uint32_t* __restrict__ redo,
                                 uint32_t* __restrict__ ticket) {
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) redo[i] = list[i];
  if (threadIdx.x == 0) ticket[1] = n;
}

constexpr uint32_t kExactSlots = 32;
constexpr uint32_t kOvfBits = 15;

// Every allocation of the search path is a reserve() that counts into the lane's alloc_events: a
// lane counts what it had to set up, and a call reports its share in isl_search_stats::allocations
// (0 once isl_index_prepare has run).

// Streams, events, per-query arrays, overflow table, push log of one lane, sized for nq queries
// on `slots` resident waves.
// The lanes' streams come from ONE pool per device and process: a card serves only so many hardware
// queues side by side, and past about twenty streams in use the search rate collapses (24 streams on
// one card: 0.39 M queries/s where 16 reach 1.4 M; two processes with 12 each: 16 k against 145 k --
// DESIGN section 4).  More lanes than pool streams simply share: lane i of any index runs on stream
// i mod pool size, its calls in stream order behind the other lane's, every call waited for through
// its own event.  ISL_MAX_STREAMS (1..32, default 16) sizes the pool -- processes that share a card
// should divide the sixteen between them.  Pool streams live as long as the process.
hipStream_t pool_stream(int32_t device, uint32_t lane, bool* created) {
  static std::mutex mu;
  static hipStream_t pool[64][32];
  static const uint32_t size = [] {
    const char* e = getenv("ISL_MAX_STREAMS");
    const int v = e ? atoi(e) : 16;
    return (uint32_t)std::min(std::max(v, 1), 32);
  }();
  *created = false;
  if (device < 0 || device >= 64) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  hipStream_t& st = pool[device][lane % size];
  if (!st) {
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); st = nullptr; }
    else *created = true;
  }
  return st;
}

}  // namespace

isl_status isl_lane::ensure_lane_stream(const isl_index* idx, isl::SearchWorkspace& ws) {
  if (ws.stream) return ISL_OK;
  bool created = false;
  // (a group workspace is not one of idx->ws: it names its pool stream itself)
  hipStream_t st = pool_stream(idx->device, ws.pool_lane >= 0 ? (uint32_t)ws.pool_lane : (uint32_t)(&ws - idx->ws), &created);
  if (!st) return isl::fail(ISL_ERR_DEVICE, "hipStreamCreate failed for a search lane");
  if (created) ws.alloc_events++;
  if (!ws.ev_done) { ISL_HIP(hipEventCreateWithFlags(&ws.ev_done, hipEventDisableTiming)); ws.alloc_events++; }
  if (!ws.ev0) { ISL_HIP(hipEventCreate(&ws.ev0)); ws.alloc_events++; }
  if (!ws.ev1) { ISL_HIP(hipEventCreate(&ws.ev1)); ws.alloc_events++; }
  if (!ws.ev_in) { ISL_HIP(hipEventCreateWithFlags(&ws.ev_in, hipEventDisableTiming)); ws.alloc_events++; }
  if (!ws.ticket) {
    ISL_TRY(ws.ticket.reserve(16, &ws.alloc_events));
    ws.ticket_clean = false;
  }
  ISL_TRY(ws.h_head.reserve(16, &ws.alloc_events));
  ws.stream = st;
  return ISL_OK;
}

void isl_lane::copy_words(const uint32_t* src, uint32_t* dst, uint64_t n, uint32_t grid, uint32_t block, hipStream_t st) {
  hipLaunchKernelGGL(copy_u32_kernel, dim3(grid), dim3(block), 0, st, src, dst, n);
}

isl_status isl_lane::prepare_workspace(const isl_index* idx, isl::SearchWorkspace& ws, uint32_t nq, uint32_t slots,
                                       uint32_t plog_cap) {
  ISL_TRY(ensure_lane_stream(idx, ws));
  uint64_t* const ev = &ws.alloc_events;
  const uint64_t cap = nq < 1024 ? 1024 : nq;  // the per-query arrays' floor
  ISL_TRY(ws.h_status.reserve(cap, ev));
  ISL_TRY(ws.h_ctr.reserve(cap * 4, ev));
  if (ws.slots < slots || !ws.ovf_tab) {
    ws.ovf_tab.reset();
    ws.slots = 0;
    // (ISL_OVF_BITS: the overflow table's size for measurements; a query that fills 3/4 of it goes to the heap-exact kernel)
    static const uint32_t ovf_bits_cfg = [] {
      const char* e = getenv("ISL_OVF_BITS");
      const int v = e ? atoi(e) : (int)kOvfBits;
      return (uint32_t)std::min(15, std::max(10, v));
    }();
    ws.ovf_bits = ovf_bits_cfg;
    uint64_t n = (uint64_t)slots << ovf_bits_cfg;
    ISL_TRY(ws.ovf_tab.reserve(n, ev));
    hipLaunchKernelGGL(fill_u32_kernel, dim3(2048), dim3(256), 0, ws.stream, ws.ovf_tab, n, EMPTY);
    ISL_HIP(hipGetLastError());
    ISL_HIP(hipStreamSynchronize(ws.stream));
    ws.slots = slots;
  }
  ISL_TRY(ws.status.reserve(cap, ev));
  ISL_TRY(ws.payload.reserve(cap, ev));
  ISL_TRY(ws.ctr.reserve(cap * 4, ev));
  ISL_TRY(ws.redo.reserve(cap, ev));
  ISL_TRY(ws.replay.reserve(cap, ev));
  ISL_TRY(ws.qsel.reserve(cap, ev));
  ISL_TRY(ws.qsel_h.reserve(cap, ev));
  return ws.plog.reserve(ws.status.capacity() * plog_cap, ev);
}

namespace {

// Staging of the host-pointer entry points: device buffers + pinned host mirrors.
isl_status prepare_host_staging(isl::SearchWorkspace& ws, uint64_t nq, uint64_t d, uint64_t k) {
  uint64_t* const ev = &ws.alloc_events;
  ISL_TRY(ws.q_stage.reserve(nq * d, ev));
  ISL_TRY(ws.h_q.reserve(nq * d, ev));
  const uint64_t slots = nq * std::max<uint64_t>(k, 1);
  ISL_TRY(ws.ids_stage.reserve(slots, ev));
  ISL_TRY(ws.dist_stage.reserve(slots, ev));
  ISL_TRY(ws.count_stage.reserve(slots, ev));
  ISL_TRY(ws.h_ids.reserve(slots, ev));
  ISL_TRY(ws.h_dist.reserve(slots, ev));
  return ws.h_count.reserve(slots, ev);
}

}  // namespace

// The shared scratch pool of the heap-exact kernel (under idx->mu).  Its sizes follow the index
// (node / row count, longest row); the setters that change those drop the pool.
isl_status isl_lane::ensure_pool(const isl_index* idx, isl::SearchWorkspace& ws) {
  isl::ExactPool& pl = idx->pool;
  if (pl.slots) return ISL_OK;
  uint64_t max_id = std::max(idx->num_nodes, idx->nvec);
  pl.vis_words = (max_id + 31) / 32 + 1;
  pl.cand_cap = std::min<uint64_t>(max_id + 1, 1ull << 21);
  pl.ulist_cap = std::max<uint32_t>(idx->max_degree, 64);
  isl_status st = ISL_OK;
  uint64_t* const ev = &ws.alloc_events;
  pl.xstate_words = 16 + 2 * (kMaxExactEf + 1);
  if ((st = pl.cand_d.reserve(kExactSlots * pl.cand_cap, ev)) == ISL_OK &&
      (st = pl.cand_id.reserve(kExactSlots * pl.cand_cap, ev)) == ISL_OK &&
      (st = pl.vis_bits.reserve(kExactSlots * pl.vis_words, ev)) == ISL_OK &&
      (st = pl.ulist.reserve((uint64_t)kExactSlots * pl.ulist_cap, ev)) == ISL_OK &&
      (st = pl.locks.reserve(kExactSlots, ev)) == ISL_OK &&
      (st = pl.xstate.reserve((uint64_t)kExactSlots * pl.xstate_words, ev)) == ISL_OK) {
    if (hipMemset(pl.locks, 0, (size_t)kExactSlots * 4) == hipSuccess) {
      pl.slots = kExactSlots;
      return ISL_OK;
    }
    st = isl::fail(ISL_ERR_DEVICE, "hipMemset failed for the exact-kernel pool");
  }
  isl::free_exact_pool(pl);
  return st;
}

namespace {

// CSR -> W (64 or 128) ids per node (EMPTY-padded) + degree; one wave per row
__global__ void pad_rows_kernel(const uint64_t* __restrict__ off, const uint32_t* __restrict__ adj, uint64_t n,
                                uint32_t W, uint32_t* __restrict__ ell, uint32_t* __restrict__ deg) {
  const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (row >= n) return;
  const uint64_t o0 = off[row];
  const uint32_t d = (uint32_t)(off[row + 1] - o0);
  for (uint32_t i = lane; i < W; i += 64) ell[row * W + i] = i < d ? adj[o0 + i] : EMPTY;
  if (lane == 0) deg[row] = d;
}

// status / counters / work-queue heads of the call -> the lane's pinned mirrors, and for a
// host-buffer call its answers too; one kernel behind the search kernels.
isl_status publish(isl::SearchWorkspace& ws, uint64_t nq, uint64_t k, hipStream_t st) {
  PublishParams pp{};
  uint32_t n = 0;
  auto seg = [&](const void* src, void* dst, uint64_t words) {
    pp.src[n] = (const uint32_t*)src; pp.dst[n] = (uint32_t*)dst; pp.words[n] = (uint32_t)words; ++n;
  };
  seg(ws.status, ws.h_status, nq);
  seg(ws.ctr, ws.h_ctr, nq * 4);
  pp.ticket_seg = n;
  seg(ws.ticket, ws.h_head, 16);
  if (ws.publish_results) {
    seg(ws.count_stage, ws.h_count, nq);
    if (k) {
      seg(ws.ids_stage, ws.h_ids, nq * k * 2);
      seg(ws.dist_stage, ws.h_dist, nq * k);
    }
  }
  hipLaunchKernelGGL(publish_kernel, dim3(16, n), dim3(256), 0, st, pp);
  ISL_HIP(hipGetLastError());
  ws.ticket_clean = true;
  return ISL_OK;
}

// (SearchCall, the call as its entry point received it, and RoundPlan, what a round asks of one enqueue:
// search_internal.hpp)

// the one switch over the fast kernel's S: each case is an object of its own (search_fast.hip)
void launch_fast(const isl_launch::FastKernel& k, uint32_t grid, size_t lds, hipStream_t st, const SearchParams& p) {
  switch (k.S) {
    case 1: isl_launch::launch_fast_segments<1>(k, grid, lds, st, &p); break;
    case 2: isl_launch::launch_fast_segments<2>(k, grid, lds, st, &p); break;
    case 4: isl_launch::launch_fast_segments<4>(k, grid, lds, st, &p); break;
    default: isl_launch::launch_fast_segments<8>(k, grid, lds, st, &p); break;
  }
}

// the two environment switches of the measurement aids, read once; the enqueue and the finish share them
bool debug_on() {
  static const bool on = getenv("ISL_DEBUG") != nullptr;
  return on;
}
// ISL_TIMELINE=<file>: start / end tick of every query of every call, appended at wait time
// (measurement aid: where a run's fill and drain go; tools/timeline.py reads the file)
const char* timeline_path() {
  static const char* const path = getenv("ISL_TIMELINE");
  return path;
}

// what plan_launches reads from the index (an index without its scratch pool gets the slots ensure_pool
// gives it ahead of the launches)
LaunchFacts launch_facts(const isl_index* idx) {
  LaunchFacts f;
  f.dtype = idx->rows.dtype();
  f.metric = (int)idx->cfg.metric;
  f.is_hnsw = idx->is_hnsw;
  f.max_level = (uint32_t)idx->max_level;
  f.recompute = idx->recompute;
  f.max_degree = idx->max_degree;
  f.seeds = idx->seeds.count() != 0;
  f.build_q_entry = idx->build_q_entry != nullptr;
  f.pool_slots = idx->pool.slots ? idx->pool.slots : kExactSlots;
  return f;
}

// The SearchParams of a call, every field assigned once; the lane's buffers are reserved by now.  What a
// single launch is told differently (nq, hbits, hcap, qsel_mode) is its step's (search_launch_plan.hpp).
SearchParams fill_params(const isl_index* idx, const isl::SearchWorkspace& ws, const SearchCall& c,
                         const CallGeometry& cg, const LaunchPlan& lp) {
  const uint64_t nq = c.nq, d = c.d, k = c.k;
  SearchParams p{};
  p.off = idx->d_off;
  p.adj = idx->d_ell ? idx->d_ell : idx->d_adj;
  p.ell_w = idx->d_ell ? idx->ell_w : 0u;
  p.ell_deg = idx->d_ell_deg;
  p.num_nodes = idx->num_nodes;
  p.emb = idx->rows.data();
  p.emb_dtype = (uint32_t)idx->rows.dtype();
  p.emb_scale = std::ldexp(1.0f, idx->rows.scale_exp());
  p.norm2 = idx->rows.norm2();
  p.nvec = idx->nvec;
  p.stride = idx->rows.stride();
  p.d = (uint32_t)d;
  p.queries = c.queries;
  p.nq = lp.nq;
  p.k = (uint32_t)k;
  p.ef = cg.ef;
  p.prune_ratio = idx->cfg.prune_ratio;
  p.prune_strategy = idx->cfg.pruning_strategy;
  p.entry = (uint32_t)std::min<uint64_t>(idx->entry_point, 0x7FFFFFF0ull);
  p.out_ids = c.ids;
  p.out_dist = c.dist;
  p.out_count = c.count;
  p.status = ws.status;
  p.payload = ws.payload;
  p.ctr = ws.ctr;
  p.ticket = ws.ticket;
  p.redo = ws.redo;
  p.prof = ws.d_prof;
  p.tline = ws.d_tline;
  p.replay = ws.replay;
  p.plog = reinterpret_cast<uint2*>(ws.plog.get());
  p.plog_cap = cg.plog_cap;
  p.hbits = cg.fg.hbits;
  p.hcap = cg.fg.hcap;
  p.otab = ws.ovf_tab;
  p.obits = ws.ovf_bits;
  p.cand_d = idx->pool.cand_d;
  p.cand_id = idx->pool.cand_id;
  p.cand_cap = idx->pool.cand_cap;
  p.vis_bits = idx->pool.vis_bits;
  p.vis_words = idx->pool.vis_words;
  p.ulist = idx->pool.ulist;
  p.ulist_cap = idx->pool.ulist_cap;
  p.pool_locks = idx->pool.locks;
  p.pool_slots = idx->pool.slots;
  if (lp.exact_park_fields) {  // the heap-exact kernel parks and resumes too (recompute provider, bounded cache)
    p.xslot = ws.xslot;
    p.xstate = idx->pool.xstate;
    p.xstate_words = idx->pool.xstate_words;
  }
  p.slot_of = idx->recompute ? idx->d_slot_of : nullptr;
  p.stamp = idx->d_stamp;
  p.round_no = idx->round_no;
  if (lp.resume) {
    p.qstate = ws.qstate;
    p.qstate_words = cg.state_words;
    p.qflag = ws.qflag;
  }
  // (a listed round's queries, or a retry's: those whose queue window was too small, alone, with a larger one)
  p.qlist = lp.qlist != QlistUse::None ? ws.qlist.get() : nullptr;
  p.miss = ws.miss;
  p.miss_cap = (uint32_t)std::min<uint64_t>(ws.miss_cap, 0xFFFFFFFFull);
  p.pref = ws.miss ? ws.miss + ws.miss_cap : nullptr;
  p.pref_cap = (uint32_t)ws.pref_cap;
  p.tl_prefetch = ws.pref_cap ? lp.tl_prefetch : 0u;
  p.layer_off = idx->d_layer_off;
  p.layer_adj = idx->d_layer_adj;
  p.max_level = lp.max_level;
  p.hnsw_order = idx->is_hnsw ? 1u : 0u;
  if (lp.construction) {
    // construction search of the HnswGraph builder: per-query entry nodes on the layer in d_ell
    p.q_entry = idx->build_q_entry;
    p.q_evals = idx->build_q_evals;
  } else if (lp.q_entry_words) {  // the seed pick's or the descent's, a launch ahead of the traversal
    p.q_entry = ws.q_entry;
    p.q_evals = ws.q_entry + nq;
  }
  p.entry_given = lp.entry_given ? 1u : 0u;
  if (lp.qsel) {
    p.qsel = ws.qsel;
    p.qsel_h = ws.qsel_h;
  }
  if (lp.two_level) {
    p.tl_tables = ws.tl_tables;
    p.tl_codes = idx->d_codes;
    p.tl_ncodes = idx->ncodes;
    p.tl_m = (uint32_t)idx->pq->m;
    p.tl_K = (uint32_t)idx->pq->K;
    p.tl_ratio = c.ratio;
    p.tl_wcap = cg.tl_wcap;
  }
  return p;
}

// Enqueues the kernels of one search on a claimed lane: geometry, plan, the lane's buffers, the
// parameters, then the plan's steps in order.
// warm = true: the same launches over zero queries (isl_index_prepare: loads the code objects and
// brings the lane's stream up) -- nothing is read or written beyond the ticket words.
isl_status search_enqueue_impl(const isl_index* idx, isl::SearchWorkspace& ws, const SearchCall& c,
                               const RoundPlan& plan, bool warm) {
  const uint64_t nq = c.nq, k = c.k;
  if (nq > 0x7FFFFFFFull) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "too many queries");
  const TwoLevelCall tl_call{c.ratio, plan.window_scale};
  CallGeometry cg;
  ISL_TRY(call_geometry(idx, c.d, k, c.ef, c.two_level ? &tl_call : nullptr, cg));
  const LaunchPlan lp = plan_launches(launch_facts(idx), CallShape{nq, c.two_level}, plan, warm, cg);
  if (lp.prepare_lane) ISL_TRY(prepare_workspace(idx, ws, (uint32_t)nq, lp.lane_slots, cg.plog_cap));
  if (!idx->pool.slots || (lp.wants_ell && !idx->d_ell && idx->d_off && idx->num_nodes)) {
    // not prepared (isl_index_prepare / isl_index_upload do this ahead of time)
    std::lock_guard<std::mutex> lock(idx->mu);
    ISL_TRY(ensure_pool(idx, ws));
    const uint32_t* before = idx->d_ell;
    ISL_TRY(isl::ensure_padded_adjacency(const_cast<isl_index*>(idx)));
    if (idx->d_ell != before) ws.alloc_events += 2;
  }
  hipStream_t st = call_stream(ws, c);
  if (c.mode == StreamMode::OWN_AFTER_USER || c.mode == StreamMode::OWN_AFTER_EVENT) {
    if (c.mode == StreamMode::OWN_AFTER_USER) ISL_HIP(hipEventRecord(ws.ev_in, c.user_stream));
    ISL_HIP(hipStreamWaitEvent(ws.stream, ws.ev_in, 0));
  }

  ws.d_prof.reset();
  if (debug_on() && lp.measures) {
    ISL_TRY(ws.d_prof.reserve(nq * 8));
    ISL_HIP(hipMemset(ws.d_prof, 0, nq * 64));
  }
  ws.d_tline.reset();
  if (timeline_path() && lp.measures) {
    ISL_TRY(ws.d_tline.reserve(nq * 2));
    ISL_HIP(hipMemset(ws.d_tline, 0, nq * 16));
  }
  if (lp.q_entry_words) ISL_TRY(ws.q_entry.reserve(lp.q_entry_words, &ws.alloc_events));
  if (lp.two_level)
    ISL_TRY(ws.tl_tables.reserve(std::max<uint64_t>(nq, 1) * idx->pq->m * idx->pq->K, &ws.alloc_events));
  const SearchParams p = fill_params(idx, ws, c, cg, lp);

  // (QS_OK: the fast kernel reads status where q_entry is set)
  if (lp.construction) ISL_HIP(hipMemsetAsync(ws.status, 0, nq * 4, st));
  // the work-queue heads are zero at this point: the publish kernel of the lane's previous call
  // left them so; only a lane's first call (or one after a failed enqueue) clears them itself
  if (!ws.ticket_clean) ISL_HIP(hipMemsetAsync(ws.ticket, 0, 64, st));
  ws.ticket_clean = false;
  ISL_HIP(hipEventRecord(ws.ev0, st));
  ws.launch_ms_read = false;
  for (uint32_t i = 0; i < lp.count; ++i) {
    const LaunchStep& s = lp.steps[i];
    SearchParams sp = p;  // what this launch is told
    sp.nq = s.nq;
    sp.hbits = s.hbits;
    sp.hcap = s.hcap;
    sp.qsel_mode = s.qsel_mode;
    switch (s.kind) {
      case StepKind::SeedRedo:
        hipLaunchKernelGGL(seed_redo_kernel, dim3(1), dim3(256), 0, st, ws.h_xlist, s.nq, ws.redo, ws.ticket);
        break;
      case StepKind::PqTables:
        ISL_TRY(isl::pq_launch_tables(idx->pq, c.queries, s.nq, ws.tl_tables, st));
        break;
      case StepKind::Classify:
        isl_launch::launch_classify(s.grid, st, &sp);
        break;
      case StepKind::TwoLevel:
        isl_launch::launch_two_level(s.metric, s.bf16, s.resume, s.qh, s.grid, s.lds, st, &sp);
        break;
      case StepKind::Descent:
        isl_launch::launch_descent(s.metric, s.bf16, s.grid, s.lds, st, &sp);
        break;
      case StepKind::EntryPick:
        ISL_TRY(isl::launch_entry_pick(idx, c.queries, s.nq, ws.q_entry, ws.q_entry + s.nq,
                                       reinterpret_cast<unsigned long long*>(ws.q_entry + 2 * (uint64_t)s.nq), ws.status,
                                       nullptr, st));
        break;
      case StepKind::Fast:
        launch_fast(isl_launch::FastKernel{s.S, s.metric, s.wide, s.dtype, s.resume, s.qh}, s.grid, s.lds, st, sp);
        break;
      case StepKind::FillRedoAll: {
        std::vector<uint32_t> all(s.nq);
        for (uint32_t q = 0; q < s.nq; q++) all[q] = q;
        const uint32_t head0[4] = {0, s.nq, 0, 0};
        ISL_HIP(hipMemcpyAsync(ws.redo, all.data(), (size_t)s.nq * 4, hipMemcpyHostToDevice, st));
        ISL_HIP(hipMemcpyAsync(ws.ticket, head0, 16, hipMemcpyHostToDevice, st));
        ISL_HIP(hipStreamSynchronize(st));
        break;
      }
      case StepKind::Exact:
        isl_launch::launch_exact(s.metric, s.hnsw, s.grid, s.lds, st, &sp);
        break;
    }
    ISL_HIP(hipGetLastError());
  }
  ISL_HIP(hipEventRecord(ws.ev1, st));
  ws.st_inflight = st;
  if (!lp.publishes) return ISL_OK;

  if (!ws.union_launch) {  // (a group launch: its scatter kernel publishes per member, search_group.hip)
    ISL_TRY(publish(ws, nq, k, st));
    // the call's own completion event: lanes may share a stream, and a caller's stream carries its other work
    ISL_HIP(hipEventRecord(ws.ev_done, st));
  }
  ws.enqueued = true;
  ws.nq_inflight = nq;
  ws.k_inflight = k;
  ws.ef_inflight = cg.ef;
  ws.fast_inflight = lp.use_fast;
  return ISL_OK;
}

// (defined beside search_finish, below)
isl_status report_debug(isl::SearchWorkspace& ws, const isl::DeviceBuffer<uint64_t>& d_prof, uint64_t nq, bool use_fast,
                        float ms);

// counters of the most recent call this thread completed, per index (isl_search_last_stats)
struct LastStats { const isl_index* idx = nullptr; isl_search_stats st{}; };
thread_local LastStats tl_last_stats;
void note_last_stats(const isl_index* idx, const isl_search_stats& st) {
  tl_last_stats.idx = idx;
  tl_last_stats.st = st;
}

}  // namespace

// A failure part-way through an enqueue (a launch error, publish, a lane buffer that could not grow)
// may leave kernels of this call on the stream: they are drained before the error goes back, because
// the caller releases the lane next and the lane's next owner rewrites its pinned buffers / may
// reallocate what those kernels still read.
isl_status isl_lane::search_enqueue(const isl_index* idx, isl::SearchWorkspace& ws, const SearchCall& c,
                                      const RoundPlan& plan, bool warm) {
  const isl_status st = search_enqueue_impl(idx, ws, c, plan, warm);
  if (st != ISL_OK) {
    const isl::ErrorRecord keep = isl::last_error();
    hipStream_t s = call_stream(ws, c);
    if (c.mode == StreamMode::USER || s) (void)hipStreamSynchronize(s);
    (void)hipGetLastError();
    ws.ticket_clean = false;
    ws.enqueued = false;
    isl::last_error() = keep;
  }
  return st;
}

// Waits for the call in flight on `ws`, leaves its counters in ws.stats and turns per-query
// failures into the CoreError the reference's sequential map would have returned.
// defer_statuses: the per-query statuses are not final yet (a batch the recompute provider works
// through in rounds, some of its queries not even started): the caller runs search_statuses itself.
isl_status isl_lane::search_finish(const isl_index* idx, isl::SearchWorkspace& ws, uint32_t* misses,
                                     bool defer_statuses) {
  if (!ws.enqueued) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "no search in flight for this token");
  ws.enqueued = false;
  const uint64_t nq = ws.nq_inflight;
  const bool use_fast = ws.fast_inflight;
  // a member of a group launch: that launch's events (the scatter kernel has filled this lane's mirrors)
  isl::SearchWorkspace& lw = ws.grp_launch ? *ws.grp_launch : ws;
  ISL_HIP(hipEventSynchronize(lw.ev_done));
  const uint32_t* ctr = ws.h_ctr;
  const uint32_t* head = ws.h_head;
  isl::DeviceBuffer<uint64_t> d_prof = std::move(ws.d_prof);
  // The launch's time is read from its events once and kept with the launch: every member of a group launch
  // reports that one figure (two reads of the same event pair may differ in the last bit).
  float ms = 0.0f;
  {
    static std::mutex ms_mu;
    std::lock_guard<std::mutex> lock(ms_mu);
    if (!lw.launch_ms_read) {
      (void)hipEventElapsedTime(&lw.launch_ms, lw.ev0, lw.ev1);
      lw.launch_ms_read = true;
    }
    ms = lw.launch_ms;
  }

  isl_search_stats& ss = ws.stats;
  ss = isl_search_stats{};
  ss.queries = nq;
  ss.exact_path = head[1];
  ss.replayed = head[3];
  ss.kernel_ms = ms;
  ss.allocations = ws.alloc_events - ws.alloc_mark + ws.grp_allocs;
  for (uint64_t i = 0; i < nq; i++) {
    ss.expansions += ctr[i * 4 + 0];
    ss.edges += ctr[i * 4 + 1];
    ss.evals += ctr[i * 4 + 2];
    ss.pushes += ctr[i * 4 + 3];
  }
  // what the next calls size their visited table by (fast_geometry): the evaluations per query of this one
  if (use_fast && !idx->recompute && !misses && nq >= 16)
    idx->evals_hint.store(((uint64_t)ws.ef_inflight << 32) | std::min<uint64_t>(ss.evals / nq, 0xFFFFFFFFull),
                          std::memory_order_relaxed);
  ISL_TRY(report_debug(ws, d_prof, nq, use_fast, ms));
  if (misses) {
    *misses = head[13];
    if (head[13]) return ISL_OK;  // a round of the recompute provider: statuses are not final yet
  }
  if (defer_statuses) return ISL_OK;
  return search_statuses(ws, nq);
}

namespace {
// The ISL_TIMELINE record and the ISL_DEBUG lines of a finished call (d_prof: its phase timers, taken from the lane).
isl_status report_debug(isl::SearchWorkspace& ws, const isl::DeviceBuffer<uint64_t>& d_prof, uint64_t nq, bool use_fast,
                        float ms) {
  const uint32_t* status = ws.h_status;
  const uint32_t* ctr = ws.h_ctr;
  const uint32_t* head = ws.h_head;
  if (ws.d_tline) {
    std::vector<uint64_t> tl(nq * 2 + 2);
    tl[0] = 0x154C494E45ull;  // record header: magic, query count
    tl[1] = nq;
    ISL_HIP(hipMemcpy(tl.data() + 2, ws.d_tline, nq * 16, hipMemcpyDeviceToHost));
    ws.d_tline.reset();
    static std::mutex tl_mu;
    std::lock_guard<std::mutex> lock(tl_mu);
    if (FILE* f = fopen(timeline_path(), "ab")) {
      fwrite(tl.data(), 8, tl.size(), f);
      fclose(f);
    }
  }
  if (d_prof) {
    std::vector<uint64_t> pr(nq * 8);
    ISL_HIP(hipMemcpy(pr.data(), d_prof, nq * 64, hipMemcpyDeviceToHost));
    double sum[4] = {0, 0, 0, 0}, grp = 0, hr = 0;
    for (uint64_t i = 0; i < nq; i++) {
      for (int j = 0; j < 4; j++) sum[j] += pr[i * 8 + j] / 100.0;
      grp += pr[i * 8 + 4];
      hr += pr[i * 8 + 5];
    }
    fprintf(stderr, "[isl] per query: %.1f hops with new rows, %.1f distance passes of <= 16 rows\n", hr / nq,
            grp / nq);
    fprintf(stderr, "[isl] mean us per query by phase: select+adjacency %.0f, visited %.0f, rows+distance %.0f, "
            "insert %.0f\n", sum[0] / nq, sum[1] / nq, sum[2] / nq, sum[3] / nq);
  }
  if (!debug_on()) return ISL_OK;
  {
    std::vector<uint64_t> pay(nq);
    ISL_HIP(hipMemcpy(pay.data(), ws.payload, nq * 8, hipMemcpyDeviceToHost));
    std::vector<double> us;
    std::vector<std::pair<double, uint32_t>> byq;
    for (uint64_t i = 0; i < nq; i++)
      if (status[i] == QS_OK && pay[i]) { us.push_back(pay[i] / 100.0); byq.push_back({pay[i] / 100.0, ctr[i * 4]}); }
    std::sort(us.begin(), us.end());
    std::sort(byq.begin(), byq.end());
    if (!us.empty())
      fprintf(stderr, "[isl] per-query time in fast kernel (us): min %.0f p50 %.0f p90 %.0f p99 %.0f max %.0f; "
              "hops of slowest %u, of median %u; kernel %.0f us\n", us.front(), us[us.size() / 2],
              us[us.size() * 9 / 10], us[us.size() * 99 / 100], us.back(), byq.back().second,
              byq[byq.size() / 2].second, ms * 1000.0);
  }
  if (head[1] || head[3]) {
    fprintf(stderr, "[isl] %u of %llu queries re-run by the exact kernel (fast kernel %s): "
            "long-row %u, visited-overflow %u, tie-candidate overflow %u, push-log overflow %u, "
            "NaN/-0 distance %u; %u re-ordered by the replay kernel\n", head[1], (unsigned long long)nq,
            use_fast ? "on" : "off", head[9], head[10], head[11], head[8], head[12], head[3]);
  }
  return ISL_OK;
}
}  // namespace

// per-query failures -> the CoreError the reference's sequential map would have returned
isl_status isl_lane::search_statuses(isl::SearchWorkspace& ws, uint64_t nq) {
  const uint32_t* status = ws.h_status;
  for (uint64_t i = 0; i < nq; i++) {  // first failing query wins, like the sequential map
    if (status[i] == QS_OK) continue;
    if (status[i] == QS_NODE_NOT_FOUND) {
      uint64_t node = 0;
      const uint64_t* payload = ws.grp_launch ? ws.grp_launch->payload + ws.grp_offset : ws.payload;
      ISL_HIP(hipMemcpy(&node, payload + i, 8, hipMemcpyDeviceToHost));
      return isl::fail_node(node);
    }
    if (status[i] == QS_SCRATCH)
      return isl::fail(ISL_ERR_SEARCH, "Search error: device scratch exhausted for query %llu (candidate heap, "
                       "visited table or the two-level search's approximate-queue window)",
                       (unsigned long long)i);
    return isl::fail(ISL_ERR_SEARCH, "Search error: query %llu left in state 0x%x",
                     (unsigned long long)i, status[i]);
  }
  return ISL_OK;
}

namespace {

// The in-memory provider: enqueue + finish.  Two-level search: a query whose approximate queue outgrew the
// LDS window is never answered differently: the queries it happened to are run again, alone, with a window
// four times the size (plan.retry of them, plan.window_scale).
isl_status search_resident(const isl_index* idx, isl::SearchWorkspace& ws, const SearchCall& c) {
  const bool tl = c.two_level;
  RoundPlan plan;
  double ms_total = 0.0;
  for (;;) {
    ISL_TRY(search_enqueue(idx, ws, c, plan));
    plan.tables_built = tl;
    ISL_TRY(search_finish(idx, ws, nullptr, tl));
    if (!tl) return ISL_OK;  // (statuses evaluated by search_finish)
    ms_total += ws.stats.kernel_ms;
    uint32_t nshort = 0;
    ISL_TRY(tl_retry_short(ws, c.nq, plan.window_scale, &nshort));
    if (!nshort) break;
    plan.retry = nshort;
    copy_words(ws.h_qlist, ws.qlist, nshort, 16, 256, call_stream(ws, c));
    ISL_HIP(hipGetLastError());
  }
  ws.stats.kernel_ms = ms_total;
  return search_statuses(ws, c.nq);
}

}  // namespace

// One synchronous search on a claimed lane: by the index's provider.
isl_status isl_lane::search_sync(const isl_index* idx, isl::SearchWorkspace& ws, const SearchCall& c) {
  return idx->recompute ? recompute_rounds(idx, ws, c) : search_resident(idx, ws, c);
}

namespace {

// Checks shared by the entry points; *done = 1 when the call is already answered.
isl_status precheck(const isl_index* idx, uint64_t nq, uint64_t d, uint64_t k, uint32_t* out_count,
                    bool count_on_device, int* done) {
  *done = 0;
  if (!idx) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "index is NULL");
  if (nq == 0) { *done = 1; return ISL_OK; }
  if (idx->num_nodes == 0) {  // is_empty() -> Ok(vec![]), leann.rs:875-877
    if (out_count) {
      if (count_on_device) {
        if (idx->device >= 0) {
          ISL_TRY(isl::use_device(idx->device));
          ISL_HIP(hipMemset(out_count, 0, nq * 4));
        }
      } else {
        memset(out_count, 0, nq * 4);
      }
    }
    *done = 1;
    return ISL_OK;
  }
  if (idx->has_dimension && d != idx->dimension)  // leann.rs:880-887
    return isl::fail_dim(idx->dimension, d);
  if (!idx->has_entry) return isl::fail(ISL_ERR_INDEX_NOT_BUILT, "Index not built");  // :889
  if (idx->device < 0 || !idx->d_off)
    return isl::fail(ISL_ERR_DEVICE, "index is not resident on a device (isl_index_upload)");
  if (!idx->rows.resident())
    return isl::fail(ISL_ERR_EMBEDDING, "Embedding error: no embedding provider attached");
  if (d != idx->rows.d())  // metric.calculate length check, distance.rs:39-44
    return isl::fail_dim(d, idx->rows.d());
  if (k == 0) {
    *done = 2;  // nothing to write but counts
  }
  return ISL_OK;
}

isl_status precheck_two_level(const isl_index* idx, uint64_t d) {
  // (first: an index that holds fp8 rows gets this answer with or without PQ codes)
  if (idx->rows.is_fp8()) return isl::fail(ISL_ERR_UNSUPPORTED, "two-level search does not run over fp8 rows");
  if (!idx->pq || !idx->d_codes)
    return isl::fail(ISL_ERR_PQ, "PQ error: no PQ codes attached (isl_index_set_pq_codes)");
  if (idx->is_hnsw) return isl::fail(ISL_ERR_UNSUPPORTED, "two-level search runs on a LeannIndex");
  if (d != idx->pq->dimension) return isl::fail_dim(idx->pq->dimension, d);  // pq.rs:308-313
  return ISL_OK;
}

__global__ void check_codes_kernel(const uint16_t* __restrict__ codes, uint64_t n, uint32_t K,
                                   uint32_t* __restrict__ flag) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (; i < n; i += stride) bad |= codes[i] >= K;
  if (bad) atomicOr(flag, 1u);
}

// ---- lanes: claimed under idx->mu, then owned by the caller until released ----
isl::SearchWorkspace* claim_lane(const isl_index* idx) {
  std::lock_guard<std::mutex> lock(idx->mu);
  for (auto& w : idx->ws)
    if (!w.busy) {
      w.busy = true;
      w.waiting = false;
      w.threaded = false;
      w.enqueued = false;
      w.token = 0;
      w.alloc_mark = w.alloc_events;
      w.u_ids = nullptr; w.u_dist = nullptr; w.u_count = nullptr;
      w.publish_results = false;
      w.grp = false; w.grp_launch = nullptr; w.grp_offset = 0; w.grp_allocs = 0; w.grp_failed = false;
      return &w;
    }
  return nullptr;
}
void release_lane(const isl_index* idx, isl::SearchWorkspace& ws) {
  std::lock_guard<std::mutex> lock(idx->mu);
  ws.busy = false;
  ws.waiting = false;
  ws.token = 0;
}
isl_status no_lane() {
  return isl::fail(ISL_ERR_SEARCH, "Search error: %d searches already in flight; isl_search_wait one first",
                   isl::kSearchLanes);
}
// RAII: the lane goes back unless a token took it over
struct LaneGuard {
  const isl_index* idx;
  isl::SearchWorkspace* ws;
  ~LaneGuard() { if (ws) release_lane(idx, *ws); }
  void keep() { ws = nullptr; }
};

// What every entry point does first, in this order (which decides the error a bad call gets): the
// checks of the reference, those of the two-level search, the caller's buffers (host or device
// pointers, as the entry point received them), the device, a free lane.  *answered: nothing is
// left to do (no queries, an empty index) and no lane was claimed.
isl_status begin_call(const isl_index* idx, const SearchCall& c, bool count_on_device, isl::SearchWorkspace** ws,
                      bool* answered) {
  int done = 0;
  ISL_TRY(precheck(idx, c.nq, c.d, c.k, c.count, count_on_device, &done));
  *answered = done == 1;
  if (*answered) return ISL_OK;
  if (c.two_level) ISL_TRY(precheck_two_level(idx, c.d));
  if (!c.queries || !c.count || (c.k && (!c.ids || !c.dist)))
    return isl::fail(ISL_ERR_INVALID_ARGUMENT, "NULL buffer");
  ISL_TRY(isl::use_device(idx->device));
  *ws = claim_lane(idx);
  if (!*ws) return no_lane();
  return ISL_OK;
}
// the token an asynchronous call hands out for its lane
void issue_token(const isl_index* idx, isl::SearchWorkspace& ws, uint64_t* token) {
  std::lock_guard<std::mutex> lock(idx->mu);
  ws.token = idx->next_token++;
  *token = ws.token;
}
// Asynchronous calls that run their synchronous form on a worker thread (the rounds of the recompute
// provider, the two-level search with its retries): the lane's stream is made to wait for the
// caller's here, and the worker's call runs on the lane's stream alone.
isl_status order_after_user_stream(const isl_index* idx, isl::SearchWorkspace& ws, SearchCall& c) {
  ISL_TRY(ensure_lane_stream(idx, ws));
  ISL_HIP(hipEventRecord(ws.ev_in, c.user_stream));
  ISL_HIP(hipStreamWaitEvent(ws.stream, ws.ev_in, 0));
  c.user_stream = nullptr;
  c.mode = StreamMode::OWN;
  return ISL_OK;
}

// host-pointer calls: the queries go through the lane's pinned buffer, from where a kernel pulls
// them into HBM; the answers come back with the publish kernel (ws.publish_results)
isl_status host_stage_in(const isl_index* idx, isl::SearchWorkspace& ws, SearchCall& c) {
  ISL_TRY(prepare_host_staging(ws, c.nq, c.d, c.k));
  ISL_TRY(ensure_lane_stream(idx, ws));
  const uint64_t bytes = c.nq * c.d * 4;
  memcpy(ws.h_q, c.queries, bytes);
  if (bytes % 16 == 0)
    hipLaunchKernelGGL(copy_u128_kernel, dim3(256), dim3(256), 0, ws.stream, (const uint4*)ws.h_q.get(), (uint4*)ws.q_stage.get(),
                       bytes / 16);
  else
    hipLaunchKernelGGL(copy_u32_kernel, dim3(256), dim3(256), 0, ws.stream, (const uint32_t*)ws.h_q.get(),
                       (uint32_t*)ws.q_stage.get(), bytes / 4);
  ISL_HIP(hipGetLastError());
  ws.publish_results = true;
  // from here on the call runs over the lane's staging buffers, on the lane's stream
  c.queries = ws.q_stage;
  c.ids = ws.ids_stage;
  c.dist = ws.dist_stage;
  c.count = ws.count_stage;
  c.user_stream = nullptr;
  c.mode = StreamMode::OWN;
  return ISL_OK;
}
void host_copy_out(const isl::SearchWorkspace& ws, uint64_t nq, uint64_t k, uint64_t* out_ids, float* out_dist,
                   uint32_t* out_count) {
  if (k) {
    memcpy(out_ids, ws.h_ids, nq * k * 8);
    memcpy(out_dist, ws.h_dist, nq * k * 4);
  }
  memcpy(out_count, ws.h_count, nq * 4);
}

// Runs `body` (the synchronous form of a call, on the claimed lane `ws`) on a host thread; the
// token's wait joins it.  The thread selects the index's device first (the HIP device is per thread).
// Thread creation can fail (std::system_error, bad_alloc): nothing may cross the C ABI, so that is an
// ISL_ERR_DEVICE of the call and the lane goes back through the caller's LaneGuard; `threaded` is set
// only once the thread object exists.
template <typename F>
isl_status start_worker(const isl_index* idx, isl::SearchWorkspace* ws, F body) {
  ws->worker_status = ISL_OK;
  ws->threaded = false;
  std::thread* th = nullptr;
  try {
    th = new std::thread([idx, ws, body]() {
      isl_status st = isl::use_device(idx->device);
      try {  // nothing may leave the thread: an exception here would end the process
        if (st == ISL_OK) st = body();
      } catch (const std::exception& e) {
        st = isl::fail(ISL_ERR_SEARCH, "Search error: %s", e.what());
      } catch (...) {
        st = isl::fail(ISL_ERR_SEARCH, "Search error: unknown exception in the call's worker thread");
      }
      ws->worker_status = st;
      ws->worker_error = isl::last_error();
    });
  } catch (const std::exception& e) {
    return isl::fail(ISL_ERR_DEVICE, "the call's worker thread could not be started: %s", e.what());
  } catch (...) {
    return isl::fail(ISL_ERR_DEVICE, "the call's worker thread could not be started");
  }
  ws->worker = th;
  ws->threaded = true;
  return ISL_OK;
}
// true when the lane's call ran on a worker: *st = its status, the caller's error record = the worker's
bool join_worker(isl::SearchWorkspace& ws, isl_status* st) {
  if (!ws.threaded) return false;
  if (ws.worker) {
    ws.worker->join();
    delete ws.worker;
    ws.worker = nullptr;
  }
  ws.threaded = false;
  *st = ws.worker_status;
  if (*st != ISL_OK) isl::last_error() = ws.worker_error;
  return true;
}

}  // namespace

namespace isl {

void join_lane_workers(const isl_index* idx) {
  for (auto& w : idx->ws)
    if (w.worker) {
      w.worker->join();
      delete w.worker;
      w.worker = nullptr;
    }
}

bool any_lane_busy(const isl_index* idx) {
  for (const auto& w : idx->ws)
    if (w.busy) return true;
  return false;
}

void free_exact_pool(ExactPool& pl) { pl = ExactPool{}; }

// padded copy of the adjacency (64 ids per node + a degree array): 260 bytes per node buy the
// traversal one dependent memory round trip per hop.  Built where the CSR becomes resident
// (isl_index_upload, isl_index_from_device_csr, isl_index_prepare); the handle's fields are set
// only once the copy is complete.  Not enough memory -> the searches stay on the CSR.
isl_status ensure_padded_adjacency(isl_index* idx) {
  if (idx->d_ell || !idx->d_off || !idx->num_nodes || idx->max_degree > 128) return ISL_OK;
  const uint64_t n = idx->num_nodes;
  const uint32_t W = idx->max_degree > 64 ? 128u : 64u;
  DeviceBuffer<uint32_t> ell, deg;
  if (ell.reserve(n * W) != ISL_OK || deg.reserve(n) != ISL_OK) {
    (void)hipGetLastError();
    return ISL_OK;
  }
  hipLaunchKernelGGL(pad_rows_kernel, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, nullptr, idx->d_off, idx->d_adj, n,
                     W, ell, deg);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) return fail(ISL_ERR_DEVICE, "padded adjacency: %s", hipGetErrorString(e));
  idx->ell_copy = std::move(ell);
  idx->ell_deg_copy = std::move(deg);
  idx->d_ell = idx->ell_copy;
  idx->d_ell_deg = idx->ell_deg_copy;
  idx->ell_w = W;
  return ISL_OK;
}

// multi-GPU exchange (shard.hip): the queries of call `token` that did not end in QS_OK get
// ISL_SHARD_POISON_COUNT as their count in the rank's record, so that every rank's merge sees which
// answers are incomplete.  Enqueued on `stream`, which must already wait for the call's kernels
// (isl_search_stream_wait).  Calls that run on a worker thread are finished by then (the stream wait
// joined them), their status array is final as well.
__global__ void poison_failed_kernel(const uint32_t* __restrict__ status, uint32_t* __restrict__ counts, uint32_t nq) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nq && status[i] != QS_OK) counts[i] = ISL_SHARD_POISON_COUNT;
}
isl_status poison_failed_queries(const isl_index* idx, uint64_t token, uint32_t* d_counts, uint64_t nq, hipStream_t stream) {
  const uint32_t* status = nullptr;
  {
    std::lock_guard<std::mutex> lock(idx->mu);
    for (auto& w : idx->ws)
      if (w.busy && w.token == token) {
        status = w.grp_launch ? w.grp_launch->status + w.grp_offset : w.status;  // (a member of a group launch)
        break;
      }
  }
  if (!status) return fail(ISL_ERR_INVALID_ARGUMENT, "unknown or already completed search token");
  hipLaunchKernelGGL(poison_failed_kernel, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, stream, status, d_counts,
                     (uint32_t)nq);
  ISL_HIP(hipGetLastError());
  return ISL_OK;
}

isl_status search_device_sync(const isl_index* idx, const float* d_queries, uint64_t nq, uint64_t d,
                              uint64_t k, uint64_t ef, uint64_t* d_ids, float* d_dist,
                              uint32_t* d_count, hipStream_t stream) {
  SearchWorkspace* ws = claim_lane(idx);
  if (!ws) return no_lane();
  LaneGuard guard{idx, ws};
  return search_sync(idx, *ws, SearchCall{d_queries, nq, d, k, ef, d_ids, d_dist, d_count, stream, StreamMode::USER});
}

void add_last_allocations(const isl_index* idx, uint64_t events) {
  if (tl_last_stats.idx == idx) tl_last_stats.st.allocations += events;
}

}  // namespace isl

extern "C" {

isl_status isl_index_prepare(isl_index* idx, uint64_t max_nq, uint64_t max_ef, uint64_t max_k, int32_t lanes) {
  if (!idx) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "index is NULL");
  if (idx->device < 0 || !idx->d_off)
    return isl::fail(ISL_ERR_DEVICE, "index is not resident on a device (isl_index_upload)");
  if (!idx->rows.resident())
    return isl::fail(ISL_ERR_EMBEDDING, "Embedding error: no embedding provider attached");
  if (lanes < 1 || lanes > isl::kSearchLanes)
    return isl::fail(ISL_ERR_INVALID_ARGUMENT, "lanes must be 1..%d", isl::kSearchLanes);
  if (max_nq == 0 || max_nq > 0x7FFFFFFFull) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "max_nq out of range");
  max_ef = std::max<uint64_t>(std::max(max_ef, max_k), 1);
  if (max_ef > kMaxExactEf)
    return isl::fail(ISL_ERR_UNSUPPORTED, "ef = %llu exceeds the device limit %u", (unsigned long long)max_ef,
                     kMaxExactEf);
  ISL_TRY(isl::use_device(idx->device));
  const uint64_t d = idx->rows.d();
  {
    std::lock_guard<std::mutex> lock(idx->mu);
    if (isl::any_lane_busy(idx))
      return isl::fail(ISL_ERR_SEARCH, "Search error: isl_index_prepare while searches are in flight");
    ISL_TRY(isl::ensure_padded_adjacency(idx));
    ISL_TRY(ensure_pool(idx, idx->ws[0]));
    // the lanes are held for the duration: the last step exercises them together
    for (int i = 0; i < lanes; ++i) idx->ws[i].busy = true;
  }
  // a smaller ef puts more waves on a CU: size the per-wave overflow tables for the most there can be
  const uint32_t ovf_slots = (uint32_t)std::min<uint64_t>(max_nq, (uint64_t)isl::device_cu_count(idx->device) * kMaxWavesPerCu);
  CallGeometry cg_max;
  ISL_TRY(call_geometry(idx, d, max_k, max_ef, nullptr, cg_max));
  struct ReleaseAll {
    isl_index* idx; int lanes;
    ~ReleaseAll() { for (int i = 0; i < lanes; ++i) release_lane(idx, idx->ws[i]); }
  } release_all{idx, lanes};
  for (int i = 0; i < lanes; ++i) {
    isl::SearchWorkspace& ws = idx->ws[i];
    ISL_TRY(prepare_workspace(idx, ws, (uint32_t)max_nq, idx->recompute ? (uint32_t)max_nq : ovf_slots, cg_max.plog_cap));
    ISL_TRY(prepare_host_staging(ws, max_nq, d, std::max<uint64_t>(max_k, 1)));
    if (idx->recompute) ISL_TRY(prepare_recompute(ws, max_nq, cg_max.state_words));
    if (idx->is_hnsw) ISL_TRY(ws.q_entry.reserve(max_nq * 2, &ws.alloc_events));
    else if (idx->seeds.count()) ISL_TRY(ws.q_entry.reserve(max_nq * 4, &ws.alloc_events));  // entry, evals, packed minima
    if (idx->pq && idx->d_codes && !idx->is_hnsw && d == idx->pq->dimension)
      ISL_TRY(ws.tl_tables.reserve(max_nq * idx->pq->m * idx->pq->K, &ws.alloc_events));
    memset(ws.h_q, 0, max_nq * d * 4);
  }
  // The kernels this index will launch, over zero queries, and one staged copy each way, on all
  // lanes AT ONCE and twice over: code objects loaded, every stream's hardware queue and copy
  // queue up, the LDS opt-in attribute set, and the runtime's pools of completion signals grown to
  // what `lanes` calls in flight need (the runtime grows them one concurrent copy at a time, at
  // several milliseconds each -- measured inside the first calls otherwise).
  for (int round = 0; round < 2; ++round) {
    for (int i = 0; i < lanes; ++i) {
      isl::SearchWorkspace& ws = idx->ws[i];
      hipLaunchKernelGGL(copy_u128_kernel, dim3(256), dim3(256), 0, ws.stream, (const uint4*)ws.h_q.get(),
                         (uint4*)ws.q_stage.get(), max_nq * d * 4 / 16);
      const uint64_t efs[] = {max_ef, std::min<uint64_t>(max_ef, 64)};
      SearchCall warm_call;  // no queries, no buffers, on the lane's stream
      warm_call.d = d;
      for (uint64_t e : efs) {
        warm_call.k = std::min<uint64_t>(max_k, e);
        warm_call.ef = e;
        ISL_TRY(search_enqueue(idx, ws, warm_call, RoundPlan{}, true));
      }
      if (idx->pq && idx->d_codes && !idx->is_hnsw && !idx->rows.is_fp8() && d == idx->pq->dimension) {
        warm_call.k = std::min<uint64_t>(max_k, max_ef);
        warm_call.ef = max_ef;
        warm_call.two_level = true;
        warm_call.ratio = 0.5f;
        ISL_TRY(search_enqueue(idx, ws, warm_call, RoundPlan{}, true));
      }
      ws.publish_results = true;
      ISL_TRY(publish(ws, max_nq, std::max<uint64_t>(max_k, 1), ws.stream));
    }
    for (int i = 0; i < lanes; ++i) ISL_HIP(hipStreamSynchronize(idx->ws[i].stream));
  }
  for (int i = 0; i < lanes; ++i) idx->ws[i].alloc_mark = idx->ws[i].alloc_events;
  // the group workspaces beside the lanes (calls that find the chip full share launches: search_group.hip)
  ISL_TRY(group_prepare(idx, max_nq, max_ef, max_k, lanes,
                        (uint32_t)(isl::device_cu_count(idx->device) * kMaxWavesPerCu), cg_max.plog_cap));
  return ISL_OK;
}

// device-pointer entries: on the caller's stream; asynchronously on the lane's, behind the caller's
static isl_status search_batch_device(const isl_index* idx, const SearchCall& c) {
  isl::SearchWorkspace* ws = nullptr;
  bool answered = false;
  ISL_TRY(begin_call(idx, c, true, &ws, &answered));
  if (answered) return ISL_OK;
  LaneGuard guard{idx, ws};
  const isl_status st = search_sync(idx, *ws, c);
  note_last_stats(idx, ws->stats);
  return st;
}

static isl_status search_batch_device_async(const isl_index* idx, SearchCall c, uint64_t* token) {
  if (!token) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "token is NULL");
  *token = 0;
  isl::SearchWorkspace* ws = nullptr;
  bool answered = false;
  ISL_TRY(begin_call(idx, c, true, &ws, &answered));
  if (answered) return ISL_OK;  // token 0: nothing to wait for
  LaneGuard guard{idx, ws};
  if (idx->recompute || c.two_level) {
    // the provider works through the batch in rounds (search, encode what was missed, resume), the
    // two-level search retries queries: the synchronous form on a thread of its own, ordered after
    // the caller's stream
    ISL_TRY(order_after_user_stream(idx, *ws, c));
    ISL_TRY(start_worker(idx, ws, [=]() {
      return idx->recompute ? recompute_coalesced(idx, *ws, c) : search_sync(idx, *ws, c);
    }));
  } else if (group_takes(idx, c)) {
    ISL_TRY(group_arrive(idx, *ws, c));  // submitted now, or held for company (search_group_plan.hpp)
  } else {
    c.mode = StreamMode::OWN_AFTER_USER;
    ISL_TRY(search_enqueue(idx, *ws, c));
  }
  issue_token(idx, *ws, token);
  guard.keep();
  return ISL_OK;
}

isl_status isl_search_batch_device(const isl_index* idx, const float* d_queries, uint64_t nq,
                                   uint64_t d, uint64_t k, uint64_t ef, uint64_t* d_out_ids,
                                   float* d_out_dist, uint32_t* d_out_count, void* stream) {
  return search_batch_device(idx, SearchCall{d_queries, nq, d, k, ef, d_out_ids, d_out_dist, d_out_count,
                                             (hipStream_t)stream, StreamMode::USER});
}

isl_status isl_search_batch_device_async(const isl_index* idx, const float* d_queries, uint64_t nq,
                                         uint64_t d, uint64_t k, uint64_t ef, uint64_t* d_out_ids,
                                         float* d_out_dist, uint32_t* d_out_count, void* stream,
                                         uint64_t* token) {
  return search_batch_device_async(idx, SearchCall{d_queries, nq, d, k, ef, d_out_ids, d_out_dist, d_out_count,
                                                   (hipStream_t)stream, StreamMode::USER}, token);
}

isl_status isl_search_batch_async(const isl_index* idx, const float* queries, uint64_t nq, uint64_t d,
                                  uint64_t k, uint64_t ef, uint64_t* out_ids, float* out_dist,
                                  uint32_t* out_count, uint64_t* token) {
  if (!token) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "token is NULL");
  *token = 0;
  SearchCall c{queries, nq, d, k, ef, out_ids, out_dist, out_count};
  isl::SearchWorkspace* ws = nullptr;
  bool answered = false;
  ISL_TRY(begin_call(idx, c, false, &ws, &answered));
  if (answered) return ISL_OK;
  LaneGuard guard{idx, ws};
  ISL_TRY(host_stage_in(idx, *ws, c));
  if (idx->recompute) {
    ISL_HIP(hipEventRecord(ws->ev_in, ws->stream));  // the staged queries are there (a call that answers this one with its own waits for it)
    ISL_TRY(start_worker(idx, ws, [=]() { return recompute_coalesced(idx, *ws, c); }));
  } else {
    ISL_TRY(search_enqueue(idx, *ws, c));
  }
  ws->u_ids = out_ids;
  ws->u_dist = out_dist;
  ws->u_count = out_count;
  issue_token(idx, *ws, token);
  guard.keep();
  return ISL_OK;
}

isl_status isl_search_wait_stats(const isl_index* idx, uint64_t token, isl_search_stats* stats) {
  if (!idx) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "index is NULL");
  if (token == 0) {
    if (stats) *stats = isl_search_stats{};
    return ISL_OK;
  }
  ISL_TRY(isl::use_device(idx->device));
  isl::SearchWorkspace* ws = nullptr;
  {
    std::lock_guard<std::mutex> lock(idx->mu);
    for (auto& w : idx->ws)
      if (w.busy && w.token == token && !w.waiting) { ws = &w; w.waiting = true; break; }
  }
  if (!ws) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "unknown or already completed search token");
  LaneGuard guard{idx, ws};
  isl_status st = ISL_OK;
  const bool grouped = ws->grp;
  if (grouped) {  // a held call goes out now; whatever else the rules release goes with this entry
    st = group_before_wait(idx, *ws);
    if (st == ISL_OK) st = search_finish(idx, *ws);
    group_after_wait(idx, *ws);
  } else {
    group_pump(idx);
    if (!join_worker(*ws, &st)) st = search_finish(idx, *ws);  // the D2H result copies sit on the same stream
  }
  if (st == ISL_OK && ws->u_count) host_copy_out(*ws, ws->nq_inflight, ws->k_inflight, ws->u_ids, ws->u_dist, ws->u_count);
  if (stats) *stats = ws->stats;
  note_last_stats(idx, ws->stats);
  return st;
}

isl_status isl_search_wait(const isl_index* idx, uint64_t token) { return isl_search_wait_stats(idx, token, nullptr); }

isl_status isl_search_stream_wait(const isl_index* idx, uint64_t token, void* stream) {
  if (!idx) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "index is NULL");
  if (token == 0) return ISL_OK;
  ISL_TRY(isl::use_device(idx->device));
  isl::SearchWorkspace* found = nullptr;
  isl::SearchWorkspace* grouped = nullptr;
  {
    std::lock_guard<std::mutex> lock(idx->mu);
    for (auto& w : idx->ws)
      if (w.busy && w.token == token) {
        if (w.grp) { grouped = &w; break; }
        if (!w.threaded) {
          ISL_HIP(hipStreamWaitEvent((hipStream_t)stream, w.ev1, 0));  // recorded behind the last search kernel
          return ISL_OK;
        }
        if (!w.worker) return ISL_OK;  // already joined
        if (w.waiting) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "the call is being waited for on another thread");
        found = &w;
        w.waiting = true;  // (keeps isl_search_wait of another thread off the lane while we join)
        break;
      }
  }
  if (grouped) {
    // a call of the group path: submitted now if it is still held (its enqueue status stays with the lane for
    // isl_search_wait); `stream` then waits for the last kernel that writes its outputs
    if (group_before_wait(idx, *grouped) == ISL_OK) ISL_HIP(hipStreamWaitEvent((hipStream_t)stream, grouped->grp_ready, 0));
    return ISL_OK;
  }
  if (!found) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "unknown or already completed search token");
  // a call that runs on a worker thread (recompute provider, two-level search): its kernels are
  // enqueued round by round, so the host waits for the worker here; the call's status stays with the
  // lane for isl_search_wait
  found->worker->join();
  delete found->worker;
  found->worker = nullptr;
  {
    std::lock_guard<std::mutex> lock(idx->mu);
    found->waiting = false;
  }
  return ISL_OK;
}

// host-pointer entry: stage the queries, search on the lane's stream, copy the answers back
static isl_status search_batch_host(const isl_index* idx, SearchCall c) {
  uint64_t* const out_ids = c.ids;
  float* const out_dist = c.dist;
  uint32_t* const out_count = c.count;
  isl::SearchWorkspace* ws = nullptr;
  bool answered = false;
  ISL_TRY(begin_call(idx, c, false, &ws, &answered));
  if (answered) return ISL_OK;
  LaneGuard guard{idx, ws};
  ISL_TRY(host_stage_in(idx, *ws, c));
  const isl_status st = search_sync(idx, *ws, c);
  note_last_stats(idx, ws->stats);
  ISL_TRY(st);
  host_copy_out(*ws, c.nq, c.k, out_ids, out_dist, out_count);  // published with the last round's kernels
  return ISL_OK;
}

isl_status isl_search_batch(const isl_index* idx, const float* queries, uint64_t nq, uint64_t d,
                            uint64_t k, uint64_t ef, uint64_t* out_ids, float* out_dist,
                            uint32_t* out_count) {
  return search_batch_host(idx, SearchCall{queries, nq, d, k, ef, out_ids, out_dist, out_count});
}

// ---- two-level search with a PQ filter (extension, see leann_search_two_level) ----
isl_status isl_index_set_pq_codes(isl_index* idx, const isl_pq* pq, const uint16_t* codes, uint64_t n,
                                  int32_t mem) {
  if (!idx || !pq || (!codes && n)) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  if (n == 0) return isl::fail(ISL_ERR_EMPTY_COLLECTION, "Empty vector collection");
  if (idx->device < 0) return isl::fail(ISL_ERR_DEVICE, "call isl_index_upload before attaching PQ codes");
  if (pq->device != idx->device)
    return isl::fail(ISL_ERR_INVALID_ARGUMENT, "quantizer and index live on different devices");
  if (n > 0x7FFFFFFFull) return isl::fail(ISL_ERR_UNSUPPORTED, "more than 2^31 - 1 code rows");
  ISL_TRY(isl::use_device(idx->device));
  std::lock_guard<std::mutex> lock(idx->mu);
  if (isl::any_lane_busy(idx))
    return isl::fail(ISL_ERR_SEARCH, "Search error: PQ codes cannot be swapped while searches are in flight");
  idx->d_codes.reset();
  idx->pq = nullptr;
  idx->ncodes = 0;
  const size_t bytes = (size_t)n * pq->m * 2;
  isl::DeviceBuffer<uint16_t> d_codes;  // joins the index once checked
  isl::DeviceBuffer<uint32_t> d_flag;
  ISL_TRY(d_codes.reserve(n * pq->m));
  ISL_HIP(hipMemcpy(d_codes, codes, bytes, mem == ISL_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice));
  // tables[sq][code] of table_distance (pq.rs:345) would index out of bounds (panic) for a code >= K
  ISL_TRY(d_flag.reserve(1));
  ISL_HIP(hipMemset(d_flag, 0, 4));
  hipLaunchKernelGGL(check_codes_kernel, dim3(1024), dim3(256), 0, nullptr, d_codes.get(), (uint64_t)n * pq->m,
                     (uint32_t)pq->K, d_flag.get());
  uint32_t flag = 0;
  hipError_t e = hipMemcpy(&flag, d_flag, 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return isl::fail(ISL_ERR_DEVICE, "code check failed: %s", hipGetErrorString(e));
  if (flag) return isl::fail(ISL_ERR_PQ, "PQ error: a code is not below num_centroids = %llu", (unsigned long long)pq->K);
  idx->d_codes = std::move(d_codes);
  idx->pq = pq;
  idx->ncodes = n;
  return ISL_OK;
}

isl_status isl_search_two_level_batch(const isl_index* idx, const float* queries, uint64_t nq, uint64_t d,
                                      uint64_t k, uint64_t ef, float rerank_ratio, uint64_t* out_ids,
                                      float* out_dist, uint32_t* out_count) {
  return search_batch_host(idx, SearchCall{queries, nq, d, k, ef, out_ids, out_dist, out_count, nullptr,
                                           StreamMode::OWN, true, rerank_ratio});
}

isl_status isl_search_two_level_batch_device(const isl_index* idx, const float* d_queries, uint64_t nq,
                                             uint64_t d, uint64_t k, uint64_t ef, float rerank_ratio,
                                             uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count,
                                             void* stream) {
  return search_batch_device(idx, SearchCall{d_queries, nq, d, k, ef, d_out_ids, d_out_dist, d_out_count,
                                             (hipStream_t)stream, StreamMode::USER, true, rerank_ratio});
}

isl_status isl_search_two_level_batch_device_async(const isl_index* idx, const float* d_queries, uint64_t nq,
                                                   uint64_t d, uint64_t k, uint64_t ef, float rerank_ratio,
                                                   uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count,
                                                   void* stream, uint64_t* token) {
  return search_batch_device_async(idx, SearchCall{d_queries, nq, d, k, ef, d_out_ids, d_out_dist, d_out_count,
                                                   (hipStream_t)stream, StreamMode::USER, true, rerank_ratio}, token);
}

isl_status isl_search(const isl_index* idx, const float* query, uint64_t d, uint64_t k,
                      uint64_t* out_ids, float* out_dist, uint32_t* out_count) {
  if (!idx) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "index is NULL");
  return isl_search_batch(idx, query, 1, d, k, idx->cfg.ef_search, out_ids, out_dist,
                          out_count);  // leann.rs:858-865
}

isl_status isl_search_last_stats(const isl_index* idx, isl_search_stats* out) {
  if (!idx || !out) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  *out = tl_last_stats.idx == idx ? tl_last_stats.st : isl_search_stats{};
  return ISL_OK;
}

}  // extern "C"
