// Recompute provider (EmbeddingProvider backed by the encoder, leann.rs:82-99): its row cache, the rounds
// that work a batch through the cache, and the coalescing of concurrent calls.  The rounds' host
// bookkeeping -- which queries a round runs, the caps -- is recompute_plan.hpp; the launches of a round are
// search_enqueue / search_finish of search.hip (search_internal.hpp).
#include "search_geometry.hpp"
#include "recompute_plan.hpp"
#include "search_internal.hpp"

using namespace isl_lane;

namespace {

// lists each missed id once: the first reporter of an id claims its slot-map entry
__global__ void dedupe_misses_kernel(const uint32_t* __restrict__ miss, uint32_t n,
                                     uint32_t* __restrict__ slot_of, uint32_t* __restrict__ uniq,
                                     uint32_t* __restrict__ uniq_count) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t id = miss[i];
  if (atomicCAS(&slot_of[id], kNoSlot, kSlotClaim) == kNoSlot) uniq[atomicAdd(uniq_count, 1u)] = id;
}

// Hands the round's unique misses their slab slots (one wave): once the slab is full a clock hand walks it and
// skips the rows some query asked for in this round (stamp == round) -- those belong to hops that
// are waiting for their last rows, evicting them would make the hop wait for THEM next round.  The
// node that held a slot before loses its row.  Ids left over when a full turn finds no more free
// slots are un-claimed and reported again next round.
__global__ __launch_bounds__(64) void assign_slots_kernel(const uint32_t* __restrict__ uniq,
                                                          const uint32_t* __restrict__ n_ptr,
                                                          uint32_t round_no, uint32_t slab_rows,
                                                          uint32_t* __restrict__ head_word,
                                                          uint32_t* __restrict__ slot_of, uint32_t* __restrict__ owner,
                                                          uint32_t* __restrict__ stamp, uint32_t* __restrict__ uslots,
                                                          uint32_t* __restrict__ taken, uint32_t quantum,
                                                          uint32_t chunk) {
  const uint32_t lane = threadIdx.x;
  // How many of the round's misses are encoded now: the encoder's GEMMs run whole waves of tiles over the
  // chip's CUs, and a batch that ends a little past a full wave pays for a whole one more (860 nodes x 64
  // tokens: 645 tiles of the hidden x hidden GEMMs = 2.52 waves on 256 CUs, 84 % of them filled).  So a
  // round takes whole encoder passes of `chunk` nodes plus a multiple of `quantum` nodes (the largest batch
  // whose narrowest GEMM still fits ONE wave of tiles), plus the rest when that rest nearly fills a wave
  // anyway; what is left over is un-claimed below and reported again next round, when it is batched with
  // that round's misses.  quantum == 0: everything (a provider whose shapes were not analysed).
  const uint32_t n_all = *n_ptr;
  uint32_t n = n_all;
  if (quantum && n >= quantum) {
    const uint32_t whole = chunk ? (n / chunk) * chunk : 0u, rem = n - whole;
    const uint32_t r = rem % quantum;
    n = whole + (rem - r) + (r * 10u >= quantum * 9u ? r : 0u);
  }
  // never-used slots first (head_word[1] counts them): nothing is evicted before the slab is full
  uint32_t fill = head_word[1], done = 0;
  {
    const uint32_t t = n < slab_rows - fill ? n : slab_rows - fill;
    for (uint32_t i = lane; i < t; i += 64) {
      const uint32_t id = uniq[i], s = fill + i;
      owner[s] = id;
      slot_of[id] = s;
      stamp[s] = round_no;
      uslots[i] = s;
    }
    done = t;
    fill += t;
  }
  uint32_t pos = *head_word % slab_rows, walked = 0;
  while (done < n && walked < slab_rows) {
    const uint32_t step = slab_rows - walked < 64u ? slab_rows - walked : 64u;
    const uint32_t s = (pos + lane) % slab_rows;
    const bool free_ = lane < step && stamp[s] != round_no;
    const uint64_t fm = ballot(free_);
    const uint32_t i = done + (uint32_t)__popcll(fm & ((1ull << lane) - 1ull));
    if (free_ && i < n) {
      const uint32_t id = uniq[i];
      const uint32_t old = owner[s];
      if (old != kNoSlot) slot_of[old] = kNoSlot;  // (never one of this round's ids: those were absent)
      owner[s] = id;
      slot_of[id] = s;
      stamp[s] = round_no;
      uslots[i] = s;
    }
    done += (uint32_t)__popcll(fm);
    pos = (pos + step) % slab_rows;
    walked += step;
  }
  if (done > n) done = n;
  for (uint32_t i = done + lane; i < n_all; i += 64) slot_of[uniq[i]] = kNoSlot;  // (the quantum's left-overs too)
  if (lane == 0) { head_word[0] = pos; head_word[1] = fill; *taken = done; }
}

// norm2[id] = sum_j row[id][j]^2 in the reference's order for the freshly encoded rows
__global__ __launch_bounds__(64) void row_norm2_list_kernel(const float* __restrict__ emb, uint64_t stride,
                                                            uint32_t d, const uint32_t* __restrict__ ids,
                                                            uint32_t n, float* __restrict__ norm2) {
  extern __shared__ __align__(16) unsigned char smem[];
  float* tile = reinterpret_cast<float*>(smem);
  const uint32_t lane = threadIdx.x;
  for (uint32_t base = blockIdx.x * 64; base < n; base += gridDim.x * 64) {
    const uint32_t R = n - base < 64 ? n - base : 64;
    const uint32_t uid = lane < R ? ids[base + lane] : 0u;
    const float v = wave_distances<METRIC_SUMSQ_RAW>(emb, stride, d, uid, R, tile, tile, 0.f);
    if (lane < R) norm2[uid] = v;
  }
}

constexpr uint32_t kTlPrefetchDefault = 0;  // (set from the measurement: DESIGN.md section 3.4)

// query lists of a lane (rounds of the recompute provider, retries of the two-level search)
isl_status ensure_qlist(isl::SearchWorkspace& ws, uint64_t nq) {
  uint64_t* const ev = &ws.alloc_events;
  const uint64_t c = nq < 1024 ? 1024 : nq;
  ISL_TRY(ws.qflag.reserve(c, ev));
  ISL_TRY(ws.qlist.reserve(c, ev));
  ISL_TRY(ws.xslot.reserve(c, ev));
  ISL_TRY(ws.h_qlist.reserve(c, ev));
  return ws.h_xlist.reserve(c, ev);
}

// Two-level search: the queries of the finished launch whose approximate-queue window was too small
// (QS_SCRATCH with payload 7) -> ws.h_qlist[0, *count).
isl_status tl_collect_short(isl::SearchWorkspace& ws, uint64_t nq, uint32_t* count) {
  *count = 0;
  bool any = false;
  for (uint64_t i = 0; i < nq && !any; ++i) any = ws.h_status[i] == QS_SCRATCH;
  if (!any) return ISL_OK;
  ISL_TRY(ensure_qlist(ws, nq));
  std::vector<uint64_t> pay(nq);
  ISL_HIP(hipMemcpy(pay.data(), ws.payload, nq * 8, hipMemcpyDeviceToHost));
  uint32_t n = 0;
  for (uint64_t i = 0; i < nq; ++i)
    if (ws.h_status[i] == QS_SCRATCH && pay[i] == 7) ws.h_qlist[n++] = (uint32_t)i;
  *count = n;
  return ISL_OK;
}

}  // namespace

namespace isl_lane {

// Two-level search, every query of the call has run to its end: those whose queue window was too small are
// listed in ws.h_qlist[0, *nshort) and the window grows for them (recompute_plan.hpp, grow_window).
// *nshort = 0: there are none, or the window is as large as it gets -- the statuses stand.
isl_status tl_retry_short(isl::SearchWorkspace& ws, uint64_t nq, uint32_t& window_scale, uint32_t* nshort) {
  *nshort = 0;
  uint32_t n = 0;
  ISL_TRY(tl_collect_short(ws, nq, &n));
  if (n && isl_rounds::grow_window(window_scale)) *nshort = n;
  return ISL_OK;
}

isl_status prepare_recompute(isl::SearchWorkspace& ws, uint64_t nq, uint64_t state_words_per_query) {
  const uint64_t cap = isl_rounds::miss_capacity(nq);
  const uint64_t pcap = isl_rounds::prefetch_capacity(nq);
  if (ws.miss_cap < cap || ws.pref_cap < pcap) {
    // the prefetch ids sit behind miss[miss_cap]: a new split means new arrays
    ws.miss.reset(); ws.uniq.reset(); ws.uslots.reset(); ws.uniq_count.reset();
    ws.miss_cap = 0;
    ws.pref_cap = 0;
    uint64_t* const ev = &ws.alloc_events;
    ISL_TRY(ws.miss.reserve(cap + pcap, ev));
    ISL_TRY(ws.uniq.reserve(cap + pcap, ev));
    ISL_TRY(ws.uslots.reserve(cap + pcap, ev));
    ISL_TRY(ws.uniq_count.reserve(1, ev));
    ws.miss_cap = cap;
    ws.pref_cap = pcap;
  }
  ISL_TRY(ensure_qlist(ws, nq));
  return ws.qstate.reserve(std::max<uint64_t>(nq, 1) * state_words_per_query, &ws.alloc_events);
}

}  // namespace isl_lane

namespace {

// The row cache and the parking state as a batch finds them, on the call's stream.
isl_status begin_batch(const isl_index* idx, isl::SearchWorkspace& ws, const SearchCall& c, hipStream_t st) {
  if (!idx->keep_rows) {  // every call starts from an empty cache: each node is encoded once per call
    ISL_HIP(hipMemsetAsync(idx->d_slot_of, 0xFF, (idx->nvec + 1) * 4, st));
    ISL_HIP(hipMemsetAsync(idx->d_owner, 0xFF, idx->rows.n() * 4, st));
    ISL_HIP(hipMemsetAsync(idx->d_stamp, 0, idx->rows.n() * 4, st));
    ISL_HIP(hipMemsetAsync(idx->d_slab_head, 0, 8, st));
  }
  ISL_HIP(hipMemsetAsync(ws.qflag, 0, c.nq * 4, st));
  ISL_HIP(hipMemsetAsync(ws.xslot, 0, c.nq * 4, st));
  if (!c.two_level) {
    // no query is parked in the heap-exact kernel's pool yet (recompute calls run one at a time per index)
    if (!idx->pool.slots) {
      std::lock_guard<std::mutex> lock(idx->mu);
      ISL_TRY(ensure_pool(idx, ws));
    }
    ISL_HIP(hipMemsetAsync(idx->pool.locks, 0, (size_t)idx->pool.slots * 4, st));
  }
  return ISL_OK;
}

struct RoundReset {  // no slot of the heap-exact kernel's pool stays with a query of this call whatever happens below
  const isl_index* idx;
  hipStream_t st;
  ~RoundReset() {
    if (idx->pool.slots && idx->pool.locks) {
      (void)hipMemsetAsync(idx->pool.locks, 0, (size_t)idx->pool.slots * 4, st);
      (void)hipStreamSynchronize(st);
    }
  }
};

// How the misses of a round are batched for the encoder, and what a parked two-level query names beyond them.
struct EncodePolicy {
  uint32_t quantum = 0, chunk = 0;  // assign_slots_kernel
  uint32_t prefetch = 0;
};
EncodePolicy encode_policy(const isl_index* idx, bool tl, uint32_t in_flight) {
  EncodePolicy e;
  // encoder batches in whole waves of GEMM tiles (assign_slots_kernel; ISL_RECOMPUTE_QUANTUM=0: every miss at once)
  isl::encoder_batch_quantum(idx->enc, idx->tok_L, &e.quantum, &e.chunk);
  if (const char* qe = getenv("ISL_RECOMPUTE_QUANTUM")) e.quantum = (uint32_t)std::max(0, atoi(qe));  // (read per call: A/B in one process)
  // Two-level search: a parked query also names the nodes it expects to promote next (tl_prefetch of them), which
  // are encoded in the same round -- fewer, fuller rounds.  Only with a slab that has room to spare (the names are
  // guesses: under a small cache they would push out rows that hops are waiting for).  ISL_TL_PREFETCH=n overrides
  // (0 = off; read per call).
  e.prefetch = (tl && idx->rows.n() >= (uint64_t)1024 * std::max<uint32_t>(1u, in_flight)) ? kTlPrefetchDefault : 0u;
  if (const char* pe = getenv("ISL_TL_PREFETCH")) e.prefetch = tl ? (uint32_t)std::min(8, std::max(0, atoi(pe))) : 0u;
  return e;
}

// Slab slots for the rows a round missed: each id once, the guesses behind the misses; *take rows were placed
// (ws.uniq, ws.uslots).  Waits for the stream.
isl_status place_misses(const isl_index* idx, isl::SearchWorkspace& ws, hipStream_t st, uint32_t misses,
                        uint32_t guesses, const EncodePolicy& enc, uint32_t* take) {
  uint32_t* h_taken = ws.h_head + 15;  // (word 15 of the pinned ticket mirror is otherwise unused)
  if (misses > ws.miss_cap) misses = (uint32_t)ws.miss_cap;
  ISL_HIP(hipMemsetAsync(ws.uniq_count, 0, 4, st));
  hipLaunchKernelGGL(dedupe_misses_kernel, dim3((misses + 255) / 256), dim3(256), 0, st, ws.miss, misses,
                     idx->d_slot_of, ws.uniq, ws.uniq_count);
  // the guesses go behind the misses in the unique list: what a full slab or the quantum leaves out is theirs first
  if (guesses)
    hipLaunchKernelGGL(dedupe_misses_kernel, dim3((guesses + 255) / 256), dim3(256), 0, st, ws.miss + ws.miss_cap, guesses,
                       idx->d_slot_of, ws.uniq, ws.uniq_count);
  // slots for the new rows (clock hand over the slab; rows asked for in this round stay)
  hipLaunchKernelGGL(assign_slots_kernel, dim3(1), dim3(64), 0, st, ws.uniq, ws.uniq_count, idx->round_no,
                     (uint32_t)idx->rows.n(), idx->d_slab_head, idx->d_slot_of, idx->d_owner, idx->d_stamp,
                     ws.uslots, ws.ticket + 15, enc.quantum, enc.chunk);
  ISL_HIP(hipGetLastError());
  copy_words(ws.ticket + 15, h_taken, 1, 1, 64, st);
  ISL_HIP(hipStreamSynchronize(st));
  *take = *h_taken;
  return ISL_OK;
}

// The placed rows: encoded into their slots, and their norms.
isl_status encode_rows(const isl_index* idx, isl::SearchWorkspace& ws, hipStream_t st, uint32_t take) {
  ISL_TRY(isl::encoder_embed_nodes(idx->enc, idx->d_tokens, idx->d_lens, idx->tok_L, ws.uniq, take,
                                   idx->enc_normalize, idx->rows.f32(), idx->rows.stride(), st, ws.uslots));
  const size_t lds = (size_t)TILE_ROWS * TILE_LD * 4 + 64;
  if (take)
    hipLaunchKernelGGL(row_norm2_list_kernel, dim3(std::min<uint32_t>((take + 63) / 64, 4096)), dim3(64), lds, st,
                       idx->rows.f32(), idx->rows.stride(), (uint32_t)idx->rows.d(), ws.uslots, take, idx->rows.norm2());
  ISL_HIP(hipGetLastError());
  return ISL_OK;
}

}  // namespace

namespace isl_lane {

// Rounds of (search; every query that needs an absent row reports it and stops) -> (encode the reported nodes
// once each) until a round completes without a miss; that last round is an ordinary search over materialised
// rows, so ids, distances, counters and error behaviour are those of the in-memory provider holding the same
// embeddings.
isl_status recompute_rounds(const isl_index* idx, isl::SearchWorkspace& ws, const SearchCall& c) {
  using isl_rounds::Verdict;
  const uint64_t nq = c.nq;
  const bool tl = c.two_level;
  // the rounds rewrite the provider's row cache: one recompute search at a time
  std::lock_guard<std::mutex> rlock(idx->recompute_mu);
  CallGeometry cg0;
  {
    const TwoLevelCall tl0{c.ratio};
    ISL_TRY(call_geometry(idx, c.d, c.k, c.ef, tl ? &tl0 : nullptr, cg0));
  }
  const bool x_park = !tl && idx->rows.n() < idx->nvec;
  const isl_rounds::Kind kind = isl_rounds::batch_kind(tl, cg0.use_fast, x_park);
  ISL_TRY(prepare_recompute(ws, nq, kind == isl_rounds::Kind::PARK ? cg0.state_words : 1));  // (the heap-exact kernel parks in the pool)
  ISL_TRY(ensure_lane_stream(idx, ws));
  hipStream_t st = call_stream(ws, c);
  ISL_TRY(begin_batch(idx, ws, c, st));
  const uint32_t in_flight = isl_rounds::max_in_flight(nq, idx->rows.n(), idx->nvec, tl, idx->max_degree);
  isl_rounds::RoundScheduler sched(kind, tl, (uint32_t)nq, in_flight, ws.h_qlist.get(), ws.h_xlist.get());
  sched.first();
  if (sched.listed() && sched.active()) copy_words(ws.h_qlist, ws.qlist, sched.active(), 16, 256, st);
  RoundReset reset{idx, st};
  const EncodePolicy enc = encode_policy(idx, tl, in_flight);
  const uint64_t max_rounds = isl_rounds::max_rounds(nq, in_flight, cg0.ef);
  RoundPlan plan;
  plan.exact_parks = x_park;
  plan.prefetch = enc.prefetch;
  uint64_t encoded = 0, rounds = 0;
  double kernel_ms = 0.0;
  uint32_t stalled = 0;
  for (;;) {
    // launch the round and finish it
    plan.active = sched.active();
    plan.exact = sched.exact();
    plan.listed = sched.listed();
    idx->round_no += 1;
    ISL_TRY(search_enqueue(idx, ws, c, plan));
    plan.tables_built = tl;
    uint32_t misses = 0;
    ISL_TRY(search_finish(idx, ws, &misses, true));
    const uint32_t guesses = enc.prefetch ? std::min<uint32_t>(ws.h_head[14], (uint32_t)ws.pref_cap) : 0u;
    kernel_ms += ws.stats.kernel_ms;
    rounds += 1;
    // the next round's lists
    Verdict v = sched.next(ws.h_status, misses);
    if (v == Verdict::SHORT_WINDOWS) {
      // the short-window queries start over with a window four times the size (and a state block to match)
      uint32_t nshort = 0;
      ISL_TRY(tl_retry_short(ws, nq, plan.window_scale, &nshort));
      if (nshort) {
        const TwoLevelCall tl1{c.ratio, plan.window_scale};
        CallGeometry cg1;
        ISL_TRY(call_geometry(idx, c.d, c.k, c.ef, &tl1, cg1));
        ISL_TRY(ws.qstate.reserve(std::max<uint64_t>(nq, 1) * cg1.state_words, &ws.alloc_events));
      }
      v = sched.restart_short(nshort);
    }
    if (v == Verdict::FINAL) {  // now the statuses are final
      ISL_TRY(search_statuses(ws, nq));
      break;
    }
    if (sched.active()) copy_words(ws.h_qlist, ws.qlist, sched.active(), 16, 256, st);
    if (rounds > max_rounds)
      return isl::fail(ISL_ERR_SEARCH, "Search error: %llu recompute rounds without completing the batch (row cache "
                       "%llu rows, %u queries in flight at a time)", (unsigned long long)rounds,
                       (unsigned long long)idx->rows.n(), in_flight);
    if (!misses) continue;  // only fresh queries to start
    // place the misses, encode them, take their norms
    uint32_t take = 0;
    ISL_TRY(place_misses(idx, ws, st, misses, guesses, enc, &take));
    // no row could be placed although rows are missing: every slot is held by a hop of this round
    if (take == 0 && ++stalled >= isl_rounds::stall_limit(kind))
      return isl::fail(ISL_ERR_SEARCH, "Search error: the recompute provider's row cache (%llu rows) is too small "
                       "for this batch (no missing row could be placed)", (unsigned long long)idx->rows.n());
    if (take) stalled = 0;
    ISL_TRY(encode_rows(idx, ws, st, take));
    encoded += take;
  }
  ws.stats.encoded_nodes = encoded;
  ws.stats.recompute_rounds = rounds;
  ws.stats.kernel_ms = kernel_ms;
  ws.stats.allocations = ws.alloc_events - ws.alloc_mark;
  return ISL_OK;
}

// ---- concurrent asynchronous calls over the recompute provider, answered together ----
// Calls over the recompute provider run one at a time per index (the rounds rewrite the provider's row cache).
// A caller that keeps several batches in flight therefore used to get them answered one after the other, each
// with its own small encoder passes -- where ONE call over all their queries encodes a node once for all of
// them and hands the encoder fuller passes (8 x 1024 queries at 10M nodes: 89.0 against 74.9 queries/s,
// DESIGN.md section 3.4).  So the asynchronous device-buffer calls queue here: the call whose turn it is takes
// every compatible call (same d, k, ef, search kind, re-rank ratio) that is waiting at that moment, runs the
// rounds ONCE over the union of their queries on its own lane, and scatters the answers; the others wake up
// answered.  Every query's answer is what its own call would have computed (a query's traversal does not
// depend on what else is in the batch).  If the union fails -- one query's NodeNotFound fails the call it
// belongs to, not its neighbours' -- every member is run by itself and gets its own status.
struct RecCall {
  SearchCall call;  // (on the member's own lane's stream: StreamMode::OWN)
  isl::SearchWorkspace* ws;
  bool done = false;
  isl_status status = ISL_OK;
  isl::ErrorRecord err;
};

isl_status recompute_coalesced(const isl_index* idx, isl::SearchWorkspace& ws, const SearchCall& c) {
  static const bool off = getenv("ISL_NO_RECOMPUTE_COALESCE") != nullptr;  // A/B switch for measurements
  if (off) return search_sync(idx, ws, c);
  const uint64_t d = c.d, k = c.k;
  RecCall me{c, &ws};
  auto& J = idx->rec_join;
  {
    std::lock_guard<std::mutex> l(J.mu);
    J.waiting.push_back(&me);
  }
  std::unique_lock<std::mutex> lead(J.leader);
  if (me.done) {  // answered by the call that had the turn before
    if (me.status != ISL_OK) isl::last_error() = me.err;
    return me.status;
  }
  constexpr uint64_t kMaxUnion = 1u << 17;  // queries one set of rounds works through
  std::vector<RecCall*> group{&me};
  uint64_t total = c.nq;
  {
    std::lock_guard<std::mutex> l(J.mu);
    std::vector<void*> rest;
    for (void* v : J.waiting) {
      RecCall* m = static_cast<RecCall*>(v);
      if (m == &me) continue;
      const SearchCall& o = m->call;
      const bool same = o.d == d && o.k == k && o.ef == c.ef && o.two_level == c.two_level && (!c.two_level || o.ratio == c.ratio);
      if (same && total + o.nq <= kMaxUnion) { group.push_back(m); total += o.nq; }
      else rest.push_back(v);
    }
    J.waiting.swap(rest);
  }
  if (group.size() == 1) return search_sync(idx, ws, c);

  auto alone = [&](RecCall* m) {  // the member's own call, on the member's own lane
    m->status = search_sync(idx, *m->ws, m->call);
    if (m->status != ISL_OK) m->err = isl::last_error();
  };
  auto fall_back = [&]() -> isl_status {  // every member by itself: its own answers, its own error
    for (RecCall* m : group)
      if (m != &me) { alone(m); m->done = true; }
    return search_sync(idx, ws, c);
  };
  uint64_t* const ev = &ws.alloc_events;
  if (ws.co_q.reserve(total * d, ev) != ISL_OK || ws.co_ids.reserve(total * std::max<uint64_t>(k, 1), ev) != ISL_OK ||
      ws.co_dist.reserve(total * std::max<uint64_t>(k, 1), ev) != ISL_OK || ws.co_cnt.reserve(total, ev) != ISL_OK ||
      ensure_lane_stream(idx, ws) != ISL_OK)
    return fall_back();
  hipStream_t st = ws.stream;
  uint64_t o = 0;
  bool copied = true;
  for (RecCall* m : group) {  // a member's queries are there once its caller's stream has reached the call (ev_in)
    if (m != &me) copied = copied && hipStreamWaitEvent(st, m->ws->ev_in, 0) == hipSuccess;
    copied = copied && hipMemcpyAsync(ws.co_q + o * d, m->call.queries, m->call.nq * d * 4, hipMemcpyDeviceToDevice, st) == hipSuccess;
    o += m->call.nq;
  }
  if (!copied) { (void)hipStreamSynchronize(st); (void)hipGetLastError(); return fall_back(); }
  // (a host-buffer call's lane publishes its answers into pinned mirrors sized for THAT call: not for the union)
  const bool publishes = ws.publish_results;
  ws.publish_results = false;
  SearchCall all_calls = c;  // the union: every member's queries, answered into the lane's own buffers
  all_calls.queries = ws.co_q;
  all_calls.nq = total;
  all_calls.ids = ws.co_ids;
  all_calls.dist = ws.co_dist;
  all_calls.count = ws.co_cnt;
  const isl_status rc = search_sync(idx, ws, all_calls);
  ws.publish_results = publishes;
  if (rc != ISL_OK) return fall_back();
  const isl_search_stats all = ws.stats;
  o = 0;
  bool scattered = true;
  for (RecCall* m : group) {
    const uint64_t mq = m->call.nq;
    if (k) {
      scattered = scattered && hipMemcpyAsync(m->call.ids, ws.co_ids + o * k, mq * k * 8, hipMemcpyDeviceToDevice, st) == hipSuccess;
      scattered = scattered && hipMemcpyAsync(m->call.dist, ws.co_dist + o * k, mq * k * 4, hipMemcpyDeviceToDevice, st) == hipSuccess;
    }
    scattered = scattered && hipMemcpyAsync(m->call.count, ws.co_cnt + o, mq * 4, hipMemcpyDeviceToDevice, st) == hipSuccess;
    if (m->ws->publish_results) {  // a host-buffer call (isl_search_batch_async): its wait copies out of the lane's pinned mirrors
      if (k) {
        scattered = scattered && hipMemcpyAsync(m->ws->h_ids, ws.co_ids + o * k, mq * k * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
        scattered = scattered && hipMemcpyAsync(m->ws->h_dist, ws.co_dist + o * k, mq * k * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
      }
      scattered = scattered && hipMemcpyAsync(m->ws->h_count, ws.co_cnt + o, mq * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
      m->ws->nq_inflight = mq;
      m->ws->k_inflight = k;
    }
    o += mq;
  }
  scattered = scattered && hipStreamSynchronize(st) == hipSuccess;
  if (!scattered) { (void)hipGetLastError(); return fall_back(); }
  // each member's counters are its own queries' (the lane's pinned mirror holds the union's, query by query);
  // rounds, encoded nodes and kernel time are the union's
  o = 0;
  for (RecCall* m : group) {
    isl_search_stats ms = all;
    ms.queries = m->call.nq;
    ms.expansions = ms.edges = ms.evals = ms.pushes = 0;
    for (uint64_t i = o; i < o + m->call.nq; ++i) {
      ms.expansions += ws.h_ctr[i * 4 + 0];
      ms.edges += ws.h_ctr[i * 4 + 1];
      ms.evals += ws.h_ctr[i * 4 + 2];
      ms.pushes += ws.h_ctr[i * 4 + 3];
    }
    m->ws->stats = ms;
    o += m->call.nq;
    if (m != &me) { m->status = ISL_OK; m->done = true; }
  }
  return ISL_OK;
}

}  // namespace isl_lane
