// Internal declarations shared by the translation units of libislands_amd.so.
// Nothing here is part of the ABI (see include/islands_amd.h for that).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/islands_amd.h"
#include "device_buffer.hpp"
#include "row_table.hpp"

namespace isl {

// ---- thread-local error record (CoreError payloads, src/core/error.rs:9-62) ----
struct ErrorRecord {
  std::string message;
  uint64_t expected = 0, actual = 0, node = 0;
};
ErrorRecord& last_error();
isl_status fail(isl_status st, const char* fmt, ...);
isl_status fail_dim(uint64_t expected, uint64_t actual);
isl_status fail_node(uint64_t node);

#define ISL_HIP(expr)                                                                   \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess)                                                               \
      return ::isl::fail(ISL_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr,                \
                         hipGetErrorString(_e), __FILE__, __LINE__);                    \
  } while (0)

#define ISL_TRY(expr)            \
  do {                           \
    isl_status _s = (expr);      \
    if (_s != ISL_OK) return _s; \
  } while (0)

// f(std::integral_constant<int, METRIC>{}) for the metric of a call: the one place a kernel template's
// metric argument is chosen at run time
template <class F>
void by_metric(uint32_t metric, F&& f) {
  switch (metric) {
    case ISL_METRIC_COSINE: f(std::integral_constant<int, ISL_METRIC_COSINE>{}); break;
    case ISL_METRIC_EUCLIDEAN: f(std::integral_constant<int, ISL_METRIC_EUCLIDEAN>{}); break;
    case ISL_METRIC_DOT: f(std::integral_constant<int, ISL_METRIC_DOT>{}); break;
    default: f(std::integral_constant<int, ISL_METRIC_MANHATTAN>{}); break;
  }
}

// Selects `device` after checking that it exists and is a gfx950 part.
isl_status use_device(int32_t device);
// compute units of a device use_device has verified (256 before that)
int device_cu_count(int32_t device);

// ---- per-index device workspace for the search kernels ----
// One lane = everything one search in flight needs: a stream, events, per-query device arrays,
// pinned host mirrors and (host-pointer entry points) staging buffers.  A lane is claimed under
// isl_index::mu and then touched by its owner alone until it is released, so the entry points do
// not hold the index mutex while they enqueue, wait or copy.
// Every array is a buffer that knows its capacity and frees itself with the lane.
struct SearchWorkspace {
  uint32_t slots = 0;          // resident waves the scratch is sized for
  uint32_t ovf_bits = 0;       // log2 entries of the per-slot overflow visited table
  DeviceBuffer<uint32_t> ovf_tab;  // [slots][1 << ovf_bits], EMPTY-filled between queries
  DeviceBuffer<uint32_t> status;  // one entry per query, at least 1024 (prepare_workspace)
  DeviceBuffer<uint64_t> payload;  // [status.capacity()]
  DeviceBuffer<uint32_t> ctr;     // [status.capacity()][4]  H,E,V,pushes
  DeviceBuffer<uint32_t> ticket;  // work-queue heads (fast, exact)
  DeviceBuffer<uint32_t> redo;    // [status.capacity()] query ids routed to the exact kernel
  DeviceBuffer<uint32_t> replay;  // [status.capacity()] query ids routed to the replay kernel
  DeviceBuffer<uint32_t> qsel;    // [status.capacity()] bf16 rows: queries whose elements are not all bf16 values
  DeviceBuffer<uint32_t> qsel_h;  // [status.capacity()] ... and the queries whose elements are
  DeviceBuffer<uint64_t> plog;    // [status.capacity()][plog_cap] push log (distance bits, id)
  // staging for the host-pointer entry points: device side ...
  DeviceBuffer<float> q_stage;
  DeviceBuffer<uint64_t> ids_stage;
  DeviceBuffer<float> dist_stage;
  DeviceBuffer<uint32_t> count_stage;
  // ... and pinned host side (the caller's buffers are pageable: copied through these)
  PinnedBuffer<float> h_q;
  PinnedBuffer<uint64_t> h_ids;
  PinnedBuffer<float> h_dist;
  PinnedBuffer<uint32_t> h_count;
  hipStream_t stream = nullptr;  // from the device's stream pool (search.hip): shared, never destroyed here
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_in = nullptr, ev_done = nullptr;
  float launch_ms = 0.0f;        // ev0 .. ev1 of the launch last enqueued here, once a wait has read it (search_finish)
  bool launch_ms_read = false;
  // call in flight on this lane (claim .. release)
  bool busy = false;           // under isl_index::mu
  bool waiting = false;        // a thread is inside isl_search_wait for this lane (under mu)
  bool enqueued = false;       // kernels of a call are on the stream (owner only)
  bool ticket_clean = false;   // the work-queue heads are (or will be, in stream order) zero
  bool publish_results = false; // host-buffer call: the publish kernel also brings the answers home
  uint64_t token = 0;
  uint64_t nq_inflight = 0, k_inflight = 0;
  uint32_t ef_inflight = 0;  // the effective ef (max(ef, k)) of the call in flight
  bool fast_inflight = false;
  hipStream_t st_inflight = nullptr;
  // host-pointer call in flight: where the answers go at wait time
  uint64_t* u_ids = nullptr;
  float* u_dist = nullptr;
  uint32_t* u_count = nullptr;
  PinnedBuffer<uint32_t> h_status;  // pinned host mirrors of status / ctr / ticket
  PinnedBuffer<uint32_t> h_ctr;
  PinnedBuffer<uint32_t> h_head;
  DeviceBuffer<uint64_t> d_prof;    // ISL_DEBUG phase timers of the call in flight
  DeviceBuffer<uint64_t> d_tline;   // ISL_TIMELINE: [nq][2] start / end ticks of every query of the call in flight
  DeviceBuffer<uint32_t> q_entry;   // HnswGraph: [2][nq] layer-0 entry and descent evaluations per query; an index
                                    // with entry seeds: [4][nq], the pick's packed 64-bit minima behind those two
  // recompute provider: the union of the calls this lane answers as one (search_recompute.hip, recompute_coalesced)
  DeviceBuffer<float> co_q;
  DeviceBuffer<uint64_t> co_ids;
  DeviceBuffer<float> co_dist;
  DeviceBuffer<uint32_t> co_cnt;
  // recompute provider: node ids whose rows a search round found absent, and their unique set
  DeviceBuffer<uint32_t> miss;
  DeviceBuffer<uint32_t> uniq;
  DeviceBuffer<uint32_t> uniq_count;
  uint64_t miss_cap = 0;
  uint64_t pref_cap = 0;         // entries behind miss[miss_cap]: ids a parked two-level query expects to promote next
  // ... and, for the searches that park and resume (fast kernel over the recompute provider): the
  // parked state of every query, its flag, the list of queries a round runs
  DeviceBuffer<uint32_t> qstate;    // [nq][state words of the call]
  DeviceBuffer<uint32_t> qflag;     // [qlist.capacity()]
  DeviceBuffer<uint32_t> qlist;     // [qlist.capacity()] device
  PinnedBuffer<uint32_t> h_qlist;   // [qlist.capacity()] pinned
  DeviceBuffer<uint32_t> uslots;    // [miss_cap] slab slots of the round's unique misses
  DeviceBuffer<uint32_t> xslot;     // [qlist.capacity()] 1 + pool slot of a query parked in the heap-exact kernel
  PinnedBuffer<uint32_t> h_xlist;   // [qlist.capacity()] pinned: the parked queries the next round hands to that kernel directly
  // two-level search: per-query PQ distance tables [nq][m * K]
  DeviceBuffer<float> tl_tables;
  // Asynchronous calls that cannot be split into "enqueue now, finish at wait" -- the rounds of the
  // recompute provider, the two-level search with its per-query retries -- run their synchronous form
  // on a host thread of their own; whoever waits for the token joins it and takes its status and
  // error record over.
  std::thread* worker = nullptr;
  bool threaded = false;         // the call in flight runs (or ran) on `worker`
  isl_status worker_status = ISL_OK;
  ErrorRecord worker_error;
  // device / pinned-host allocations, stream and event creations made for this lane so far: a
  // call's share of it is reported in isl_search_stats::allocations (0 after isl_index_prepare)
  uint64_t alloc_events = 0;
  uint64_t alloc_mark = 0;       // alloc_events when the call in flight was claimed
  isl_search_stats stats{};      // statistics of the call that finished last on this lane
  // ---- grouped launches (search_group.hip) ----
  // A lane whose call went in through the group path (all under the group state's mutex until the call's wait
  // has passed group_before_wait):
  bool grp = false;                        // the call is the group state's: held, or a member of a launch
  SearchWorkspace* grp_launch = nullptr;   // the group workspace whose launch answers it (NULL: held, or alone on this lane)
  uint32_t grp_offset = 0;                 // its first query in that launch's union
  hipEvent_t grp_ready = nullptr;          // recorded behind the last kernel that writes the call's outputs
  bool grp_marked = false;                 // ev_in is on the caller's stream: the call's launch waits for it
  uint64_t grp_allocs = 0;                 // what the launch's workspace had to set up (isl_search_stats::allocations)
  bool grp_failed = false;                 // the launch could not be enqueued: the wait returns grp_status / grp_error
  isl_status grp_status = ISL_OK;
  ErrorRecord grp_error;
  // A group workspace (never one of isl_index::ws):
  int32_t pool_lane = -1;                  // which stream of the device's pool it runs on (a lane: its own index)
  bool union_launch = false;               // search_enqueue leaves publishing to the group's scatter kernel
  PinnedBuffer<uint64_t> h_members;        // member table of the launch in flight, read by the gather / scatter kernels
  DeviceBuffer<uint32_t> grp_scratch;      // per-member counts and the scatter kernel's block counters (zero between launches)
};

constexpr int kSearchLanes = 32;  // independent workspaces = searches that may be in flight (on <= 16 pooled streams)

// GPU_MAX_HW_QUEUES as the process had it when the library was loaded; HIP's own default, 4, when it had none
// (api_index.hip: what the library sets itself at load comes too late once HIP has started, and cannot be told apart)
int hw_queues_at_load();
// Calls wait for company only where the hardware queues are the bottleneck.  With 32 queues the dispatcher
// already is the queue and holding calls back costs 2-7 % (profiles/search_group_ab.json, 32-queue leg); with four
// it gains 35-40 %.  Measured at 4 and at 32 only; in between, eight queues hold the eight launches that
// overlap at 32, so grouping is on below eight.
constexpr int kGroupBelowQueues = 8;
// ISL_NO_GROUP=1: no call waits for company (one launch per call, as before the group path existed), =0: calls do
// whatever the queues are, unset: by the queues; ISL_GROUP_CAP=<queries>: the most one launch takes;
// ISL_GROUP_ROOM=<queries>: stands in for the resident waves in "is there room on the chip" (small tests force
// holding with it).  0 = not set.  ISL_GROUP_MARK=1: every call of the group path puts its marker on the caller's
// stream, also where that stream has nothing pending (measurements: what the marker costs);
// ISL_GROUP_TRACE=1: one stderr line per arrival, launch and observed completion, with host clocks.
struct GroupSwitches { bool off; uint32_t cap, room; bool mark_always, trace; };
inline GroupSwitches group_switches() {
  auto num = [](const char* name) -> uint32_t {
    const char* e = getenv(name);
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (uint32_t)std::min<long long>(v, 0x7FFFFFFF) : 0u;
  };
  const char* off = getenv("ISL_NO_GROUP");
  const bool is_off = (off && *off) ? strcmp(off, "0") != 0 : hw_queues_at_load() >= kGroupBelowQueues;
  return GroupSwitches{is_off, num("ISL_GROUP_CAP"), num("ISL_GROUP_ROOM"), num("ISL_GROUP_MARK") != 0,
                       num("ISL_GROUP_TRACE") != 0};
}
struct GroupState;  // search_group.hip

// The inner answers of one refined search in flight (search_refine.hip): [nq][candidates] ids and distances, [nq]
// counts, and for the host-pointer form the staged queries and the final answers.
struct RefineScratch {
  bool busy = false;  // under isl_index::mu
  DeviceBuffer<uint64_t> ids;
  DeviceBuffer<float> dist;
  DeviceBuffer<uint32_t> count;
  DeviceBuffer<float> q_stage;
  DeviceBuffer<uint64_t> out_ids;
  DeviceBuffer<float> out_dist;
  DeviceBuffer<uint32_t> out_count;
};

// Scratch of the heap-exact kernel, ONE pool per index shared by every lane: a workgroup that
// finds work in its redo queue claims a free slot (lock word per slot), so concurrent searches
// do not need a private copy each.
struct ExactPool {
  uint32_t slots = 0;
  uint64_t cand_cap = 0;        // entries per slot in the candidate heap
  DeviceBuffer<float> cand_d;       // [slots][cand_cap]
  DeviceBuffer<uint32_t> cand_id;
  DeviceBuffer<uint32_t> vis_bits;  // [slots][vis_words] visited bitmap
  uint64_t vis_words = 0;
  DeviceBuffer<uint32_t> ulist;     // [slots][ulist_cap] unvisited ids of one hop
  uint32_t ulist_cap = 0;
  DeviceBuffer<uint32_t> locks;     // [slots] 0 = free, 1 = held by a workgroup (or by a query parked in the slot)
  DeviceBuffer<uint32_t> xstate;    // [slots][xstate_words] recompute provider: result heap + scalars of a parked query
  uint32_t xstate_words = 0;
};

}  // namespace isl

// ProductQuantizer (pq.rs:109-118) resident on a device: the codebooks.
struct isl_pq {
  uint64_t dimension = 0, m = 0, K = 0, dsub = 0, cstride = 0;
  int32_t metric = ISL_METRIC_EUCLIDEAN;
  int32_t device = 0;
  isl::DeviceBuffer<float> d_codebooks;  // [m][K][cstride], rows 16-byte aligned, slack at the end
};

// The opaque handle of the ABI.  Host side mirrors LeannIndex (leann.rs:492-500).
struct isl_index {
  isl_leann_config cfg{};
  // CsrGraph, leann.rs:193-208 (host copy; may be absent for device-born graphs)
  bool host_csr_valid = true;
  std::vector<uint64_t> node_offsets{0};
  std::vector<uint64_t> neighbors;
  std::vector<uint64_t> levels;
  std::vector<uint64_t> degree_counts;
  bool has_entry = false;
  uint64_t entry_point = 0;
  uint64_t max_level = 0;
  uint64_t num_nodes = 0;
  bool has_dimension = false;
  uint64_t dimension = 0;

  // device residency
  int32_t device = -1;
  isl::DeviceBuffer<uint64_t> d_off;  // [num_nodes + 1]
  isl::DeviceBuffer<uint32_t> d_adj;  // [nnz] (duplicates within a row removed, first occurrence kept)
  uint64_t nnz = 0;
  uint32_t max_degree = 0;
  // distance evaluations per query of the most recent in-memory search call and the ef it ran with, packed
  // (ef << 32 | evaluations; 0 = none yet): the size of the visited table of later calls WITH THAT ef follows it
  // (search.hip, fast_geometry)
  mutable std::atomic<uint64_t> evals_hint{0};
  // The embedding provider's rows.  In-memory provider (leann.rs:104-159): `rows` holds all nvec of them, f32 or
  // bf16.  Recompute provider: nvec is still the provider's length (the node count), while `rows` is the bounded
  // f32 slab indexed by SLOT -- rows.n() slots, the slab_rows of recompute_plan.hpp.
  isl::RowTable rows;
  uint64_t nvec = 0;
  // how often a row block was allocated for this handle (isl_index_capacity): a call that appends into or compacts
  // a reserved table leaves it as it is
  uint64_t row_allocations = 0;

  // entry seeds (entry_seeds.hip); empty by default
  isl::EntrySeeds seeds;

  // refine table and the scratch of the refined searches (search_refine.hip); empty by default.  One scratch set per
  // refined call in flight, claimed and released under `mu`, kept for the next call.
  isl::RefineTable refine;
  mutable std::vector<std::unique_ptr<isl::RefineScratch>> refine_scratch;

  // graph under construction (build.hip): fixed-width adjacency rows, searched in place
  uint32_t* d_ell = nullptr;      // [num_nodes][ell_w]: the builder's rows (borrowed) or ell_copy
  uint32_t* d_ell_deg = nullptr;  // [num_nodes]
  uint32_t ell_w = 0;
  isl::DeviceBuffer<uint32_t> ell_copy, ell_deg_copy;  // the padded copy made at the first search

  // HnswGraph under construction (hnsw_build.hip): [nq] entry node of every query of the next construction
  // search on the layer in d_ell, and the evaluations its counters start from (device arrays, borrowed);
  // nothing descends.  The builder hands in the descent's count for every layer: it does not read the
  // construction searches' counters, so they are not HnswGraph's running count below the first layer searched.
  uint32_t* build_q_entry = nullptr;
  uint32_t* build_q_evals = nullptr;

  // recompute provider (EmbeddingProvider backed by the encoder, leann.rs:82-99): embeddings are
  // not stored (leann.rs:366-371); the search reports the rows it misses and the provider encodes
  // them from the resident token table into a bounded row cache
  struct isl_encoder* enc = nullptr;   // borrowed
  isl::DeviceBuffer<uint16_t> d_tokens; // [nvec][tok_L]
  isl::DeviceBuffer<uint16_t> d_lens;   // [nvec] or NULL
  uint32_t tok_L = 0;
  // the rows live in a bounded slab (`rows`, indexed by SLOT): slot_of[id] = the node's
  // slot or 0xFFFFFFFF, owner[slot] = the node in it; slots are handed out round-robin, so the
  // oldest rows make room once the slab is full
  isl::DeviceBuffer<uint32_t> d_slot_of;    // [nvec]
  isl::DeviceBuffer<uint32_t> d_owner;      // [rows.n()]
  isl::DeviceBuffer<uint32_t> d_stamp;      // [rows.n()] round in which a row was last asked for
  isl::DeviceBuffer<uint32_t> d_slab_head;  // [1] where the clock hand of the slot allocator stands
  mutable uint32_t round_no = 1;       // rounds of recompute searches so far (under recompute_mu)
  bool recompute = false, keep_rows = false;
  int32_t enc_normalize = 1;

  // HnswGraph facade (hnsw.rs): distance-only heap order + upper layers for the greedy descent
  bool is_hnsw = false;
  uint64_t hnsw_layers = 0;
  isl::DeviceBuffer<const uint64_t*> d_layer_off;  // device array of device pointers, [max_level + 1]
  isl::DeviceBuffer<const uint32_t*> d_layer_adj;
  // the upper layers' arrays (u64 offsets and u32 ids alike), held as bytes only to be freed with the index
  std::vector<isl::DeviceBuffer<unsigned char>> hnsw_owned;

  // two-level search (extension): PQ codes of every node, [ncodes][pq->m] u16 as ProductQuantizer::encode
  // writes them (pq.rs:221-244); the quantizer is borrowed
  const isl_pq* pq = nullptr;
  isl::DeviceBuffer<uint16_t> d_codes;
  uint64_t ncodes = 0;

  mutable std::mutex mu;  // lane claims, the exact pool, index mutation -- never held across a search
  mutable std::mutex recompute_mu;  // searches over the recompute provider share its row table
  // asynchronous calls over the recompute provider that wait for their turn: the one that gets it answers every
  // compatible call waiting at that moment together with its own (search_recompute.hip, recompute_coalesced)
  struct RecJoin {
    std::mutex mu;        // guards `waiting`
    std::mutex leader;    // held by the call that is running the rounds
    std::vector<void*> waiting;
  };
  mutable RecJoin rec_join;
  mutable isl::SearchWorkspace ws[isl::kSearchLanes];
  mutable isl::ExactPool pool;
  mutable uint64_t next_token = 1;
  // grouped launches of asynchronous device-pointer calls (search_group.hip; rules: search_group_plan.hpp).
  // The switches are read when the handle is created; the state comes with the first such call or with
  // isl_index_prepare and goes with the handle.
  const isl::GroupSwitches group_sw = isl::group_switches();
  mutable std::mutex group_mu;              // guards `group` and everything in it; never taken under `mu`
  mutable isl::GroupState* group = nullptr;
};

// HnswGraph handle (hnsw.hip, hnsw_build.hip).
struct isl_hnsw {
  isl_index* core = nullptr;  // layer 0 + vectors + workspaces
  uint64_t m = 0, m0 = 0, ef_construction = 0;
  uint64_t dim = 0;
  double ml = 0.0;            // HnswConfig::ml / max_layers: carried for to_bytes and for isl_hnsw_insert
  uint64_t max_layers = 16;
  int32_t device = 0;         // where the graph lives, or where an empty one will once it takes rows
  // upper layers as the device holds them (host copies of the pointers in core->d_layer_off / d_layer_adj)
  std::vector<const uint64_t*> layer_off;
  std::vector<const uint32_t*> layer_adj;
  // host mirror of every layer in CSR form, read back on demand (get_neighbors, to_bytes)
  mutable std::mutex host_mu;
  mutable bool host_valid = false;
  mutable std::vector<std::vector<uint64_t>> h_off;
  mutable std::vector<std::vector<uint64_t>> h_adj;
};

namespace isl {
// One synchronous search over device buffers on a free lane (no argument checks): the path
// isl_search_batch_device takes, used by the graph builder for its construction searches.
isl_status search_device_sync(const isl_index* idx, const float* d_queries, uint64_t nq, uint64_t d,
                              uint64_t k, uint64_t ef, uint64_t* d_ids, float* d_dist,
                              uint32_t* d_count, hipStream_t stream);
// search.hip -- adds `events` to isl_search_stats::allocations of what isl_search_last_stats reports to this thread
// for `idx` (the refined search: the scratch it had to grow beside the inner search's own set-up)
void add_last_allocations(const isl_index* idx, uint64_t events);
// shard.hip: marks the queries of call `token` that failed with ISL_SHARD_POISON_COUNT in d_counts [nq]
isl_status poison_failed_queries(const isl_index* idx, uint64_t token, uint32_t* d_counts, uint64_t nq, hipStream_t stream);
isl_status materialise_host_csr(const isl_index* idx);
// api_index.hip -- the row table of a graph that grows: old's rows and norms copied on the device, then n_new
// rows of the same stored type (`dtype`) from `rows` (host or device, `mem`) and their norms; `idx` is a fresh
// construction graph
isl_status set_grown_embeddings(isl_index* idx, const isl_index* old, const void* rows, int32_t dtype, uint64_t n_new,
                                uint64_t d, int32_t mem);
// build_distance_tables (pq.rs:307-338) for nq device-resident queries into d_tables [nq][m][K]
isl_status pq_launch_tables(const isl_pq* pq, const float* d_queries, uint64_t nq, float* d_tables,
                            hipStream_t st);
// entry_seeds.hip -- the nearest seed of nq device-resident queries, enqueued on `st`: node ids into q_entry [nq] (with
// q_evals [nq] = 1 and status [nq] = QS_OK, what the traversal reads beside a given entry) and / or as u64 into
// d_out_ids; `packed` [nq] is scratch.  Nothing is launched for an index without seeds or for nq == 0.
isl_status launch_entry_pick(const isl_index* idx, const float* d_queries, uint64_t nq, uint32_t* q_entry,
                             uint32_t* q_evals, unsigned long long* packed, uint32_t* status, uint64_t* d_out_ids,
                             hipStream_t st);
// ... ISL_ENTRY_SEEDS=N after a successful build: selects N seeds for `idx` (unset or 0: nothing)
isl_status env_entry_seeds(isl_index* idx);
// ... what every call that makes a table asks of the handle first (`who` names the call in the message), and the
// table itself from checked ids (under idx->mu, no search in flight): graph_reach.hip installs its cover through these
isl_status check_seedable_index(const isl_index* idx, const char* who);
isl_status install_entry_seeds(isl_index* idx, const std::vector<uint64_t>& ids);
void free_workspace(SearchWorkspace& ws);
void free_exact_pool(ExactPool& pool);
// true while a search is in flight on any lane (call under idx->mu): provider / PQ setters and
// isl_index_free must not free tables such a search reads
bool any_lane_busy(const isl_index* idx);
// joins the host threads of asynchronous calls still running on the index's lanes (isl_index_free)
void join_lane_workers(const isl_index* idx);
// search_group.hip (isl_index_free, where idx->group is set): submits what is held, drains the group workspaces'
// streams and frees the state
void free_group_state(isl_index* idx);
// Builds the padded adjacency (64 ids per node + degrees) the traversal reads; under idx->mu.
isl_status ensure_padded_adjacency(isl_index* idx);
// hnsw.hip -- HnswConfig::validate (hnsw.rs:72-85) and the metric's range
isl_status hnsw_config_validate(uint64_t m, uint64_t m0, uint64_t ef_construction, int64_t metric);
// hnsw.hip -- the row types an HnswGraph stores, before any device call: f32 or bf16; fp8 -> ISL_ERR_UNSUPPORTED,
// anything else -> ISL_ERR_INVALID_ARGUMENT
isl_status hnsw_row_dtype(int32_t dtype);
// hnsw.hip -- the upper layers of a finished graph, device CSR arrays per layer (entry 0 unused: layer 0 is the
// core index): uploads the two pointer tables the descent reads and records them in `h`
isl_status attach_upper_layers(isl_hnsw* h, const std::vector<const uint64_t*>& offs,
                               const std::vector<const uint32_t*>& adjs);
}  // namespace isl
