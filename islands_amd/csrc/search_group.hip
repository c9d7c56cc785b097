// Grouped launches: asynchronous device-pointer calls that find the chip full share one launch.
//
// The rules (who may share, when a call is held, how a held set is cut) are search_group_plan.hpp; this unit is
// their host side and two small kernels.  Everything here is host-driven: nothing waits or spins on the device,
// there is no host thread and no callback.  A group launch is
//   1. group_gather_kernel: the members' query blocks -> the group workspace's contiguous buffer, behind the ev_in
//      of every member that found work pending on its caller's stream (recorded there when the call arrived, so
//      the order after it is kept; a call from an idle stream records nothing: group_arrive);
//   2. search_enqueue, unchanged, over the union (queries, nq, staged outputs of the group workspace);
//   3. group_scatter_kernel: each member's ids, distances and counts into that member's own output pointers,
//      its statuses and counters into its lane's pinned mirrors, its share of the launch's exact-path and
//      replayed counts into its lane's head mirror; the launch's work-queue heads are zeroed for the next one.
// A member keeps its lane and token; search_finish waits on the launch's event and reads the member's mirrors.
// A launch of ONE call does not come here at all: it runs on the call's own lane through search_enqueue, as an
// ungrouped call does.
#include <cstdarg>
#include <ctime>
#include <memory>

#include "search_geometry.hpp"
#include "search_group_plan.hpp"
#include "search_internal.hpp"

using namespace isl_lane;

namespace isl {

struct GroupState {
  isl_group::Planner plan;
  std::vector<std::unique_ptr<SearchWorkspace>> slots;  // group workspaces (stable addresses)
  SearchCall calls[kSearchLanes];                       // the call of every lane the group path holds
  uint64_t launches = 0, shared_launches = 0, shared_calls = 0;  // isl_index_group_counters
  uint64_t arrived_calls = 0, marked_calls = 0;                  // isl_index_group_markers
  uint32_t launch_of[kSearchLanes] = {};                         // ISL_GROUP_TRACE: the launch a lane's call went out in
};

}  // namespace isl

namespace {

// one row of the member table (pinned host memory of the group workspace; 64 bytes)
struct GroupMember {
  const float* q;
  uint64_t* ids;
  float* dist;
  uint32_t* count;
  uint32_t* h_status;
  uint32_t* h_ctr;
  uint32_t* h_head;
  uint32_t offset, nq;
};
static_assert(sizeof(GroupMember) == 64, "member table rows are eight words");

constexpr uint32_t kMaxMembers = isl::kSearchLanes;
constexpr uint32_t kScatterBlocks = 64;  // per member; four waves each, one query per wave at a time

// blockIdx.y = member: its nq x d query block -> dst[offset * d ...]
__global__ void group_gather_kernel(const GroupMember* __restrict__ tab, float* __restrict__ dst, uint32_t d) {
  const GroupMember m = tab[blockIdx.y];
  const uint64_t n = (uint64_t)m.nq * d;
  const float* __restrict__ src = m.q;
  float* __restrict__ out = dst + (uint64_t)m.offset * d;
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  if (n % 4 == 0 && (((uintptr_t)src | (uintptr_t)out) & 15) == 0) {
    const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(src);
    uint4* __restrict__ o4 = reinterpret_cast<uint4*>(out);
    for (uint64_t i = t; i < n / 4; i += stride) o4[i] = s4[i];
  } else {
    for (uint64_t i = t; i < n; i += stride) out[i] = src[i];
  }
}

struct ScatterParams {
  const GroupMember* tab;
  // the union's staged answers and per-query words (group workspace)
  const uint64_t* ids;
  const float* dist;
  const uint32_t* count;
  const uint32_t* status;
  const uint32_t* ctr;
  const uint32_t* redo;
  const uint2* plog;
  uint32_t* ticket;   // the launch's work-queue heads: -> h_head, then zero for the workspace's next launch
  uint32_t* h_head;
  uint32_t* scratch;  // [member][4] exact-path count, replayed count, blocks done, -; [kMaxMembers * 4] blocks done in all
  uint32_t k, ef, plog_cap;
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
  return v;
}

// blockIdx.y = member; a wave takes one query of the member at a time.
// isl_search_stats stays exact per call: exact_path = the entries of the launch's redo list in the member's query
// range.  The fast kernel keeps no list of the queries it re-ordered in place (it only counts them, ticket[3]), so
// `replayed` is re-derived per query from what that kernel's test reads: a query that ended QS_OK outside the redo
// list was replayed exactly when two of the first min(len, k + 1) entries of its sorted result set have equal
// distances (search_kernels.hip.h, "equal distances inside the returned prefix (or across its boundary)"), len =
// min(pushes, ef).  Inside the prefix those are the returned distances; across the boundary, entry k + 1 has the
// k-th distance exactly when the push log holds more pushes of that distance than the answer returns (the result
// set is the ef smallest pushes).  A replayed query's pushes all fit its log (otherwise it is on the redo list).
__global__ void group_scatter_kernel(ScatterParams sp) {
  const GroupMember m = sp.tab[blockIdx.y];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
  const uint32_t k = sp.k;
  const uint32_t nredo = *((volatile uint32_t*)&sp.ticket[1]);  // (zeroed by the last block, after every block has read it)
  uint32_t n_exact = 0, n_replayed = 0;
  for (uint32_t qi = wave; qi < m.nq; qi += nwaves) {
    const uint32_t q = m.offset + qi;
    const uint32_t cnt = sp.count[q];
    const uint32_t st = sp.status[q];
    if (lane == 0) {
      m.count[qi] = cnt;
      m.h_status[qi] = st;
    }
    if (lane < 4) m.h_ctr[qi * 4 + lane] = sp.ctr[q * 4 + lane];
    const uint32_t outn = cnt < k ? cnt : k;  // slots past a query's count are not written, as by the search kernels
    for (uint32_t e = lane; e < outn; e += 64) {
      m.ids[(uint64_t)qi * k + e] = sp.ids[(uint64_t)q * k + e];
      m.dist[(uint64_t)qi * k + e] = sp.dist[(uint64_t)q * k + e];
    }
    bool hit = false;
    for (uint32_t i = lane; i < nredo; i += 64) hit |= sp.redo[i] == q;
    if (__ballot(hit)) { n_exact += 1; continue; }
    if (st != QS_OK || outn == 0) continue;
    const uint32_t* db = reinterpret_cast<const uint32_t*>(sp.dist) + (uint64_t)q * k;
    bool dup = false;
    for (uint32_t e = lane; e + 1 < outn; e += 64) dup |= db[e] == db[e + 1];
    bool tie = __ballot(dup) != 0;
    const uint32_t pushes = sp.ctr[q * 4 + 3];
    const uint32_t len = pushes < sp.ef ? pushes : sp.ef;
    if (!tie && outn == k && len >= k + 1) {
      const uint32_t dk = db[k - 1];
      uint32_t returned = 0, pushed = 0;
      for (uint32_t e = lane; e < k; e += 64) returned += db[e] == dk;
      const uint2* pl = sp.plog + (uint64_t)q * sp.plog_cap;
      const uint32_t logged = pushes < sp.plog_cap ? pushes : sp.plog_cap;
      for (uint32_t i = lane; i < logged; i += 64) pushed += pl[i].x == dk;
      tie = wave_sum(pushed) > wave_sum(returned);
    }
    if (tie && pushes <= sp.plog_cap) n_replayed += 1;
  }
  uint32_t* mine = sp.scratch + blockIdx.y * 4;
  if (lane == 0) {
    if (n_exact) atomicAdd(&mine[0], n_exact);
    if (n_replayed) atomicAdd(&mine[1], n_replayed);
  }
  __threadfence();
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (atomicAdd(&mine[2], 1u) == gridDim.x - 1) {  // the member's last block: its head mirror, scratch back to zero
    __threadfence();
    const uint32_t ex = atomicExch(&mine[0], 0u), rp = atomicExch(&mine[1], 0u);
    mine[2] = 0u;
    for (uint32_t i = 0; i < 16; ++i) m.h_head[i] = i == 1 ? ex : i == 3 ? rp : 0u;
  }
  uint32_t* all = sp.scratch + kMaxMembers * 4;
  if (atomicAdd(all, 1u) == gridDim.x * gridDim.y - 1) {  // the launch's last block
    *all = 0u;
    for (uint32_t i = 0; i < 16; ++i) {
      sp.h_head[i] = sp.ticket[i];
      sp.ticket[i] = 0u;
    }
  }
}

__global__ void zero_u32_kernel(uint32_t* p, uint32_t n) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 0u;
}

// ISL_GROUP_TRACE: one stderr line with the host's clocks in front -- the boot-time clock is the one a kernel trace's
// timestamps are on, the monotonic one is the interpreter's perf_counter
void trace_line(const char* fmt, ...) {
  timespec b{}, m{};
  clock_gettime(CLOCK_BOOTTIME, &b);
  clock_gettime(CLOCK_MONOTONIC, &m);
  char text[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(text, sizeof text, fmt, ap);
  va_end(ap);
  fprintf(stderr, "isl group-trace boot_ns=%lld mono_ns=%lld %s\n", (long long)b.tv_sec * 1000000000ll + b.tv_nsec,
          (long long)m.tv_sec * 1000000000ll + m.tv_nsec, text);
}

uint32_t group_cap(const isl_index* idx) { return idx->group_sw.cap ? idx->group_sw.cap : isl_group::kDefaultCap; }

isl::GroupState& state_of(const isl_index* idx) {  // under idx->group_mu
  if (!idx->group) {
    idx->group = new isl::GroupState();
    idx->group->plan.configure(group_cap(idx), 0);
  }
  return *idx->group;
}

// a group workspace able to take `nq` queries of the call shape (d, k): its buffers beyond prepare_workspace's
isl_status prepare_slot(const isl_index* idx, isl::SearchWorkspace& gw, uint64_t nq, uint64_t d, uint64_t k) {
  uint64_t* const ev = &gw.alloc_events;
  gw.union_launch = true;
  ISL_TRY(ensure_lane_stream(idx, gw));
  ISL_TRY(gw.q_stage.reserve(nq * d, ev));
  const uint64_t outs = nq * std::max<uint64_t>(k, 1);
  ISL_TRY(gw.ids_stage.reserve(outs, ev));
  ISL_TRY(gw.dist_stage.reserve(outs, ev));
  ISL_TRY(gw.count_stage.reserve(nq, ev));
  ISL_TRY(gw.h_members.reserve((uint64_t)kMaxMembers * 8, ev));
  if (!gw.grp_scratch) {
    ISL_TRY(gw.grp_scratch.reserve(kMaxMembers * 4 + 4, ev));
    hipLaunchKernelGGL(zero_u32_kernel, dim3(1), dim3(256), 0, gw.stream, gw.grp_scratch.get(), kMaxMembers * 4 + 4);
    ISL_HIP(hipGetLastError());
  }
  return ISL_OK;
}

// the group workspace `w` of the state, created on first use (under idx->group_mu)
isl::SearchWorkspace& slot(isl::GroupState& g, int32_t w) {
  if (!g.slots[w]) {
    g.slots[w].reset(new isl::SearchWorkspace());
    // pool streams from the far end: the lanes claim theirs from the front, and the calls that go out alone
    // while a group is in flight are the lowest lanes
    g.slots[w]->pool_lane = isl::kSearchLanes - 1 - w;
  }
  return *g.slots[w];
}

void grow_slots(const isl_index* idx, isl::GroupState& g, uint32_t n) {
  if (g.slots.size() < n) g.slots.resize(n);
  g.plan.configure(group_cap(idx), n);
}

isl_status enqueue_alone(const isl_index* idx, isl::GroupState& g, const isl_group::Launch& L) {
  const uint32_t lane_no = L.members[0].call;
  isl::SearchWorkspace& ws = idx->ws[lane_no];
  SearchCall c = g.calls[lane_no];
  c.user_stream = nullptr;
  // behind ev_in where the call put it on the caller's stream when it arrived
  c.mode = ws.grp_marked ? StreamMode::OWN_AFTER_EVENT : StreamMode::OWN;
  ISL_TRY(search_enqueue(idx, ws, c));
  ws.grp_launch = nullptr;
  ws.grp_offset = 0;
  ws.grp_ready = ws.ev1;  // behind the last search kernel: the answers are in the caller's buffers
  return ISL_OK;
}

isl_status enqueue_group_impl(const isl_index* idx, isl::GroupState& g, const isl_group::Launch& L,
                              isl::SearchWorkspace& gw) {
  const uint64_t d = L.key.d, k = L.key.k;
  const uint32_t nm = (uint32_t)L.members.size();
  if (nm > kMaxMembers) return isl::fail(ISL_ERR_SEARCH, "Search error: %u calls in one group launch", nm);
  CallGeometry cg;
  ISL_TRY(call_geometry(idx, d, k, L.key.ef, nullptr, cg));
  // everything the launch may have to set up comes first: setting up synchronises the stream, which must not
  // yet wait for the callers' streams then
  ISL_TRY(prepare_slot(idx, gw, L.nq, d, k));
  ISL_TRY(prepare_workspace(idx, gw, L.nq, (uint32_t)std::min<uint64_t>(L.nq, cg.lane_slots), cg.plog_cap));
  GroupMember* tab = reinterpret_cast<GroupMember*>(gw.h_members.get());
  for (uint32_t i = 0; i < nm; ++i) {
    const isl_group::Member& mb = L.members[i];
    isl::SearchWorkspace& ws = idx->ws[mb.call];
    const SearchCall& c = g.calls[mb.call];
    // the member's own mirrors must hold its queries' words (isl_index_prepare sized them; a lane's first call may not have)
    ISL_TRY(ws.h_status.reserve(std::max<uint64_t>(mb.nq, 1024), &ws.alloc_events));
    ISL_TRY(ws.h_ctr.reserve(std::max<uint64_t>(mb.nq, 1024) * 4, &ws.alloc_events));
    tab[i] = GroupMember{c.queries, c.ids, c.dist, c.count, ws.h_status, ws.h_ctr, ws.h_head, mb.offset, mb.nq};
    if (ws.grp_marked) ISL_HIP(hipStreamWaitEvent(gw.stream, ws.ev_in, 0));
  }
  hipLaunchKernelGGL(group_gather_kernel, dim3(64, nm), dim3(256), 0, gw.stream, tab, gw.q_stage.get(), (uint32_t)d);
  ISL_HIP(hipGetLastError());
  SearchCall u;
  u.queries = gw.q_stage;
  u.nq = L.nq;
  u.d = d;
  u.k = k;
  u.ef = L.key.ef;
  u.ids = gw.ids_stage;
  u.dist = gw.dist_stage;
  u.count = gw.count_stage;
  u.mode = StreamMode::OWN;
  ISL_TRY(search_enqueue(idx, gw, u));
  ScatterParams sp{};
  sp.tab = tab;
  sp.ids = gw.ids_stage;
  sp.dist = gw.dist_stage;
  sp.count = gw.count_stage;
  sp.status = gw.status;
  sp.ctr = gw.ctr;
  sp.redo = gw.redo;
  sp.plog = reinterpret_cast<const uint2*>(gw.plog.get());
  sp.ticket = gw.ticket;
  sp.h_head = gw.h_head;
  sp.scratch = gw.grp_scratch;
  sp.k = (uint32_t)k;
  sp.ef = cg.ef;
  sp.plog_cap = cg.plog_cap;
  hipLaunchKernelGGL(group_scatter_kernel, dim3(kScatterBlocks, nm), dim3(256), 0, gw.stream, sp);
  ISL_HIP(hipGetLastError());
  gw.ticket_clean = true;  // (in stream order: the scatter kernel's last block zeroes the heads)
  ISL_HIP(hipEventRecord(gw.ev_done, gw.stream));
  return ISL_OK;
}

// As search_enqueue does for its own kernels: a failure part-way leaves nothing of the launch on the stream.
isl_status enqueue_group(const isl_index* idx, isl::GroupState& g, const isl_group::Launch& L) {
  isl::SearchWorkspace& gw = slot(g, L.workspace);
  const uint64_t mark = gw.alloc_events;
  const isl_status st = enqueue_group_impl(idx, g, L, gw);
  gw.enqueued = false;  // (the members are waited for, not the workspace)
  if (st != ISL_OK) {
    const isl::ErrorRecord keep = isl::last_error();
    if (gw.stream) (void)hipStreamSynchronize(gw.stream);
    (void)hipGetLastError();
    gw.ticket_clean = false;
    isl::last_error() = keep;
    return st;
  }
  for (const isl_group::Member& mb : L.members) {
    isl::SearchWorkspace& ws = idx->ws[mb.call];
    ws.grp_launch = &gw;
    ws.grp_offset = mb.offset;
    ws.grp_ready = gw.ev_done;  // behind the scatter kernel
    ws.grp_allocs = gw.alloc_events - mark;
    ws.enqueued = true;
    ws.nq_inflight = mb.nq;
    ws.k_inflight = L.key.k;
    ws.ef_inflight = gw.ef_inflight;
    ws.fast_inflight = gw.fast_inflight;
    ws.st_inflight = gw.stream;
  }
  return ISL_OK;
}

// launches whose event has completed leave the in-flight count (under idx->group_mu)
void poll(const isl_index* idx, isl::GroupState& g) {
  for (const isl_group::Planner::Live& l : g.plan.live()) {
    hipEvent_t ev = l.workspace >= 0 ? g.slots[l.workspace]->ev_done : idx->ws[l.first_call].ev_done;
    const hipError_t e = hipEventQuery(ev);
    if (e != hipSuccess) (void)hipGetLastError();  // hipErrorNotReady
    if (idx->group_sw.trace) {
      uint32_t marks = 0, marks_pending = 0;  // the members' markers on their callers' streams, and those not yet reached
      for (int i = 0; i < isl::kSearchLanes; ++i) {
        const isl::SearchWorkspace& ws = idx->ws[i];
        if (g.launch_of[i] != l.id || !ws.grp || !ws.grp_marked) continue;
        marks += 1;
        if (hipEventQuery(ws.ev_in) != hipSuccess) { (void)hipGetLastError(); marks_pending += 1; }
      }
      trace_line("poll launch=%u done=%d markers=%u markers_pending=%u", l.id, e == hipSuccess ? 1 : 0, marks, marks_pending);
    }
    if (e == hipSuccess) g.plan.complete(l.id);
  }
}

// Submits what the rules release (wanted = a held call that must go now, or kNone).  A launch that cannot be
// enqueued fails every member's wait with that error; nothing of it stays in flight.  (under idx->group_mu)
void submit(const isl_index* idx, isl::GroupState& g, uint32_t wanted) {
  isl_group::Launch L;
  for (;;) {
    if (wanted != isl_group::kNone && !g.plan.held(wanted)) wanted = isl_group::kNone;
    if (!g.plan.next(wanted, L)) break;
    const isl_status st = L.workspace < 0 ? enqueue_alone(idx, g, L) : enqueue_group(idx, g, L);
    if (idx->group_sw.trace) {
      char calls[256];
      int at = 0;
      uint32_t marks = 0;
      for (const isl_group::Member& mb : L.members) {
        g.launch_of[mb.call] = L.id;
        marks += idx->ws[mb.call].grp_marked ? 1u : 0u;
        if (at < (int)sizeof calls - 12) at += snprintf(calls + at, sizeof calls - at, "%s%u", at ? "," : "", mb.call);
      }
      hipStream_t on = L.workspace < 0 ? idx->ws[L.members[0].call].stream : g.slots[L.workspace]->stream;
      trace_line("launch id=%u status=%d workspace=%d queries=%u lanes=%s markers=%u stream=%p wanted=%d inflight=%llu",
                 L.id, (int)st, L.workspace, L.nq, calls, marks, (void*)on, wanted == isl_group::kNone ? -1 : (int)wanted,
                 (unsigned long long)g.plan.inflight());
    }
    if (st == ISL_OK) {
      g.launches += 1;
      if (L.workspace >= 0) { g.shared_launches += 1; g.shared_calls += L.members.size(); }
      continue;
    }
    for (const isl_group::Member& mb : L.members) {
      isl::SearchWorkspace& ws = idx->ws[mb.call];
      ws.grp_failed = true;
      ws.grp_status = st;
      ws.grp_error = isl::last_error();
      ws.grp_launch = nullptr;
      ws.enqueued = false;
    }
    g.plan.abandon(L.id);
  }
}

}  // namespace

bool isl_lane::group_takes(const isl_index* idx, const SearchCall& c) {
  static const bool instrumented = getenv("ISL_TIMELINE") != nullptr || getenv("ISL_DEBUG") != nullptr;
  isl_group::CallTraits t;
  t.device_async = true;  // (asked by isl_search_batch_device_async alone)
  t.recompute = idx->recompute;
  t.two_level = c.two_level;
  t.hnsw = idx->is_hnsw;
  t.construction = idx->build_q_entry != nullptr;
  t.instrumented = instrumented;
  t.nq = c.nq;
  return isl_group::groupable(t, idx->group_sw.off, group_cap(idx));
}

isl_status isl_lane::group_arrive(const isl_index* idx, isl::SearchWorkspace& ws, const SearchCall& c) {
  CallGeometry cg;
  ISL_TRY(call_geometry(idx, c.d, c.k, c.ef, nullptr, cg));
  ISL_TRY(ensure_lane_stream(idx, ws));
  // The call is ordered after the caller's stream as of now.  A stream with nothing pending orders nothing, and
  // then no marker goes on it: the caller's stream shares its hardware queue with launch streams, and a marker in
  // that queue is reached only when the traversal kernel in front of it has ended -- every launch that waits for
  // it starts milliseconds late, on whichever queue it sits itself.
  bool marked = idx->group_sw.mark_always;
  if (!marked && hipStreamQuery(c.user_stream) != hipSuccess) {
    (void)hipGetLastError();  // pending work (or a stream that cannot be asked): the marker, as for any other order
    marked = true;
  }
  if (marked) ISL_HIP(hipEventRecord(ws.ev_in, c.user_stream));
  const uint32_t lane_no = (uint32_t)(&ws - idx->ws);
  std::lock_guard<std::mutex> lock(idx->group_mu);
  isl::GroupState& g = state_of(idx);
  if (g.slots.empty()) grow_slots(idx, g, isl::kSearchLanes / 2);  // not prepared: workspaces come as launches need them
  g.calls[lane_no] = c;
  g.arrived_calls += 1;
  g.marked_calls += marked ? 1 : 0;
  if (idx->group_sw.trace) trace_line("arrive lane=%u queries=%llu marker=%d", lane_no, (unsigned long long)c.nq, marked ? 1 : 0);
  ws.grp = true;
  ws.grp_marked = marked;
  ws.grp_failed = false;
  ws.grp_launch = nullptr;
  ws.grp_allocs = 0;
  poll(idx, g);
  const uint32_t room = idx->group_sw.room ? idx->group_sw.room : cg.slots;
  g.plan.arrive(lane_no, (uint32_t)c.nq, isl_group::Key{c.d, c.k, cg.ef}, room);
  submit(idx, g, isl_group::kNone);
  if (ws.grp_failed) {  // this call's own launch: the error is the call's
    ws.grp = false;
    isl::last_error() = ws.grp_error;
    return ws.grp_status;
  }
  return ISL_OK;
}

void isl_lane::group_pump(const isl_index* idx) {
  std::lock_guard<std::mutex> lock(idx->group_mu);
  if (!idx->group || !idx->group->plan.any_held()) return;
  poll(idx, *idx->group);
  submit(idx, *idx->group, isl_group::kNone);
}

isl_status isl_lane::group_before_wait(const isl_index* idx, isl::SearchWorkspace& ws) {
  std::lock_guard<std::mutex> lock(idx->group_mu);
  isl::GroupState& g = state_of(idx);
  poll(idx, g);
  submit(idx, g, (uint32_t)(&ws - idx->ws));
  if (ws.grp_failed) {
    isl::last_error() = ws.grp_error;
    return ws.grp_status;
  }
  return ISL_OK;
}

void isl_lane::group_after_wait(const isl_index* idx, isl::SearchWorkspace& ws) {
  std::lock_guard<std::mutex> lock(idx->group_mu);
  if (!idx->group) return;
  isl::GroupState& g = *idx->group;
  const isl::ErrorRecord keep = isl::last_error();
  g.plan.finished((uint32_t)(&ws - idx->ws));
  ws.grp = false;
  ws.grp_launch = nullptr;
  if (g.plan.any_held()) {
    poll(idx, g);
    submit(idx, g, isl_group::kNone);
  }
  isl::last_error() = keep;
}

isl_status isl_lane::group_prepare(const isl_index* idx, uint64_t max_nq, uint64_t max_ef, uint64_t max_k, int32_t lanes,
                                   uint32_t ovf_waves, uint32_t plog_cap) {
  if (idx->group_sw.off || idx->recompute || idx->is_hnsw || idx->build_q_entry) return ISL_OK;
  std::lock_guard<std::mutex> lock(idx->group_mu);
  isl::GroupState& g = state_of(idx);
  const uint32_t cap = group_cap(idx);
  const uint32_t n = isl_group::workspaces_for((uint32_t)lanes, max_nq, cap);
  const uint64_t nq = isl_group::workspace_queries((uint32_t)lanes, max_nq, cap);
  grow_slots(idx, g, std::max<uint32_t>(n, (uint32_t)g.slots.size()));
  const uint64_t d = idx->rows.d();
  for (uint32_t w = 0; w < n; ++w) {
    isl::SearchWorkspace& gw = slot(g, (int32_t)w);
    ISL_TRY(prepare_slot(idx, gw, nq, d, std::max<uint64_t>(max_k, 1)));
    // (the overflow tables as the lanes size theirs: for the most waves any ef puts on the chip)
    ISL_TRY(prepare_workspace(idx, gw, (uint32_t)nq, (uint32_t)std::min<uint64_t>(nq, ovf_waves), plog_cap));
    if (idx->seeds.count()) ISL_TRY(gw.q_entry.reserve(nq * 4, &gw.alloc_events));
  }
  // the launches of a group over zero queries and no members, twice over, as isl_index_prepare warms the lanes
  for (int round = 0; round < 2; ++round) {
    for (uint32_t w = 0; w < n; ++w) {
      isl::SearchWorkspace& gw = *g.slots[w];
      GroupMember* tab = reinterpret_cast<GroupMember*>(gw.h_members.get());
      tab[0] = GroupMember{};
      hipLaunchKernelGGL(group_gather_kernel, dim3(1, 1), dim3(256), 0, gw.stream, tab, gw.q_stage.get(), (uint32_t)d);
      ISL_HIP(hipGetLastError());
      SearchCall warm_call;
      warm_call.d = d;
      warm_call.k = std::min<uint64_t>(max_k, max_ef);
      warm_call.ef = max_ef;
      ISL_TRY(search_enqueue(idx, gw, warm_call, RoundPlan{}, true));
      ScatterParams sp{};
      sp.tab = tab;
      sp.ids = gw.ids_stage;
      sp.dist = gw.dist_stage;
      sp.count = gw.count_stage;
      sp.status = gw.status;
      sp.ctr = gw.ctr;
      sp.redo = gw.redo;
      sp.plog = reinterpret_cast<const uint2*>(gw.plog.get());
      sp.ticket = gw.ticket;
      sp.h_head = gw.h_head;
      sp.scratch = gw.grp_scratch;
      sp.k = (uint32_t)std::max<uint64_t>(max_k, 1);
      sp.ef = (uint32_t)max_ef;
      sp.plog_cap = plog_cap;
      // (a member of no queries: its head mirror is the workspace's own, overwritten by the launch's heads)
      tab[0].h_head = gw.h_head;
      hipLaunchKernelGGL(group_scatter_kernel, dim3(kScatterBlocks, 1), dim3(256), 0, gw.stream, sp);
      ISL_HIP(hipGetLastError());
      gw.ticket_clean = true;
      ISL_HIP(hipEventRecord(gw.ev_done, gw.stream));
    }
    for (uint32_t w = 0; w < n; ++w) ISL_HIP(hipStreamSynchronize(g.slots[w]->stream));
  }
  return ISL_OK;
}

extern "C" isl_status isl_index_group_counters(const isl_index* idx, uint64_t* launches, uint64_t* shared_launches,
                                               uint64_t* shared_calls) {
  if (!idx) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "index is NULL");
  std::lock_guard<std::mutex> lock(idx->group_mu);
  const isl::GroupState* g = idx->group;
  if (launches) *launches = g ? g->launches : 0;
  if (shared_launches) *shared_launches = g ? g->shared_launches : 0;
  if (shared_calls) *shared_calls = g ? g->shared_calls : 0;
  return ISL_OK;
}

extern "C" isl_status isl_index_group_markers(const isl_index* idx, uint64_t* calls, uint64_t* marked_calls) {
  if (!idx) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "index is NULL");
  std::lock_guard<std::mutex> lock(idx->group_mu);
  const isl::GroupState* g = idx->group;
  if (calls) *calls = g ? g->arrived_calls : 0;
  if (marked_calls) *marked_calls = g ? g->marked_calls : 0;
  return ISL_OK;
}

void isl::free_group_state(isl_index* idx) {
  std::lock_guard<std::mutex> lock(idx->group_mu);
  GroupState* g = idx->group;
  if (!g) return;
  // held calls go out (their callers' buffers and lanes are theirs to wait for; the lanes are drained next)
  for (int i = 0; i < kSearchLanes; ++i)
    if (g->plan.held((uint32_t)i)) submit(idx, *g, (uint32_t)i);
  for (auto& s : g->slots)
    if (s) {
      if (s->stream) (void)hipStreamSynchronize(s->stream);
      (void)hipGetLastError();
      free_workspace(*s);
    }
  delete g;
  idx->group = nullptr;
}
