// Host-only arithmetic of the grouped search launches (search_group.hip): which asynchronous calls may share a
// launch, when an arriving call is submitted and when it is held, how a held set is cut, where each member's
// queries lie in the union.  Plain C++ without a device header, in the manner of recompute_plan.hpp and
// remove_plan.hpp: tests/cpp/search_group_plan_dump.cpp drives it with g++ alone
// (tests/test_search_group_plan_cpu.py).
//
// Why: a process gets a handful of hardware queues (four, unless its environment says otherwise before HIP
// starts).  The lanes' streams share them, and in one queue the next call's traversal kernel starts only when the
// previous call's slowest query has finished.  A call that finds every resident wave taken therefore gains
// nothing by being enqueued at once; held back, it can share ONE launch with the calls that arrive behind it, and
// that launch's tail is paid once for all of them.
//
// The rules:
//   * a call is submitted at once when fewer than `room` queries of the index are in flight (room = the resident
//     waves of the call's launch geometry), together with every compatible call that is held, as one launch;
//   * otherwise it is held; a held set goes out when its queries reach `cap`, when a later entry into the
//     library finds room (pump), or when one of its members is waited for;
//   * a set of more than `cap` queries is cut in arrival order;
//   * a launch of one call runs on the call's own lane exactly as an ungrouped call does; a launch of several
//     needs a group workspace, and stays held while none is free (a member that is waited for then goes alone).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace isl_group {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kDefaultCap = 4096;  // queries of one launch (ISL_GROUP_CAP; measured: profiles/search_group_cap.json)

// Calls of one index share a launch only with the same d, k and (effective) ef.
struct Key {
  uint64_t d = 0, k = 0, ef = 0;
  bool operator==(const Key& o) const { return d == o.d && k == o.k && ef == o.ef; }
};

// What else decides whether a call may wait for company at all; every other call keeps the ungrouped path.
struct CallTraits {
  bool device_async = false;   // came in through isl_search_batch_device_async
  bool recompute = false;      // recompute provider
  bool two_level = false;
  bool hnsw = false;           // HnswGraph facade
  bool construction = false;   // the builder's construction searches (build_q_entry)
  bool instrumented = false;   // ISL_TIMELINE or ISL_DEBUG set
  uint64_t nq = 0;
};
inline bool groupable(const CallTraits& t, bool grouping_off, uint32_t cap) {
  return !grouping_off && t.device_async && !t.recompute && !t.two_level && !t.hnsw && !t.construction &&
         !t.instrumented && t.nq >= 1 && t.nq <= cap;
}

// Group workspaces isl_index_prepare sets up for `lanes` calls of up to max_nq queries: enough that all of them
// can be in flight in launches of `cap` (+1: a cut leaves launches short of cap), and never more than lanes / 2,
// since a launch that needs one has at least two members.
inline uint32_t workspaces_for(uint32_t lanes, uint64_t max_nq, uint32_t cap) {
  if (lanes < 2 || cap == 0) return 0;
  const uint64_t by_queries = ((uint64_t)lanes * max_nq + cap - 1) / cap + 1;
  return (uint32_t)std::min<uint64_t>(by_queries, lanes / 2);
}
// ... and the queries each of them is sized for
inline uint64_t workspace_queries(uint32_t lanes, uint64_t max_nq, uint32_t cap) {
  return std::min<uint64_t>(cap, (uint64_t)lanes * max_nq);
}

struct Member {
  uint32_t call = 0;    // the caller's name for it (the lane's index)
  uint32_t nq = 0;
  uint32_t offset = 0;  // first query of the member in the union
};
struct Launch {
  uint32_t id = 0;
  int32_t workspace = -1;  // group workspace, or -1: one call on its own lane
  Key key{};
  uint32_t nq = 0;
  std::vector<Member> members;
};

class Planner {
 public:
  void configure(uint32_t cap, uint32_t workspaces) {
    cap_ = std::max<uint32_t>(cap, 1);
    if (workspaces > ws_busy_.size()) ws_busy_.resize(workspaces, false);
  }
  uint32_t cap() const { return cap_; }
  uint32_t workspaces() const { return (uint32_t)ws_busy_.size(); }
  uint64_t inflight() const { return inflight_; }
  bool held(uint32_t call) const {
    for (const Held& h : held_) if (h.call == call) return true;
    return false;
  }
  bool any_held() const { return !held_.empty(); }

  // a groupable call (nq <= cap) arrives; `room` = resident waves of its launch geometry (or ISL_GROUP_ROOM)
  void arrive(uint32_t call, uint32_t nq, const Key& key, uint32_t room) { held_.push_back(Held{call, nq, key, room}); }

  // The next launch to submit, or false.  wanted = a held call that is being waited for (its set goes whatever
  // is in flight), kNone at a pump.  The launch is in flight from here on.
  bool next(uint32_t wanted, Launch& out) {
    if (wanted != kNone) {
      for (const Held& h : held_)
        if (h.call == wanted) return take(h.key, true, wanted, out);
      return false;
    }
    std::vector<Key> seen;
    for (size_t i = 0; i < held_.size(); ++i) {
      const Key key = held_[i].key;
      if (std::find(seen.begin(), seen.end(), key) != seen.end()) continue;
      seen.push_back(key);
      uint64_t total = 0;
      for (const Held& h : held_) if (h.key == key) total += h.nq;
      if ((total >= cap_ || inflight_ < held_[i].room) && take(key, false, kNone, out)) return true;
    }
    return false;
  }

  // launches not yet seen complete: what the host asks hipEventQuery about
  struct Live { uint32_t id; int32_t workspace; uint32_t first_call; };
  std::vector<Live> live() const {
    std::vector<Live> v;
    for (const Flight& f : flights_) if (!f.complete) v.push_back(Live{f.id, f.workspace, f.calls.front()});
    return v;
  }
  // the launch's event has been seen complete
  void complete(uint32_t launch) {
    for (size_t i = 0; i < flights_.size(); ++i)
      if (flights_[i].id == launch) { settle(i); return; }
  }
  // a member's wait is over (its launch is complete then); the workspace is free once every member's is.
  // Returns the workspace that became free, or -1.
  int32_t finished(uint32_t call) {
    for (size_t i = 0; i < flights_.size(); ++i) {
      Flight& f = flights_[i];
      auto it = std::find(f.calls.begin(), f.calls.end(), call);
      if (it == f.calls.end()) continue;
      f.calls.erase(it);
      if (!f.complete) { f.complete = true; inflight_ -= f.nq; }
      if (!f.calls.empty()) return -1;
      const int32_t w = f.workspace;
      if (w >= 0) ws_busy_[w] = false;
      flights_.erase(flights_.begin() + i);
      return w;
    }
    return -1;
  }
  // the launch could not be enqueued: nothing of it is in flight, its members are gone
  void abandon(uint32_t launch) {
    for (size_t i = 0; i < flights_.size(); ++i)
      if (flights_[i].id == launch) {
        Flight& f = flights_[i];
        if (!f.complete) inflight_ -= f.nq;
        if (f.workspace >= 0) ws_busy_[f.workspace] = false;
        flights_.erase(flights_.begin() + i);
        return;
      }
  }
  // a held call leaves without a launch (its caller gave up on it)
  void drop(uint32_t call) {
    for (size_t i = 0; i < held_.size(); ++i)
      if (held_[i].call == call) { held_.erase(held_.begin() + i); return; }
  }

 private:
  struct Held { uint32_t call, nq; Key key; uint32_t room; };
  struct Flight { uint32_t id; int32_t workspace; uint32_t nq; bool complete; std::vector<uint32_t> calls; };

  void settle(size_t i) {
    Flight& f = flights_[i];
    if (f.complete) return;
    f.complete = true;
    inflight_ -= f.nq;
  }
  int32_t free_workspace() const {
    for (size_t w = 0; w < ws_busy_.size(); ++w) if (!ws_busy_[w]) return (int32_t)w;
    return -1;
  }
  // the held calls of `key` in arrival order, cut at cap
  bool take(const Key& key, bool forced, uint32_t wanted, Launch& out) {
    std::vector<size_t> pick;
    uint64_t total = 0;
    for (size_t i = 0; i < held_.size(); ++i) {
      if (!(held_[i].key == key)) continue;
      if (!pick.empty() && total + held_[i].nq > cap_) break;
      pick.push_back(i);
      total += held_[i].nq;
    }
    if (pick.empty()) return false;
    int32_t w = -1;
    if (pick.size() > 1) {
      w = free_workspace();
      if (w < 0) {
        if (!forced) return false;  // stays held
        // no workspace and somebody waits: that call alone, on its own lane
        pick.clear();
        for (size_t i = 0; i < held_.size(); ++i) if (held_[i].call == wanted) pick.push_back(i);
      }
    }
    out = Launch{};
    out.id = next_id_++;
    out.workspace = pick.size() > 1 ? w : -1;
    out.key = key;
    Flight f{out.id, out.workspace, 0, false, {}};
    for (size_t i : pick) {
      out.members.push_back(Member{held_[i].call, held_[i].nq, out.nq});
      out.nq += held_[i].nq;
      f.calls.push_back(held_[i].call);
    }
    f.nq = out.nq;
    for (size_t n = pick.size(); n-- > 0;) held_.erase(held_.begin() + pick[n]);
    if (out.workspace >= 0) ws_busy_[out.workspace] = true;
    inflight_ += out.nq;
    flights_.push_back(f);
    return true;
  }

  uint32_t cap_ = kDefaultCap;
  uint32_t next_id_ = 1;
  uint64_t inflight_ = 0;
  std::vector<Held> held_;
  std::vector<Flight> flights_;
  std::vector<bool> ws_busy_;
};

}  // namespace isl_group
