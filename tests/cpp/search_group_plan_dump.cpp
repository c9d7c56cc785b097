// The planner of the grouped search launches (islands_amd/csrc/search_group_plan.hpp) without a device or the
// library:
//   g++ -std=c++17 tests/cpp/search_group_plan_dump.cpp -o search_group_plan_dump
// stdin, one command per line:
//   config CAP WORKSPACES
//   arrive CALL NQ D K EF ROOM     the call joins the held set, then a pump (as group_arrive does)
//   pump                           a later entry into the library
//   wait CALL                      the call is about to be waited for: it goes now if held, then a pump
//   complete LAUNCH                the launch's event was seen complete
//   done CALL                      the call's wait is over, then a pump (as group_after_wait does)
//   traits ASYNC RECOMPUTE TWO_LEVEL HNSW CONSTRUCTION INSTRUMENTED NQ OFF CAP   -> "groupable 0|1"
//   workspaces LANES MAX_NQ CAP    -> "workspaces N queries Q"
// stdout: "launch ID ws W nq N key D K EF : CALL/NQ@OFFSET ..." for every launch a command submits, and after
// every command of the first six kinds "state inflight N held H".
// (tests/test_search_group_plan_cpu.py)
#include <cstdio>
#include <cstring>

#include "../../islands_amd/csrc/search_group_plan.hpp"

using namespace isl_group;

// the loop of search_group.hip's submit()
static void submit(Planner& p, uint32_t wanted) {
  Launch L;
  for (;;) {
    if (wanted != kNone && !p.held(wanted)) wanted = kNone;
    if (!p.next(wanted, L)) break;
    std::printf("launch %u ws %d nq %u key %llu %llu %llu :", L.id, L.workspace, L.nq, (unsigned long long)L.key.d,
                (unsigned long long)L.key.k, (unsigned long long)L.key.ef);
    for (const Member& m : L.members) std::printf(" %u/%u@%u", m.call, m.nq, m.offset);
    std::printf("\n");
  }
}

int main() {
  Planner p;
  char cmd[32];
  std::vector<uint32_t> held_calls;
  while (std::scanf("%31s", cmd) == 1) {
    if (!std::strcmp(cmd, "traits")) {
      unsigned a[6], off = 0, cap = 0;
      unsigned long long nq = 0;
      if (std::scanf("%u %u %u %u %u %u %llu %u %u", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &nq, &off, &cap) != 9) return 2;
      CallTraits t;
      t.device_async = a[0]; t.recompute = a[1]; t.two_level = a[2]; t.hnsw = a[3]; t.construction = a[4];
      t.instrumented = a[5]; t.nq = nq;
      std::printf("groupable %d\n", groupable(t, off != 0, cap) ? 1 : 0);
      continue;
    }
    if (!std::strcmp(cmd, "workspaces")) {
      unsigned lanes = 0, cap = 0;
      unsigned long long max_nq = 0;
      if (std::scanf("%u %llu %u", &lanes, &max_nq, &cap) != 3) return 2;
      std::printf("workspaces %u queries %llu\n", workspaces_for(lanes, max_nq, cap),
                  (unsigned long long)workspace_queries(lanes, max_nq, cap));
      continue;
    }
    if (!std::strcmp(cmd, "config")) {
      unsigned cap = 0, ws = 0;
      if (std::scanf("%u %u", &cap, &ws) != 2) return 2;
      p.configure(cap, ws);
    } else if (!std::strcmp(cmd, "arrive")) {
      unsigned call = 0, nq = 0, room = 0;
      unsigned long long d = 0, k = 0, ef = 0;
      if (std::scanf("%u %u %llu %llu %llu %u", &call, &nq, &d, &k, &ef, &room) != 6) return 2;
      p.arrive(call, nq, Key{d, k, ef}, room);
      held_calls.push_back(call);
      submit(p, kNone);
    } else if (!std::strcmp(cmd, "pump")) {
      submit(p, kNone);
    } else if (!std::strcmp(cmd, "wait")) {
      unsigned call = 0;
      if (std::scanf("%u", &call) != 1) return 2;
      submit(p, call);
    } else if (!std::strcmp(cmd, "complete")) {
      unsigned id = 0;
      if (std::scanf("%u", &id) != 1) return 2;
      p.complete(id);
    } else if (!std::strcmp(cmd, "done")) {
      unsigned call = 0;
      if (std::scanf("%u", &call) != 1) return 2;
      p.finished(call);
      submit(p, kNone);
    } else {
      return 2;
    }
    unsigned held = 0;
    for (uint32_t c : held_calls) held += p.held(c) ? 1 : 0;
    for (size_t i = 0; i < held_calls.size();)
      if (!p.held(held_calls[i])) held_calls.erase(held_calls.begin() + i); else ++i;
    std::printf("state inflight %llu held %u\n", (unsigned long long)p.inflight(), held);
  }
  return 0;
}
