// The round scheduler and the caps of islands_amd/csrc/recompute_plan.hpp without a device or the library:
//   g++ -std=c++17 tests/cpp/recompute_plan_dump.cpp -o recompute_plan_dump
// stdin, first word "rounds": nq, the in-flight cap, the kind (0 re-run, 1 park, 2 the heap-exact kernel's
// queue), two_level (0 / 1), ef; then one line per round with one status for each query started so far (a
// query the round did not list keeps the status of its last run); after a "short" verdict one line "n id ...":
// the queries whose window was too small.  stdout: "round r listed L q <ids> x <ids> -> verdict" per round
// ("launch", "final", or "short", which a second line of the same round follows once the short queries are
// handed over), then "rounds R of M" with M the round cap.
// first word "caps": slab_rows, nvec, nq, two_level, max_degree, use_fast, ef -> the cap functions, one per line.
// (tests/test_recompute_plan_cpu.py)
#include <cstdio>
#include <cstring>

#include "../../islands_amd/csrc/recompute_plan.hpp"

using namespace isl_rounds;

static const char* name(Verdict v) { return v == Verdict::LAUNCH ? "launch" : v == Verdict::FINAL ? "final" : "short"; }

static int caps() {
  unsigned long long slab = 0, nvec = 0, nq = 0, max_degree = 0, ef = 0;
  unsigned tl = 0, use_fast = 0;
  if (std::scanf("%llu %llu %llu %u %llu %u %llu", &slab, &nvec, &nq, &tl, &max_degree, &use_fast, &ef) != 7) return 2;
  const uint32_t in_flight = max_in_flight(nq, slab, nvec, tl != 0, max_degree);
  const Kind kind = batch_kind(tl != 0, use_fast != 0, !tl && slab < nvec);
  std::printf("hop_rows %llu\nin_flight %u\nkind %d\n", (unsigned long long)hop_rows(tl != 0, max_degree), in_flight, (int)kind);
  std::printf("max_rounds %llu\n", (unsigned long long)max_rounds(nq, in_flight, ef));
  std::printf("miss_capacity %llu\nprefetch_capacity %llu\n", (unsigned long long)miss_capacity(nq),
              (unsigned long long)prefetch_capacity(nq));
  std::printf("stall_limit %u\nwindow", stall_limit(kind));
  uint32_t scale = 1;
  do std::printf(" %u", scale); while (grow_window(scale));
  std::printf("\n");
  return 0;
}

static int rounds() {
  unsigned nq = 0, cap = 0, kind = 0, tl = 0;
  unsigned long long ef = 0;
  if (std::scanf("%u %u %u %u %llu", &nq, &cap, &kind, &tl, &ef) != 5 || kind > 2 || !nq || !cap) return 2;
  std::vector<uint32_t> qlist(nq), xlist(nq), status(nq, 0u);  // (exactly nq words each: the sanitizer build sees an overrun)
  RoundScheduler s((Kind)kind, tl != 0, nq, cap, qlist.data(), xlist.data());
  const uint64_t most = max_rounds(nq, cap, ef);
  uint64_t r = 0;
  uint32_t started = kind == 0 ? nq : 0;  // a batch that re-runs starts every query at once
  auto print = [&]() {
    std::printf("round %llu listed %d q", (unsigned long long)r, s.listed() ? 1 : 0);
    for (uint32_t i = 0; s.listed() && i < s.active(); ++i) { std::printf(" %u", qlist[i]); started = std::max(started, qlist[i] + 1); }
    if (!s.listed()) { std::printf(" [0,%u)", s.active()); started = std::max(started, s.active()); }
    std::printf(" x");
    for (uint32_t i = 0; i < s.exact(); ++i) { std::printf(" %u", xlist[i]); started = std::max(started, xlist[i] + 1); }
  };
  s.first();
  print();
  std::printf(" -> launch\n");
  for (;;) {
    r += 1;
    uint32_t misses = 0;
    for (uint32_t i = 0; i < started; ++i) {
      if (std::scanf("%u", &status[i]) != 1) return 3;
      misses += status[i] == QS_BLOCKED || status[i] == QS_BLOCKED_X;
    }
    Verdict v = s.next(status.data(), misses);
    if (v == Verdict::SHORT_WINDOWS) {
      unsigned n = 0;
      if (std::scanf("%u", &n) != 1 || n > nq) return 3;
      for (uint32_t i = 0; i < n; ++i)
        if (std::scanf("%u", &qlist[i]) != 1) return 3;
      print();
      std::printf(" -> short\n");
      v = s.restart_short(n);
    }
    print();
    std::printf(" -> %s\n", name(v));
    if (v == Verdict::FINAL) break;
    if (r > most) { std::printf("round cap exceeded\n"); return 1; }
  }
  std::printf("rounds %llu of %llu\n", (unsigned long long)r, (unsigned long long)most);
  return 0;
}

int main() {
  char what[16] = {0};
  if (std::scanf("%15s", what) != 1) return 2;
  if (!std::strcmp(what, "caps")) return caps();
  if (!std::strcmp(what, "rounds")) return rounds();
  return 2;
}
