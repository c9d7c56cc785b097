// Prints what one enqueue launches (islands_amd/csrc/search_launch_plan.hpp) over a grid of calls: per case one
// summary line (the call, the figures of its geometry the steps draw on, the call-level facts) and one line per
// step.  Needs no device (an index whose device is -1 answers 256 compute units); the facts are filled by hand.
// tests/test_search_launch_plan_cpu.py compares the output with hand-written sequences and with
// tests/golden/search_launch_plan.txt.
#include "../../islands_amd/csrc/search_launch_plan.hpp"
#include <cstdio>
#include <cstring>
#include <initializer_list>

using isl_lane::RoundPlan;

namespace {

const char* kind_name(StepKind k) {
  switch (k) {
    case StepKind::SeedRedo: return "SeedRedo";
    case StepKind::PqTables: return "PqTables";
    case StepKind::Classify: return "Classify";
    case StepKind::TwoLevel: return "TwoLevel";
    case StepKind::Descent: return "Descent";
    case StepKind::EntryPick: return "EntryPick";
    case StepKind::Fast: return "Fast";
    case StepKind::FillRedoAll: return "FillRedoAll";
    case StepKind::Exact: return "Exact";
  }
  return "?";
}

struct Variant {
  const char* name;
  bool two_level, hnsw;
  uint32_t max_level;
  bool seeds, build, recompute, warm;
  RoundPlan rp;
  bool prepare_reaches;  // isl_index_prepare / group_prepare can make this launch (warm variants)
};

RoundPlan round(uint32_t active, uint32_t exact, bool listed, bool exact_parks = false, bool tables_built = false,
                uint32_t prefetch = 0) {
  RoundPlan rp;
  rp.active = active;
  rp.exact = exact;
  rp.listed = listed;
  rp.exact_parks = exact_parks;
  rp.tables_built = tables_built;
  rp.prefetch = prefetch;
  return rp;
}
RoundPlan retry(uint32_t n, uint32_t scale) {
  RoundPlan rp;
  rp.retry = n;
  rp.window_scale = scale;
  rp.tables_built = true;
  return rp;
}

}  // namespace

int main() {
  isl_index* idx = new isl_index();
  idx->device = -1;
  idx->ncodes = 1000000;
  const uint32_t d = 100, k = 10;
  const struct { const char* name; int dtype; } dtypes[] = {
      {"f32", ISL_DTYPE_F32}, {"bf16", ISL_DTYPE_BF16}, {"fp8", ISL_DTYPE_FP8_E4M3}};
  for (const auto& dt : dtypes)
    for (uint32_t deg : {64u, 65u, 128u, 129u})
      for (uint32_t ef : {10u, 128u, 512u, 513u})
        for (uint32_t nq : {1u, 70u, 5000u}) {
          // a round's figures follow nq: a first round over all of it, a listed one over half, one with only
          // queries parked in the heap-exact kernel, a two-level round that resumes
          const uint32_t half = std::max(1u, nq / 2);
          const Variant variants[] = {
              {"plain", false, false, 0, false, false, false, false, RoundPlan{}, false},
              {"hnsw0", false, true, 0, false, false, false, false, RoundPlan{}, false},
              {"hnsw2", false, true, 2, false, false, false, false, RoundPlan{}, false},
              {"seeds", false, false, 0, true, false, false, false, RoundPlan{}, false},
              {"build", false, true, 2, false, true, false, false, RoundPlan{}, false},
              {"build+seeds", false, false, 0, true, true, false, false, RoundPlan{}, false},
              {"tl", true, false, 0, false, false, false, false, RoundPlan{}, false},
              {"tl+seeds", true, false, 0, true, false, false, false, RoundPlan{}, false},
              {"tl-retry4", true, false, 0, false, false, false, false, retry(half, 4), false},
              {"rec-first", false, false, 0, false, false, true, false, round(nq, 0, false), false},
              {"rec-first-parks", false, false, 0, false, false, true, false, round(nq, 0, false, true), false},
              {"rec-listed", false, false, 0, false, false, true, false, round(half, 3, true, true), false},
              {"rec-exact-only", false, false, 0, false, false, true, false, round(0, 5, true, true), false},
              {"rec-rerun", false, false, 0, true, false, true, false, RoundPlan{}, false},
              {"rec-tl-first", true, false, 0, false, false, true, false, round(nq, 0, false, false, false, 4), false},
              {"rec-tl-resume", true, false, 0, false, false, true, false, round(half, 0, true, false, true, 4), false},
              {"warm-plain", false, false, 0, false, false, false, true, RoundPlan{}, true},
              {"warm-hnsw0", false, true, 0, false, false, false, true, RoundPlan{}, true},
              {"warm-hnsw2", false, true, 2, false, false, false, true, RoundPlan{}, true},
              {"warm-seeds", false, false, 0, true, false, false, true, RoundPlan{}, true},
              {"warm-build", false, true, 2, false, true, false, true, RoundPlan{}, true},
              {"warm-tl", true, false, 0, false, false, false, true, RoundPlan{}, dt.dtype != ISL_DTYPE_FP8_E4M3},
              {"warm-rec", false, false, 0, false, false, true, true, RoundPlan{}, true},
              {"warm-rec-tl", true, false, 0, false, false, true, true, RoundPlan{}, dt.dtype != ISL_DTYPE_FP8_E4M3},
          };
          for (const Variant& v : variants) {
            // The plain call runs row type x degree x ef at 70 queries, and 1 and 5000 queries at two ef.  The others
            // run the base shape (64 ids, ef 128) over f32 and bf16 rows; those whose sequence depends on the fast
            // kernel also run, over f32 rows, one shape past each of its limits (129 ids; ef 513); the descent and a
            // first round also run at 5000 queries.
            auto among = [&](std::initializer_list<const char*> names) {
              for (const char* n : names)
                if (!strcmp(n, v.name)) return true;
              return false;
            };
            const bool is_plain = &v == &variants[0], base = deg == 64 && ef == 128;
            const bool fp8 = dt.dtype == ISL_DTYPE_FP8_E4M3, f32 = dt.dtype == ISL_DTYPE_F32;
            if (is_plain && nq != 70 && (fp8 || deg != 64 || ef > 128)) continue;
            if (!is_plain) {
              const bool past = f32 && ((deg == 129 && ef == 128) || (deg == 64 && ef == 513)) &&
                                among({"hnsw2", "seeds", "build", "tl", "rec-first", "rec-listed", "rec-exact-only",
                                       "rec-rerun", "warm-plain", "warm-hnsw2"});
              if (fp8 || !(base || past)) continue;
              if (nq == 1 || (nq == 5000 && !(base && among({"hnsw2", "rec-first"})))) continue;
            }
            if (v.warm && (!v.prepare_reaches || nq != 70)) continue;  // (a warm call has no queries: once per shape)
            if (v.two_level && dt.dtype == ISL_DTYPE_FP8_E4M3) continue;  // (no two-level search over fp8 rows)
            idx->max_degree = deg;
            idx->rows.set_dtype(dt.dtype);
            idx->recompute = v.recompute;
            idx->is_hnsw = v.hnsw;
            idx->evals_hint.store(0);
            LaunchFacts f;
            f.dtype = dt.dtype;
            f.metric = 0;
            f.is_hnsw = v.hnsw;
            f.max_level = v.max_level;
            f.recompute = v.recompute;
            f.max_degree = deg;
            f.seeds = v.seeds;
            f.build_q_entry = v.build;
            f.pool_slots = 32;
            const uint64_t call_nq = v.warm ? 0 : nq;
            TwoLevelCall t{0.5f, v.rp.window_scale};
            CallGeometry cg;
            const isl_status st = call_geometry(idx, d, k, ef, v.two_level ? &t : nullptr, cg);
            printf("case %s %s deg=%u ef=%u nq=%llu", v.name, dt.name, deg, ef, (unsigned long long)call_nq);
            if (st != ISL_OK) { printf(" -> status %d\n", (int)st); continue; }
            const LaunchPlan lp = plan_launches(f, CallShape{call_nq, v.two_level}, v.rp, v.warm, cg);
            // (figures and facts that are zero are left out)
            auto fig = [](const char* name, unsigned long long v) { if (v) printf(" %s=%llu", name, v); };
            printf(" | lds");
            fig("fg", cg.fg.lds), fig("fgq", cg.fgq.lds), fig("tl", cg.tl_lds), fig("tlq", cg.tl_lds_q);
            fig("exact", cg.exact_lds), fig("descent", cg.descent_lds);
            // the call-level facts: the flags that are set, then the figures
            printf(" | plan steps=%u flags=", lp.count);
            const struct { const char* name; bool on; } flags[] = {
                {"two_level", lp.two_level}, {"use_fast", lp.use_fast}, {"resume", lp.resume}, {"seeded", lp.seeded},
                {"prepare_lane", lp.prepare_lane}, {"wants_ell", lp.wants_ell}, {"measures", lp.measures},
                {"construction", lp.construction}, {"entry_given", lp.entry_given},
                {"exact_park_fields", lp.exact_park_fields}, {"qsel", lp.qsel}, {"publishes", lp.publishes}};
            for (const auto& fl : flags)
              if (fl.on) printf("%s,", fl.name);
            fig("lane_slots", lp.lane_slots), fig("nq", lp.nq), fig("max_level", lp.max_level);
            fig("q_entry_words", lp.q_entry_words), fig("qlist", (unsigned)lp.qlist), fig("tl_prefetch", lp.tl_prefetch);
            printf("\n");
            for (uint32_t i = 0; i < lp.count; ++i) {
              const LaunchStep& s = lp.steps[i];
              // (selectors: S, wide, dtype, resume, qh, bf16, hnsw, metric)
              printf(" step %s grid=%u lds=%zu nq=%u hbits=%u hcap=%u qsel_mode=%u sel=%d,%d,%d,%d,%d,%d,%d,%d\n",
                     kind_name(s.kind), s.grid, s.lds, s.nq, s.hbits, s.hcap, s.qsel_mode, s.S,
                     (int)s.wide, s.dtype, (int)s.resume, (int)s.qh, (int)s.bf16, (int)s.hnsw, s.metric);
            }
          }
        }
  return 0;
}
