// Launch geometry of the search path: which kernel answers a call, with how much LDS per wave, on
// how many resident waves, with what table sizes.  Host-only arithmetic over the index's fields;
// search.hip takes every such figure from the one CallGeometry record of a call, so the table size
// a kernel is told and the LDS / state block reserved for it cannot disagree.
// tests/cpp/geometry_dump.cpp prints these functions over a grid of calls without a device.
#pragma once

#include "search_kernels.hip.h"

namespace {

constexpr size_t kCuLdsBytes = 160 * 1024;  // LDS of one CU
constexpr size_t kMaxWavesPerCu = 16;       // resident waves per CU the launch geometry may count on
constexpr uint32_t kMaxExactEf = 4096;

// resident waves per CU that `lds` bytes of LDS per wave leave room for (0: one wave does not fit)
inline size_t waves_per_cu(size_t lds) { return std::min(kMaxWavesPerCu, kCuLdsBytes / lds); }
// ... and on the whole device (a launch runs on at least one wave per CU)
inline uint32_t resident_waves(int ncu, size_t lds) {
  return std::max<uint32_t>(1, (uint32_t)ncu * (uint32_t)std::max<size_t>(1, waves_per_cu(lds)));
}
// result-set segments of 64 entries the fast kernel is instantiated with
inline int fast_segments(uint32_t ef) { return ef <= 64 ? 1 : ef <= 128 ? 2 : ef <= 256 ? 4 : 8; }
// qbytes = bytes per query element in LDS: 4, or 2 for the instantiations that keep a bf16-valued
// query as bf16 (bf16 rows; at d = 4096 the query is what bounds the waves per CU)
// (+ 64 bytes when d is not a multiple of 16: the operand prefetch of direct_group may touch the
// rest of the last step)
inline size_t query_lds_bytes(uint32_t d, uint32_t qbytes) {
  return qbytes == 2 ? (size_t)((d + 7) / 8 * 8) * 2 + 64 : (size_t)((d + 3) / 4 * 4) * 4 + ((d & 15) ? 64 : 0);
}

struct FastGeom {
  uint32_t hbits;  // the table ef (and a long query) alone give: 1 << hbits entries; what parked queries' state blocks hold
  size_t lds;
  uint32_t hcap;   // entries of the table this launch runs with (1 << hbits unless the index's hint enlarged it)
};

// vhint = distance evaluations per query this index's searches have been making (0 = unknown): every
// evaluated node is an entry of the visited table.
// fixed_table: the launch's table is 1 << hbits entries whatever else is set (the two-level search, and
// searches that park: their LDS and state blocks are sized by hbits)
inline FastGeom fast_geometry(uint32_t ef, uint32_t d, uint32_t qbytes = 4, uint32_t vhint = 0, bool fixed_table = false) {
  // visited capacity grows with ef (V is roughly 10-30 x ef); overflow goes to HBM
  uint32_t hbits = ef <= 64 ? 10 : ef <= 160 ? 11 : ef <= 320 ? 12 : 13;
  static const int hbits_env = [] { const char* e = getenv("ISL_HBITS"); return e ? atoi(e) : 0; }();
  // A long query takes most of a wave's LDS (d = 4096: 16 KB as float32, 8 KB as bf16) and the waves
  // per CU with it; once it is at least as large as the visited table, half a table buys more
  // through occupancy than it costs through the overflow table in HBM (10M x 4096 bf16 rows,
  // ef = 128: 0.40 -> 0.45 of the HBM peak).  At d = 768 the full table wins and stays.
  const size_t qlds = (size_t)d * qbytes;
  if (qlds >= ((size_t)4 << hbits) && hbits > 9) hbits -= 1;
  // visited table, merge buffer, query
  const size_t rest = (size_t)mbuf_entries(ef) * 8 + query_lds_bytes(d, qbytes);
  if (hbits_env >= 8 && hbits_env <= 14) hbits = (uint32_t)hbits_env;  // experiments only
  uint32_t hcap = 1u << hbits;
  // Round 4: a larger table when the index's queries have been filling it past its 7/8 limit on average.
  // How many nodes a query evaluates is a property of the graph and the data, not of ef alone (ef = 128: 1226
  // on the tree-of-clusters rows with the harness graph, 3100-3400 on manifold rows with an exact-kNN graph),
  // and a query past the limit pays an atomic round trip to its HBM overflow table for every further hop:
  // measured on the latter rows (1M x 768, 20 steps, profiles/r04_bench_M_knn_1m_hbits{11,12,13}.json)
  // 2048 entries 558 k queries/s, 4096 entries 686 k (12 -> 7 waves per CU and still +23 %), 8192 entries 602 k.
  // The table need not be a power of two (hslot_cap): it takes what the average query needs, in steps of 512
  // entries and at most four times the default, and then whatever else fits beside the same number of waves per CU.
  static const bool no_hint = getenv("ISL_NO_VISITED_HINT") != nullptr;  // A/B switch for measurements
  static const int hcap_env = [] { const char* e = getenv("ISL_HCAP"); return e ? atoi(e) : 0; }();  // experiments only
  if (vhint && !no_hint && hbits_env == 0 && !fixed_table) {
    const uint64_t need = ((uint64_t)vhint * 8 + 6) / 7;
    if (need > hcap) {
      const uint64_t most = (uint64_t)4 << hbits;  // (2 x until the densest graph of DESIGN section 4: 4096 entries 357 k, 5696 420 k queries/s)
      uint64_t want = std::min<uint64_t>((need + 511) / 512 * 512, most);
      auto lds_of = [&](uint64_t cap) { return (cap * 4 + rest + 511) / 512 * 512; };  // (LDS is handed out in 512-byte granules)
      auto room = [&](size_t waves) -> uint64_t {  // the largest table that leaves `waves` waves per CU
        const size_t each = kCuLdsBytes / waves / 512 * 512;
        return each > rest ? std::min<uint64_t>((each - rest) / 4 / 64 * 64, most) : 0;
      };
      const size_t per_cu = std::max<size_t>(1, kCuLdsBytes / lds_of(want));
      want = std::max(want, room(per_cu));           // what fits beside the same waves is free
      if (room(per_cu + 1) >= need) want = room(per_cu + 1);  // one more wave per CU if the average query still fits
      hcap = (uint32_t)want;
    }
  }
  if (hcap_env >= 256 && hcap_env <= 16384 && !fixed_table) hcap = (uint32_t)hcap_env / 64 * 64;
  const size_t lds = (size_t)hcap * 4 + rest;
  return {hbits, lds, hcap};
}

inline size_t exact_lds(uint32_t ef, uint32_t d) {
  return (size_t)TILE_ROWS * TILE_LD * 4 + 64 * 4 + 64 * 4 + 8 * 4 + (size_t)(ef + 1) * 8 + 16 +
         (size_t)((d + 3) / 4 * 4) * 4;
}
// the greedy descent through an HnswGraph's upper layers holds the query alone
// (bf16 rows: their distance routine walks the query in steps of 32 elements and fetches the operand of a step
// whole, the last one included -- d rounded up to whole steps, as build_plan.hpp's query_floats_bf16)
inline size_t descent_lds(uint32_t d, bool bf16_rows = false) {
  return (size_t)(bf16_rows ? (d + 31) / 32 * 32 : (d + 3) / 4 * 4) * 4 + 64;
}

// Two-level search: LDS of one wave = visited table + approximate-queue window + R + staging + query
struct TwoLevelCall {
  float ratio;
  uint32_t window_scale = 1;  // the window grows 4x per retry after a query outgrew it
};
inline size_t two_level_lds(uint32_t hbits, uint32_t wcap, uint32_t ef, uint32_t d, uint32_t qbytes = 4) {
  return ((size_t)4 << hbits) + (size_t)(wcap + 64) * 8 + (size_t)tl_res_entries(ef) * 8 + 64 * 8 +
         128 * 4 + (size_t)kTlLdsWords * 4 + query_lds_bytes(d, qbytes);
}

inline uint32_t push_log_cap(uint32_t ef) { return std::max<uint32_t>(1024, 12 * ef); }  // pushes per query ~ 3-6 x ef

// Launch geometry of one call: which kernel answers it and what its lane must hold.
struct CallGeometry {
  uint32_t ef = 0;
  bool use_fast = false;
  int segments = 1;        // the fast kernel's S
  FastGeom fg{};           // visited table (p.hbits, p.hcap) and, for the fast kernel, LDS of a wave
  uint32_t slots = 0;      // resident waves of the launch
  uint32_t vhint = 0;      // evaluations per query the visited table was sized for (0 = by ef alone)
  // the fast kernel's bf16-query instantiation, which runs in front on bf16 rows of up to 64 ids
  // (qh; otherwise a copy of fg / slots)
  bool qh = false;
  FastGeom fgq{};
  uint32_t slots_q = 0;
  uint32_t plog_cap = 0;
  size_t exact_lds = 0, descent_lds = 0;
  uint32_t tl_wcap = 0;
  size_t tl_lds = 0;
  uint32_t tl_hbits_q = 0;   // the bf16-query instantiation: visited-table bits, LDS, resident waves
  size_t tl_lds_q = 0;
  uint32_t tl_slots_q = 0;
  uint32_t state_words = 0;  // words of one parked query of this call's traversal kernel (recompute provider)
  uint32_t lane_slots = 0;   // the most resident waves of any launch of the call: the slots its lane holds scratch for
};

inline isl_status call_geometry(const isl_index* idx, uint64_t d, uint64_t k, uint64_t ef_in, const TwoLevelCall* tl,
                                CallGeometry& g) {
  g.ef = (uint32_t)std::min<uint64_t>(std::max(ef_in, k), 0xFFFFFFFFull);  // leann.rs:890
  if (std::max(ef_in, k) > kMaxExactEf)
    return isl::fail(ISL_ERR_UNSUPPORTED, "ef = %llu exceeds the device limit %u",
                     (unsigned long long)std::max(ef_in, k), kMaxExactEf);
  const uint32_t ef = g.ef;
  const int ncu = isl::device_cu_count(idx->device);
  // (searches over the recompute provider park their visited table in state blocks sized by ef alone; the
  // two-level search sizes its own LDS: neither takes the hint)
  const bool fixed_table = tl || idx->recompute;
  g.vhint = 0;
  if (!fixed_table) {  // (the evaluations of a call with another ef say nothing about this one)
    const uint64_t h = idx->evals_hint.load(std::memory_order_relaxed);
    if ((uint32_t)(h >> 32) == ef) g.vhint = (uint32_t)h;
  }
  g.fg = fast_geometry(ef, (uint32_t)d, 4, g.vhint, fixed_table);
  g.segments = fast_segments(ef);
  // resident waves per CU: bounded by LDS (visited table + query) and by the kernel's VGPR
  // budget (<= 128 -> 4 per SIMD)
  g.use_fast = !tl && ef <= 512 && ef >= 1 && idx->max_degree <= 128 && waves_per_cu(g.fg.lds) > 0;
  g.slots = resident_waves(ncu, g.fg.lds);
  // bf16 rows: first the kernel that keeps the query as bf16 in LDS (half the LDS per wave, more
  // waves per CU), then the float32-query kernel over the queries that one passed on
  g.qh = g.use_fast && idx->rows.is_bf16() && idx->max_degree <= 64;
  g.fgq = g.qh ? fast_geometry(ef, (uint32_t)d, 2, g.vhint, fixed_table) : g.fg;
  if (tl) {
    // Window of the approximate queue: ceil(a * |AQ|) must stay inside it.  |AQ| is bounded by the
    // node count and runs at about 10 x ef (1235 at ef = 128 on the 10M-node bench graph); 20 x ef
    // covers the long queries, and one that outgrows it is re-run alone with four times the window
    // (never answered differently).  The window is most of a wave's LDS: round 2 sized it for
    // 32 x ef and ran 3 waves per CU at d = 4096.
    const float a = tl->ratio > 0.0f ? std::min(tl->ratio, 1.0f) : 0.0f;
    const double bound = (double)std::min<uint64_t>(idx->ncodes, (uint64_t)20 * ef * tl->window_scale);
    const uint64_t want = (uint64_t)(a * bound) + 64;
    g.tl_wcap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((want + 63) / 64 * 64, 256), 16384);
    while (g.tl_wcap > 256 && two_level_lds(g.fg.hbits, g.tl_wcap, ef, (uint32_t)d) > kCuLdsBytes) g.tl_wcap -= 64;
    g.tl_lds = two_level_lds(g.fg.hbits, g.tl_wcap, ef, (uint32_t)d);
    if (g.tl_lds > kCuLdsBytes)
      return isl::fail(ISL_ERR_UNSUPPORTED, "two-level search: ef = %u, d = %llu do not fit the LDS", ef,
                       (unsigned long long)d);
    g.slots = resident_waves(ncu, g.tl_lds);
    // bf16 rows: the queries whose elements are bf16 values keep their query as bf16 in LDS
    g.tl_hbits_q = fast_geometry(ef, (uint32_t)d, 2).hbits;
    g.tl_lds_q = two_level_lds(g.tl_hbits_q, g.tl_wcap, ef, (uint32_t)d, 2);
    g.tl_slots_q = resident_waves(ncu, g.tl_lds_q);
  }
  g.slots_q = g.qh ? resident_waves(ncu, g.fgq.lds) : g.slots;
  g.lane_slots = std::max(std::max(g.slots, g.slots_q), g.tl_slots_q);
  g.state_words = tl ? isl_launch::tl_state_words(ef, g.tl_wcap, g.fg.hbits)
                     : isl_launch::fast_state_words(g.segments, g.fg.hbits);
  g.plog_cap = push_log_cap(ef);
  g.exact_lds = exact_lds(ef, (uint32_t)d);
  g.descent_lds = descent_lds((uint32_t)d, idx->is_hnsw && idx->rows.is_bf16());  // (an HnswGraph alone descends)
  return ISL_OK;
}

}  // namespace
