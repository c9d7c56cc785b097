// Host-only arithmetic of the two graph builders (build.hip, hnsw_build.hip): which nodes a step inserts,
// how much LDS the selection and link kernels are launched with, what the device tables can hold.  Plain
// C++ without a device header, in the manner of search_geometry.hpp: tests/cpp/build_plan_dump.cpp prints
// the planner's steps with g++ alone (tests/test_hnsw_build_cpu.py).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace isl_plan {

// ---- what the device tables hold
constexpr uint64_t kMaxM0 = 128;              // a row under re-selection is m0 + 1 <= 129 ids: three slices of 64
constexpr uint64_t kMaxEfConstruction = 512;  // the lists of a selection live in LDS
constexpr uint64_t kMaxNodes = 0x7FFFFFF0ull; // 32-bit ids, one flag bit
// NULL, or why the device builders refuse the shape
inline const char* shape_limit(uint64_t m0, uint64_t ef_construction, uint64_t n) {
  if (m0 > kMaxM0) return "the device builder keeps rows of up to 129 ids: m0 <= 128";
  if (ef_construction > kMaxEfConstruction) return "ef_construction <= 512 on the device";
  if (n >= kMaxNodes) return "num_nodes exceeds the device id range";
  return nullptr;
}

// ---- steps
// A step never inserts more than an eighth of the nodes already in the graph: the nodes of a step cannot
// see each other, and a young graph would otherwise end up as a star.
inline uint64_t ramp(uint64_t batch, uint64_t n, uint64_t id0) {
  return std::min<uint64_t>(std::min<uint64_t>(batch, n - id0), std::max<uint64_t>(1, id0 / 8));
}

// One step of the plan: nodes order[first .. first + count), sorted by level (highest first).
struct Step {
  uint64_t first;
  uint32_t count;
  uint32_t top;  // the step's highest level
};

// ramp() nodes per step for nodes n0 .. n-1 of `lv` (all n levels), the graph holding nodes 0 .. n0-1 with top
// layer max_level0; cut so that a node above the current top layer is the only node of its step.  n0 = 0 is
// the empty graph: node 0 starts it (no step) and the plan begins at node 1 under lv[0].  All-zero levels
// (LeannIndex::build, whose levels do not shape the graph) are never cut and leave `order` the identity.
inline void plan_steps_from(const std::vector<uint32_t>& lv, uint64_t n0, uint32_t max_level0, uint64_t batch,
                            std::vector<Step>& steps, std::vector<uint32_t>& order) {
  const uint64_t n = lv.size();
  order.resize(n);
  for (uint64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
  uint32_t max_level = n0 ? max_level0 : (n ? lv[0] : 0);
  for (uint64_t id0 = n0 ? n0 : 1; id0 < n;) {
    uint64_t nb = ramp(batch, n, id0);
    if (lv[id0] > max_level) {
      nb = 1;
    } else {
      for (uint64_t j = 1; j < nb; ++j)
        if (lv[id0 + j] > max_level) { nb = j; break; }
    }
    uint32_t top = 0;
    for (uint64_t j = 0; j < nb; ++j) top = std::max(top, lv[id0 + j]);
    if (top > 0 && nb > 1)
      std::stable_sort(order.begin() + id0, order.begin() + id0 + nb, [&](uint32_t a, uint32_t b) { return lv[a] > lv[b]; });
    steps.push_back(Step{id0, (uint32_t)nb, top});
    max_level = std::max(max_level, top);
    id0 += nb;
  }
}

// the whole collection: from node 1 on, node 0 having started the graph
inline void plan_steps(const std::vector<uint32_t>& lv, uint64_t batch, std::vector<Step>& steps,
                       std::vector<uint32_t>& order) {
  plan_steps_from(lv, 1, lv.empty() ? 0 : lv[0], batch, steps, order);
}

// the most nodes any step inserts (>= 1): what the per-step buffers are sized for
inline uint64_t largest_step(const std::vector<Step>& steps) {
  uint64_t b = 1;
  for (const Step& s : steps) b = std::max<uint64_t>(b, s.count);
  return b;
}

// ---- LDS
// floats of a wave's query in LDS behind the distance tile: d rounded up to whole float4 plus 16 of slack
// (the kernels lay their lists out behind it, the host reserves it)
constexpr uint32_t query_floats(uint32_t d) { return (d + 3u) / 4u * 4u + 16u; }
// bytes of LDS of the reference-rule link kernel and the insertion descent: tile + query
constexpr size_t link_lds(size_t tile_bytes, uint32_t d) { return tile_bytes + (size_t)query_floats(d) * 4; }
// ... and of a selection: four lists of up to nmax candidates and a row of M behind the query
constexpr size_t select_lds(size_t tile_bytes, uint32_t d, uint32_t nmax, uint32_t M) {
  return link_lds(tile_bytes, d) + (size_t)nmax * 16 + (size_t)M * 4;
}
// bf16 rows: the kernels measure with the tile-free routine (direct_distances over 16-byte loads of 8
// elements), so there is no tile -- the LDS is the query, widened to f32, plus the lists.  That routine
// walks the query in steps of 32 elements and fetches the operand of a step whole, the last one included:
// d rounded up to whole steps, plus the same 16 of slack.
constexpr uint32_t query_floats_bf16(uint32_t d) { return (d + 31u) / 32u * 32u + 16u; }
constexpr size_t link_lds_bf16(uint32_t d) { return (size_t)query_floats_bf16(d) * 4; }
constexpr size_t select_lds_bf16(uint32_t d, uint32_t nmax, uint32_t M) {
  return link_lds_bf16(d) + (size_t)nmax * 16 + (size_t)M * 4;
}

}  // namespace isl_plan
