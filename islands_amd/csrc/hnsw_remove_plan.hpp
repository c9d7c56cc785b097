// Host-only arithmetic of isl_hnsw_remove (hnsw_build.hip) on top of remove_plan.hpp: how many layers the shrunk
// graph has, how many survivors each layer holds, how a (layer, node) pair of the touched list is packed and the
// LDS of the one repair launch that serves every layer.  Plain C++ without a device header:
// tests/cpp/hnsw_remove_plan_dump.cpp prints it with g++ alone (tests/test_hnsw_remove_cpu.py).
#pragma once

#include "remove_plan.hpp"

namespace isl_plan {

// the device builders keep up to 64 layers (hnsw_build.hip, all_levels)
constexpr uint64_t kMaxLayers = 64;

// One entry of the touched list: a survivor that lost a neighbour on one layer.  Ids stay below kMaxNodes
// (32 bits), layers below kMaxLayers.
constexpr uint64_t touched_pair(uint32_t layer, uint32_t node) { return ((uint64_t)layer << 32) | node; }
constexpr uint32_t pair_layer(uint64_t pair) { return (uint32_t)(pair >> 32); }
constexpr uint32_t pair_node(uint64_t pair) { return (uint32_t)pair; }

// ids a list of `layer` keeps: m0 on layer 0, m above
constexpr uint32_t layer_cap(uint32_t layer, uint32_t m, uint32_t m0) { return layer ? m : m0; }

// layers of the shrunk graph: max_level + 1 of the entry rule's answer (the layers above cease to exist); a graph
// without nodes or without entry point has none above 0
inline uint64_t layers_after(const Entry& e) { return e.has ? e.max_level + 1 : 1; }

// members[L] = survivors whose level is at least L, for the `layers` layers of the OLD graph: the rows of layer L
// that can hold a list, so their sum bounds the touched list.  `levels`: of all old nodes.
inline std::vector<uint64_t> layer_members(const std::vector<uint64_t>& levels, const std::vector<uint32_t>& survivors,
                                           uint64_t layers) {
  std::vector<uint64_t> members(layers, 0);
  for (uint32_t s : survivors) {
    const uint64_t lv = s < levels.size() ? levels[s] : 0;
    for (uint64_t L = 0; L < layers && L <= lv; ++L) ++members[L];
  }
  return members;
}
inline uint64_t touched_capacity(const std::vector<uint64_t>& members) {
  uint64_t sum = 0;
  for (uint64_t m : members) sum += m;
  return sum;
}

// LDS of the repair launch over all layers: the selection of remove_plan.hpp's repair_lds into a row of the
// larger of m0 and m (HnswConfig::validate has m0 >= m; a handle is not trusted to)
constexpr size_t hnsw_repair_lds(size_t tile_bytes, uint32_t d, uint32_t m, uint32_t m0) {
  return repair_lds(tile_bytes, d, m0 > m ? m0 : m);
}

}  // namespace isl_plan
