// What the two graph builders share (build.hip: LeannIndex::build and the kernels; hnsw_build.hip:
// HnswGraph::insert over per-layer tables).  Internal, not part of the ABI.
#pragma once

#include "common.hpp"

namespace isl_build {

struct BuildParams {
  const float* emb;
  const float* norm2;
  uint64_t stride;
  uint32_t d;
  uint32_t* ell;       // [n][W]
  uint32_t* ell_deg;   // [n]
  uint32_t* lock;      // [n]
  uint32_t W, m0;
  uint32_t ef;         // candidates per new node (row pitch of cand_*)
  const uint64_t* cand_ids;   // [B][ef] ascending distance (search output)
  const float* cand_dist;
  const uint32_t* cand_cnt;   // [B]
  uint32_t* sel;       // [B][m0] selected neighbours
  uint32_t* sel_cnt;   // [B]
  uint64_t id0;        // first node of the step
  uint32_t B;
  float hub_percentile;
  uint32_t high_degree;  // LeannConfig::high_degree_pruning
  uint32_t locking;      // batch > 1
  float alpha;           // ISL_SELECT_DIVERSE: occlusion factor
  uint32_t keep_pruned;  // ISL_SELECT_DIVERSE: occluded candidates fill a short row
  // HnswGraph builder: ell / ell_deg / W / m0 are those of ONE layer
  const uint32_t* node_ids;     // [B] the new nodes of the step that have this layer (instead of id0 + b)
  const uint32_t* node_levels;  // [n] HnswNode::level
  uint32_t layer;
  uint32_t* cur_of;             // [n] `current` of every node being inserted: selected[0] after a layer
};

// struct_size, rule and alpha of caller-supplied options, before any device call
isl_status check_build_options(const isl_build_options* o, bool need_rule);
// bytes of LDS of the selection kernels (tile, query, lists of up to nmax candidates, a row of M) and of
// the reference-rule link kernel
size_t select_lds(uint64_t d, uint32_t nmax, uint32_t M);
size_t link_lds(uint64_t d);

// take(m0) of the search result (select_kernel without the hub rule: p.high_degree == 0)
void select_truncate(uint32_t grid, const BuildParams& p);
void select_diverse(int metric, uint32_t grid, size_t lds, const BuildParams& p);
// link_kernel in its HnswGraph mode (insert_node, hnsw.rs:295-318)
void link_hnsw(int metric, bool diverse, uint32_t grid, size_t lds, const BuildParams& p);
// fixed-width table -> CSR neighbours (one wave per row)
void ell_to_csr(const uint32_t* ell, const uint32_t* deg, uint32_t W, const uint64_t* off, uint64_t n,
                       uint32_t* adj);

}  // namespace isl_build
