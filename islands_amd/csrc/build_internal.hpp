// What the two graph builders share (build.hip: LeannIndex::build, the kernels and the scaffold below;
// hnsw_build.hip: HnswGraph::insert over per-layer tables; build_plan.hpp: their host-only arithmetic).
// Internal, not part of the ABI.
#pragma once

#include "build_plan.hpp"
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
  // LeannIndex::build over bf16 rows (isl_index_build_rows): the table the kernels' bf16 instantiations read
  // instead of emb (NULL otherwise); stride is then in bf16 elements, norm2 is of the widened values
  const uint16_t* emb16;
};

// struct_size, rule and alpha of caller-supplied options, before any device call
isl_status check_build_options(const isl_build_options* o, bool need_rule);
// bytes of LDS of the reference-rule link kernel and of the insertion descent (tile + query)
size_t link_lds(uint64_t d);
// ISL_DTYPE_F32 / ISL_DTYPE_BF16, before any device call
isl_status check_row_dtype(int32_t dtype);

// One table the nodes of a step are inserted on: the whole graph of LeannIndex::build, or one layer of an
// HnswGraph under construction.
struct Table {
  uint32_t* ell;   // [n][M + 1]
  uint32_t* deg;   // [n]
  uint32_t M;      // ids a row keeps
};

// A construction in progress.  It owns the construction graph `g` (an isl_index whose adjacency is the table
// being searched), every temporary device allocation, the per-step buffers and, until release(), what the
// finished graph will keep.  Leaving the scope is the one failure path: everything is freed and the error
// record of the first failure survives the frees.
struct Scaffold {
  isl_index* g = nullptr;
  isl_index* res = nullptr;   // the finished index, once there is one
  isl::TempScope tmp;         // freed on every way out
  std::vector<isl::DeviceBuffer<unsigned char>> keep;  // res->hnsw_owned after release(), freed before it
  float* qbuf = nullptr;      // [B][d] queries of a step: the rows of its nodes
  uint64_t* cand_ids = nullptr;  // [B][ef] what the construction search found (p.cand_*)
  float* cand_dist = nullptr;
  uint32_t* cand_cnt = nullptr;
  BuildParams p{};            // rows, per-step buffers and rule parameters; insert() fills in the table
  bool diverse = false, hnsw = false;

  Scaffold() = default;
  Scaffold(const Scaffold&) = delete;
  Scaffold& operator=(const Scaffold&) = delete;
  ~Scaffold();

  // `count` elements on the device (at least one), owned by tmp or keep
  template <class T>
  isl_status alloc(T** out, uint64_t count, bool zero = false, bool kept = false) {
    return alloc_bytes((void**)out, count * sizeof(T), zero, kept);
  }
  isl_status alloc_bytes(void** out, uint64_t bytes, bool zero, bool kept);
  // The construction graph over `vectors` and the buffers of steps of up to B nodes, rows of up to m0 ids.
  // cfg: metric (and, for LeannIndex::build, the hub rule); opts: the selection rule.
  // dtype: what `vectors` holds and the construction graph stores (isl_set_embeddings); bf16 rows are for
  // LeannIndex::build alone (not with hnsw).
  // With `old` (a finished graph that grows, isl_index_insert / isl_hnsw_insert) the rows come from two sources:
  // the first old->nvec of the n are old's rows and norms, copied on the device; `vectors` holds the
  // n - old->nvec new ones, of old's stored type.
  isl_status open(const isl_leann_config& cfg, const isl_build_options& opts, bool hnsw, const void* vectors,
                  int32_t dtype, uint64_t n, uint64_t d, int32_t mem, int32_t device, uint64_t B, uint32_t m0,
                  uint32_t ef, const isl_index* old = nullptr);
  // Inserts `cnt` nodes on table `t`, their rows being in qbuf: construction search over the table, selection
  // (truncation / hub rule, or select()), links both ways.  The nodes are id0 .. id0 + cnt - 1, or node_ids[]
  // on `layer` of an HnswGraph.  Returns once the kernels are launched.
  isl_status insert(const Table& t, uint32_t cnt, bool locking, uint64_t id0, const uint32_t* node_ids = nullptr,
                    uint32_t layer = 0);
  // CSR arrays of a finished layer -> the first n0 rows of table `t` (one wave per row), the way back in
  // for a graph that grows.  *d_flag (device, zeroed by the caller) collects what the table cannot take:
  // 1 = a list longer than t.M, 2 = offsets that do not fit `nnz`, 4 = an id that is not below n0; such a
  // list is cut or left out, never written past its row.
  isl_status csr_to_table(const Table& t, const uint64_t* off, const uint32_t* adj, uint64_t nnz, uint64_t n0,
                          uint32_t* d_flag);
  // fixed-width table -> CSR arrays on the device (one wave per row)
  isl_status table_to_csr(const Table& t, uint64_t n, bool kept, uint64_t** off, uint32_t** adj);
  // success: the finished graph leaves with the construction graph's rows and what was kept for it
  isl_index* release();
};

// ---- what the two removals share (isl_index_remove in build.hip, isl_hnsw_remove in hnsw_build.hip; the kernels
// are build.hip's).  A graph that shrinks is a set of layers -- one for a flat index -- each with its OLD CSR, the
// table its lists return to and, once the repaired degrees are known, the CSR of the survivors.  The kernels read
// an array of these in device memory and take the layer from blockIdx.y or from the touched pair.
struct RemoveLayer {
  const uint64_t* off;      // the OLD CSR over the old ids: every list is computed from the old lists only
  const uint32_t* adj;
  uint32_t* ell;            // [n0][M + 1] the table: a touched row is written by its wave alone, never read
  uint32_t* deg;            // [n0]
  uint32_t M;               // ids a row of this layer keeps
  uint32_t reserved;
  const uint64_t* new_off;  // [n + 1] the survivors' CSR over the new ids (compact_lists)
  uint32_t* new_adj;
};

struct RepairParams {
  const void* emb;            // the OLD rows, by old id
  const float* norm2;
  uint64_t stride;
  uint32_t d;
  float alpha;
  uint32_t keep_pruned;
  const RemoveLayer* layers;  // device array
  const uint32_t* levels;     // [n0] HnswGraph: a node has layer L iff levels[node] >= L; NULL: every node has every layer
  const uint32_t* remap;      // [n0] new id or isl_plan::kGone
  const uint64_t* touched;    // [grid] isl_plan::touched_pair
  unsigned long long* total;  // [1] sum of |C(p)| over the touched pairs
};

// LDS of a repair launch whose widest layer keeps `widest` ids, for the rows' stored type
size_t repair_lds(const isl::RowTable& rows, uint32_t widest);
// The launches below return once the kernel is enqueued on the default stream.
// (layer, node) pairs of the survivors that lost a neighbour, all layers in one launch: d_counts [1 + layers],
// zeroed by the caller, receives the number of pairs and the pairs per layer; at most `cap` pairs are written.
isl_status list_touched(const RemoveLayer* d_layers, uint32_t layers, const uint32_t* d_levels, const uint32_t* d_remap,
                        uint64_t n0, uint64_t* d_pairs, uint32_t cap, uint32_t* d_counts);
// one wave per pair rebuilds the pair's table row
isl_status launch_repair(uint32_t metric, bool diverse, const isl::RowTable& rows, uint32_t grid, size_t lds,
                         const RepairParams& p);
// the tables of layers 0 .. layers-1 -> their new CSRs through the remap, one launch; *d_flag (zeroed by the caller)
// is raised by a removed id left in a survivor's row
isl_status compact_lists(const RemoveLayer* d_layers, uint32_t layers, const uint32_t* d_levels, const uint32_t* d_remap,
                         uint64_t n0, uint32_t* d_flag);
// rows and norms of the n survivors d_surv[] (old ids, ascending), bit for bit, into `out`, a fresh table of the
// same stored type (row_table.hpp has the layout)
isl_status gather_survivors(const isl::RowTable& rows, const uint32_t* d_surv, uint64_t n, isl::RowTable& out);

}  // namespace isl_build
