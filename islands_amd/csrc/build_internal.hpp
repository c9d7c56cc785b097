// What the two graph builders share (build.hip: LeannIndex::build, the kernels and the scaffold below;
// hnsw_build.hip: HnswGraph::insert over per-layer tables; build_plan.hpp: their host-only arithmetic).
// Internal, not part of the ABI.
#pragma once

#include "build_plan.hpp"
#include "common.hpp"
#include "remove_plan.hpp"
#include "row_compact_plan.hpp"

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
  // bf16 rows (isl_index_build_rows, isl_hnsw_build_rows): the table the kernels' bf16 instantiations read
  // instead of emb (NULL otherwise); stride is then in bf16 elements, norm2 is of the widened values
  const uint16_t* emb16;
};

// The options of a call: the defaults, or the caller's once struct_size, rule and alpha are checked (before any
// device call)
isl_status resolve_build_options(const isl_build_options* in, bool need_rule, isl_build_options& out);
// "the device copy of layer 0 is not the lists verbatim": the host lists are longer than what was uploaded, because
// ids repeated inside a list were removed at upload.  A builder that reads the device CSR back into its table
// would quietly build on another graph.
bool device_lists_differ(const isl_index* idx);
// old -> new ids of a removal for the caller, ISL_REMOVED for a removed one; `remap` NULL: nothing was removed
void write_remap(const std::vector<uint32_t>* remap, uint64_t n0, uint64_t* out_remap);
// bytes of LDS of the reference-rule link kernel and of the insertion descent over f32 rows (tile + query; bf16 rows:
// isl_plan::link_lds_bf16)
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
  isl::RowTable* appended = nullptr;  // the reserved table rows were appended to: zeroed behind its count on failure

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
  // dtype: what `vectors` holds and the construction graph stores (isl_set_embeddings): f32 or bf16, either builder.
  // With `old` (a finished graph that grows, isl_index_insert / isl_hnsw_insert) the rows come from two sources:
  // the first old->nvec of the n are old's rows and norms, copied on the device; `vectors` holds the
  // n - old->nvec new ones, of old's stored type.
  // With `into` (old's reserved table, or that of an empty handle, with room for all n rows) nothing is allocated or
  // copied: the new rows are filled in behind into->n() and the construction graph reads a view of the table.
  isl_status open(const isl_leann_config& cfg, const isl_build_options& opts, bool hnsw, const void* vectors,
                  int32_t dtype, uint64_t n, uint64_t d, int32_t mem, int32_t device, uint64_t B, uint32_t m0,
                  uint32_t ef, const isl_index* old = nullptr, isl::RowTable* into = nullptr);
  // Inserts `cnt` nodes on table `t`, their rows being in qbuf: construction search over the table, selection
  // (truncation / hub rule, or select()), links both ways.  The nodes are id0 .. id0 + cnt - 1, or node_ids[]
  // on `layer` of an HnswGraph.  Returns once the kernels are launched.
  isl_status insert(const Table& t, uint32_t cnt, bool locking, uint64_t id0, const uint32_t* node_ids = nullptr,
                    uint32_t layer = 0);
  // bf16 rows: the queries of a step, widened into qbuf -- nodes id0 .. id0 + cnt - 1, or node_ids[] of an HnswGraph
  // layer, whose searches also start where cur_of / evals_of say (g->build_q_entry / build_q_evals).  Enqueues one
  // kernel; the caller reads hipGetLastError.
  void gather_bf16(uint64_t id0, uint32_t cnt, const uint32_t* node_ids = nullptr, const uint32_t* cur_of = nullptr,
                   const uint32_t* evals_of = nullptr);
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

// ---- what the two removals share: the kernels and the one routine that drives them are build.hip's;
// isl_index_remove (build.hip) and isl_hnsw_remove (hnsw_build.hip) call it and make their own handle from what it
// returns.  A graph that shrinks is a set of layers -- one for a flat index -- each with its OLD CSR, the table its
// lists return to and, once the repaired degrees are known, the CSR of the survivors.  The kernels read an array of
// these in device memory and take the layer from blockIdx.y or from the touched pair.
struct RemoveLayer {
  const uint64_t* off;      // the OLD CSR over the old ids: every list is computed from the old lists only
  const uint32_t* adj;
  uint32_t* ell;            // [n0][M + 1] the table: a touched row is written by its wave alone, never read
  uint32_t* deg;            // [n0]
  uint32_t M;               // ids a row of this layer keeps
  uint32_t reserved;
  const uint64_t* new_off;  // [n + 1] the survivors' CSR over the new ids (table_to_csr_remap_kernel)
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

// One layer as its caller hands it in: the old CSR on the device and the ids a list of the layer keeps.
struct ShrinkLayer {
  const uint64_t* off;
  const uint32_t* adj;
  uint64_t nnz;
  uint32_t M;
};

// What shrink_import leaves for shrink_finish, all of it owned by the caller's Scaffold.
struct ShrinkTables {
  std::vector<RemoveLayer> ly;  // per layer: old CSR and table
  uint32_t* d_deg = nullptr;    // [layers][n0] the tables' degrees: one block, read back in one copy
  uint32_t* d_flag = nullptr;   // [0] what the import could not take (Scaffold::csr_to_table's bits), [1] compaction,
                                // [2 ..] the touched pairs: all, then per layer
};

// What shrink_finish returns.
struct Shrunk {
  std::vector<const uint64_t*> off;  // per kept layer, the survivors' CSR over the new ids: layer 0 from the
  std::vector<const uint32_t*> adj;  // Scaffold's tmp; the layers above from keep, one block of offsets over ALL new
                                     // ids (a node below a layer has an empty row there) and one of ids
  isl::RowTable rows;                // the survivors' rows and norms, bit for bit, in the stored type
  isl_plan::Entry entry;             // remove_plan.hpp's entry rule
  std::vector<uint64_t> levels;      // of the survivors
  // for the caller's ISL_DEBUG line
  std::vector<uint32_t> counts;      // [1 + layers] touched (layer, node) pairs: all, then per layer
  unsigned long long candidates = 0; // sum of |C(p)| over them
  float repair_ms = 0.0f;            // the repair kernel, timed under ISL_DEBUG alone
};

// The removal in two halves, so that each caller words its own refusals in between.
// shrink_import: every layer's list returns to a table of n0 rows in its stored order (an untouched row is finished
// with that copy), all launches enqueued; the caller reads t.d_flag[0] once and refuses what it must.
isl_status shrink_import(Scaffold& c, const std::vector<ShrinkLayer>& layers, uint64_t n0, ShrinkTables& t);
// shrink_finish, once the CSRs are known to be in range: one kernel lists the (layer, node) pairs that lost a
// neighbour, one repair launch rebuilds those rows from the layer's OLD CSR under M_L, one launch compacts the kept
// layers through the remap and one gathers the survivors' rows.  Two read-backs in between: the pair counts and the
// repaired degrees.  `old_rows`: resident f32 or bf16 rows of all n0 nodes; `remap` / `survivors`:
// isl_plan::build_remap's, at least one survivor.  The levels play two roles.  `levels` (of all old nodes, or empty
// = all 0) and has_entry / entry / max_level always feed the entry rule.  With `levels_name_layers` they also say
// which node has which layer (a node has layer L iff levels[node] >= L): the kernels then read them from a device
// copy, and the layers above the new max_level cease to exist.  Without it the kernels get no level array: every
// node has every layer and every layer is kept -- a flat index, whose levels only name the entry point.
// `call` names the entry point in messages.  Without `gather_rows` out.rows stays empty: the caller compacts the
// old table in place once everything else stands (isl_index_remove on a reserved index).
isl_status shrink_finish(Scaffold& c, ShrinkTables& t, const isl::RowTable& old_rows, uint32_t metric,
                         const isl_build_options& opts, const std::vector<uint32_t>& remap,
                         const std::vector<uint32_t>& survivors, const std::vector<uint64_t>& levels, bool has_entry,
                         uint64_t entry, uint64_t max_level, bool levels_name_layers, const char* call, Shrunk& out,
                         bool gather_rows = true);

}  // namespace isl_build
