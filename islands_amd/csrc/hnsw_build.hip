// HnswGraph::insert on the device (src/core/hnsw.rs:214-329): the descent kernel, its gather, isl_hnsw_build (a
// whole collection) and isl_hnsw_insert (more rows into an existing graph) -- one loop, grow(), entered at node 0
// or at the graph's len.  (What reads a finished graph back -- levels, lists, rows, to_bytes -- is hnsw.hip's.)
//
// The graph under construction is one fixed-width table per layer ([n][M_L + 1] ids + a degree array;
// M_L = m0 on layer 0, m above), the layout the search kernels already read during LeannIndex::build.  A
// node that lacks a layer has degree 0 there, which is exactly what neighbors_at(layer) == None means to
// the descent and to search_layer (hnsw.rs:363-364).  Nodes are inserted in id order, `batch` per step:
//   1. insert_descent_kernel: every node of the step walks from the entry point down to its level + 1
//      (hnsw.rs:263-282) on the graph as of the step's start and leaves its `current`;
//   2. per layer, from the step's highest level down to 0, the nodes that have the layer run the
//      construction search (the search path itself: isl::search_device_sync over the layer's table with
//      per-query entry nodes, HnswGraph heap order, equal distances decided by the heap-exact kernel),
//      the selection (build.hip: truncation or select()) and link_kernel's HNSW mode -- Scaffold::insert of
//      build_internal.hpp, the call LeannIndex::build makes once per step on its one table.
// The steps follow from `levels` alone (a node above the current top layer is alone in its step), so the
// whole plan is laid out once (plan_steps, build_plan.hpp): the nodes of a step sorted by level, highest first
// -- the nodes that have layer L are then a prefix of the step.
// With batch = 1 and ISL_SELECT_REFERENCE this is the reference's construction, list by list.
// Rows are f32 or bf16 bit patterns (isl_hnsw_build_rows / isl_hnsw_insert_rows): bf16 rows stay bf16 in the
// construction graph and in the finished one, every kernel that measures takes the row type as a template parameter
// and works on the exact f32 images, so the graph is the one built from the widened rows.
// A graph that grows returns to this layout first: its CSR layers are written back into tables of len + n_new
// rows (Scaffold::csr_to_table), its rows are copied beside the new ones, and the plan starts at node len.  The
// grown graph is built beside the old one and swapped into the handle at the end.
// A graph that shrinks (isl_hnsw_remove, shrink()) hands its layers to the removal routine of build.hip
// (isl_build::shrink_import / shrink_finish, the one isl_index_remove calls with its single layer), which repairs
// and compacts every layer in one pass; the shrunk graph is swapped in as a grown one is (install_core).  The
// host-only arithmetic is hnsw_remove_plan.hpp's.
#include "device_common.hip.h"
#include "build_internal.hpp"
#include "hnsw_remove_plan.hpp"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

namespace {

using namespace isl_dev;
using isl_build::BuildParams;

struct DescentParams {
  const void* emb;     // rows of the stored type: f32, or bf16 bit patterns (ROWT of the kernel)
  const float* norm2;  // of the (widened) rows
  uint64_t stride;     // in elements of that type
  uint32_t d;
  const uint32_t* const* tab;  // [top + 1] device pointers: layer tables (index 0 unused here)
  const uint32_t* const* deg;  // [top + 1] their degree arrays
  uint32_t W;                  // row pitch of the layers above 0: m + 1
  const uint32_t* node_ids;    // [B] the step's nodes
  const uint32_t* levels;      // [n]
  uint32_t B;
  uint32_t entry, max_level;   // as of the step's start
  uint32_t* cur_of;            // [n] out: `current` at layer level + 1 (the entry point if nothing is above)
  uint32_t* evals_of;          // [n] out: distance evaluations of the descent (+ 1 for the entry point)
};

// hnsw.rs:254-282 for one new node per wave: current = entry point, then per layer max_level .. level + 1
// rounds in which the list of the node the round STARTED at is scanned in order and `current` moves to
// every strictly closer id, until a round changes nothing.
// ROWT = uint16_t: bf16 rows.  The node's own row is widened exactly into the query area (no tile in front of it;
// norm_a is the row's norm2, the bits the d-step sum over the widened values gives) and the neighbours are measured
// with the tile-free routine: the f32 chain over the exact images.
template <int METRIC_API, typename ROWT = float>
__global__ __launch_bounds__(64) void insert_descent_kernel(DescentParams p) {
  constexpr int METRIC = METRIC_API == ISL_METRIC_COSINE ? METRIC_COSINE_PRE : METRIC_API;
  constexpr bool BF16 = sizeof(ROWT) == 2;
  extern __shared__ __align__(16) unsigned char smem[];
  float* tile = reinterpret_cast<float*>(smem);
  float* qs = tile + (BF16 ? 0 : TILE_ROWS * TILE_LD);
  const ROWT* emb = static_cast<const ROWT*>(p.emb);
  const uint32_t lane = threadIdx.x, b = blockIdx.x;
  if (b >= p.B) return;
  const uint32_t node = p.node_ids[b];
  const uint32_t level = p.levels[node];
  float q_norm;
  if constexpr (BF16) {
    widen_row_query(emb + (uint64_t)node * p.stride, p.d, qs);
    q_norm = METRIC == METRIC_COSINE_PRE ? p.norm2[node] : 0.0f;
  } else {
    q_norm = load_query<METRIC>(emb + (uint64_t)node * p.stride, p.d, qs);
  }
  uint32_t cur = p.entry, cV = 1;
  const float e_aux = METRIC == METRIC_COSINE_PRE ? p.norm2[cur] : 0.0f;
  float cd;
  if constexpr (BF16) cd = rl_f(direct_distances<METRIC, uint16_t>(emb, p.stride, p.d, cur, 1, qs, q_norm, e_aux), 0);
  else cd = rl_f(wave_distances<METRIC>(emb, p.stride, p.d, cur, 1, qs, tile, q_norm, e_aux), 0);
  for (uint32_t layer = p.max_level; layer > level; --layer) {
    const uint32_t* tab = p.tab[layer];
    const uint32_t* deg = p.deg[layer];
    for (;;) {
      const uint32_t* row = tab + (uint64_t)cur * p.W;
      const uint32_t dg = deg[cur] < p.W ? deg[cur] : p.W;
      bool changed = false;
      uint32_t nxt = cur;
      float nd = cd;
      for (uint32_t base = 0; base < dg; base += 64) {
        const uint32_t R = dg - base < 64u ? dg - base : 64u;
        const uint32_t gid = lane < R ? row[base + lane] : cur;
        const float aux = (METRIC == METRIC_COSINE_PRE && lane < R) ? p.norm2[gid] : 0.0f;
        float gd;  // lane j < R: d(node, row gid(j)), by the routine that reads the stored type
        if constexpr (BF16) gd = direct_distances<METRIC, uint16_t>(emb, p.stride, p.d, gid, R, qs, q_norm, aux);
        else gd = wave_distances<METRIC>(emb, p.stride, p.d, gid, R, qs, tile, q_norm, aux);
        cV += R;
        for (uint32_t r = 0; r < R; ++r) {  // list order, strict `<` (hnsw.rs:271)
          const float dr = rl_f(gd, (int)r);
          if (dr < nd) { nxt = rl_u(gid, (int)r); nd = dr; changed = true; }
        }
      }
      cur = nxt;
      cd = nd;
      if (!changed) break;
    }
  }
  if (lane == 0) {
    p.cur_of[node] = cur;
    p.evals_of[node] = cV;
  }
}

// The queries of one layer's construction search: the rows of the step's first `cnt` nodes, and where each
// starts.
__global__ void gather_layer_kernel(const float* __restrict__ emb, uint64_t stride, uint32_t d,
                                    const uint32_t* __restrict__ node_ids, uint32_t cnt,
                                    const uint32_t* __restrict__ cur_of, const uint32_t* __restrict__ evals_of,
                                    float* __restrict__ q, uint32_t* __restrict__ q_entry,
                                    uint32_t* __restrict__ q_evals) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cnt) {
    q_entry[i] = cur_of[node_ids[i]];
    q_evals[i] = evals_of[node_ids[i]];
  }
  if (i >= (uint64_t)cnt * d) return;
  q[i] = emb[(uint64_t)node_ids[i / d] * stride + i % d];
}

}  // namespace

extern "C" {

void isl_hnsw_config_default(isl_hnsw_config* c) {  // hnsw.rs:37-48
  if (!c) return;
  c->m = 16;
  c->m0 = 32;
  c->ef_construction = 200;
  c->ml = 1.0 / std::log(16.0);
  c->metric = ISL_METRIC_COSINE;
  c->max_layers = 16;
}

}  // extern "C"

namespace {

// out[i] = the level of position first + i of the `seed` stream (isl_hnsw_random_levels is first = 0)
isl_status random_levels_at(uint64_t seed, uint64_t first, uint64_t n, double ml, uint64_t max_layers, uint64_t* out) {
  if (!out && n) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  if (max_layers == 0 || !std::isfinite(ml) || ml < 0.0)
    return isl::fail(ISL_ERR_INVALID_ARGUMENT, "isl_hnsw_random_levels: max_layers >= 1 and a finite ml >= 0");
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t z = seed + (first + i + 1) * 0x9E3779B97F4A7C15ull;  // splitmix64
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const double r = ((double)(z >> 11) + 0.5) * (1.0 / 9007199254740992.0);  // in (0, 1)
    const double lv = std::floor(-std::log(r) * ml);                          // hnsw.rs:209
    out[i] = lv >= (double)(max_layers - 1) ? max_layers - 1 : (uint64_t)lv;
  }
  return ISL_OK;
}

// The levels of all n nodes of the graph a call leaves behind: those of `old` (NULL: an empty graph), then
// the new nodes' -- as handed in, or positions n0 .. n-1 of the seed's stream -- with `top`, the highest layer
// of that graph, and the checks that need nothing but them.  (isl_hnsw_insert refuses a handle whose levels do
// not match its layers, such as one made without levels that has layers above 0.)
isl_status all_levels(const isl_index* old, const isl_hnsw_config& cfg, uint64_t n, const uint64_t* levels_in,
                      uint64_t level_seed, std::vector<uint64_t>& lv, uint64_t& top) {
  using isl::fail;
  const uint64_t n0 = old ? old->num_nodes : 0;
  lv.assign(n, 0);
  for (uint64_t i = 0; i < n0 && i < old->levels.size(); ++i) lv[i] = old->levels[i];
  if (levels_in) std::copy(levels_in, levels_in + (n - n0), lv.begin() + n0);
  else ISL_TRY(random_levels_at(level_seed, n0, n - n0, cfg.ml, cfg.max_layers, lv.data() + n0));
  top = old ? old->max_level : 0;  // what the old nodes reach: checked when the handle was made
  for (uint64_t i = n0; i < n; ++i) {
    if (lv[i] >= cfg.max_layers)
      return fail(ISL_ERR_INVALID_ARGUMENT, "levels[%llu] = %llu is not below max_layers = %llu",
                  (unsigned long long)(i - n0), (unsigned long long)lv[i], (unsigned long long)cfg.max_layers);
    top = std::max(top, lv[i]);
  }
  if (const char* why = isl_plan::shape_limit(cfg.m0, cfg.ef_construction, n)) return fail(ISL_ERR_UNSUPPORTED, "%s", why);
  if (top >= 64) return fail(ISL_ERR_UNSUPPORTED, "the device builder keeps up to 64 layers");
  return ISL_OK;
}

// What `call` (isl_hnsw_insert, isl_hnsw_remove) refuses once the layers of `from` have returned to their tables:
// *d_flag holds Scaffold::csr_to_table's bits over all layers, read here once.  Past this the CSRs are in range.
// (isl_hnsw_insert has refused a layer 0 that is not verbatim before it came here.)
isl_status check_import(const char* call, const uint32_t* d_flag, const isl_hnsw* from) {
  using isl::fail;
  uint32_t flag = 0;
  if (hipMemcpy(&flag, d_flag, 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(ISL_ERR_DEVICE, "importing the graph's layers failed");
  if (flag & 1u)
    return fail(ISL_ERR_UNSUPPORTED, "%s: the graph has a list longer than its layer keeps (m0 = %u on layer 0, m = %u "
                "above)", call, (uint32_t)from->m0, (uint32_t)from->m);
  if (isl_build::device_lists_differ(from->core))
    return fail(ISL_ERR_UNSUPPORTED, "%s: the device copy of layer 0 is not the lists verbatim (ids repeated inside a "
                "list were removed at upload)", call);
  if (flag) return fail(ISL_ERR_UNSUPPORTED, "%s: the graph's layers name ids or offsets outside it", call);
  return ISL_OK;
}

// HnswGraph::insert for nodes n0 .. n-1 of a graph that holds n0 (`from`: a finished graph with at least one
// node, whose CSR layers return to the builder's tables; NULL: nothing, node 0 starts the graph).  One loop
// over the plan's steps -- descent, per-layer gather, Scaffold::insert -- then compaction and
// attach_upper_layers.  `from` is only read; the graph of all n nodes leaves in `out`, built beside it.
// `vectors`: the n_new rows, of `dtype` (f32 or bf16 bit patterns; the stored type of `from` where there is one), which
// the grown graph keeps as they are.
isl_status grow(const isl_hnsw_config& cfg, const isl_build_options& opts, const isl_hnsw* from, const void* vectors,
                int32_t dtype, uint64_t n_new, uint64_t d, const std::vector<uint64_t>& levels, uint64_t top,
                int32_t mem, int32_t device, std::unique_ptr<isl_hnsw>& out) {
  using isl::fail;
  const isl_index* old = from ? from->core : nullptr;
  const uint64_t n0 = old ? old->num_nodes : 0, n = n0 + n_new;
  ISL_TRY(isl::use_device(device));

  const std::vector<uint32_t> lv(levels.begin(), levels.end());  // what the planner and the kernels read
  std::vector<isl_plan::Step> steps;
  std::vector<uint32_t> order;
  isl_plan::plan_steps_from(lv, n0, old ? (uint32_t)old->max_level : 0u, opts.batch ? opts.batch : 1, steps, order);
  const uint64_t B = isl_plan::largest_step(steps);

  const uint32_t m = (uint32_t)cfg.m, m0 = (uint32_t)cfg.m0, ef = (uint32_t)cfg.ef_construction;
  const uint64_t layers = top + 1;
  isl_leann_config lcfg;
  isl_leann_config_paper_default(&lcfg);
  lcfg.metric = cfg.metric;
  lcfg.prune_ratio = 0.0f;
  isl_build::Scaffold c;
  ISL_TRY(c.open(lcfg, opts, true, vectors, dtype, n, d, mem, device, B, m0, ef, old));
  isl_index* g = c.g;

  // one table per layer, and what the descent and the per-layer gathers read
  std::vector<isl_build::Table> tab(layers);
  std::vector<uint32_t*> h_ell(layers), h_deg(layers);
  for (uint64_t L = 0; L < layers; ++L) {
    tab[L].M = L ? m : m0;
    ISL_TRY(c.alloc(&tab[L].ell, n * (tab[L].M + 1)));
    ISL_TRY(c.alloc(&tab[L].deg, n, true));
    h_ell[L] = tab[L].ell;
    h_deg[L] = tab[L].deg;
  }
  if (old) {
    // the finished layers return to the tables: layer 0 from the core index's CSR, the layers above from the
    // descent's arrays.  Rows n0 .. n-1, nodes that lack a layer and layers the old graph did not have keep
    // degree 0.
    uint32_t* d_flag = nullptr;
    ISL_TRY(c.alloc(&d_flag, 1, true));
    ISL_TRY(c.csr_to_table(tab[0], old->d_off, old->d_adj, old->nnz, n0, d_flag));
    for (uint64_t L = 1; L <= old->max_level && L < from->layer_off.size(); ++L) {
      uint64_t nnz = 0;
      if (hipMemcpy(&nnz, from->layer_off[L] + n0, 8, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(ISL_ERR_DEVICE, "cannot read the offsets of layer %llu", (unsigned long long)L);
      ISL_TRY(c.csr_to_table(tab[L], from->layer_off[L], from->layer_adj[L], nnz, n0, d_flag));
    }
    ISL_TRY(check_import("isl_hnsw_insert", d_flag, from));
  }
  uint32_t **d_tab = nullptr, **d_deg = nullptr;
  uint32_t *d_lv = nullptr, *d_order = nullptr, *cur_of = nullptr, *evals_of = nullptr;
  ISL_TRY(c.alloc(&d_tab, layers));
  ISL_TRY(c.alloc(&d_deg, layers));
  ISL_TRY(c.alloc(&d_lv, n));
  ISL_TRY(c.alloc(&d_order, n));
  ISL_TRY(c.alloc(&cur_of, n, true));
  ISL_TRY(c.alloc(&evals_of, n, true));
  ISL_TRY(c.alloc(&g->build_q_entry, B * 2));
  g->build_q_evals = g->build_q_entry + B;
  if (hipMemcpy(d_lv, lv.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_order, order.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_tab, h_ell.data(), layers * sizeof(void*), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_deg, h_deg.data(), layers * sizeof(void*), hipMemcpyHostToDevice) != hipSuccess)
    return fail(ISL_ERR_DEVICE, "cannot stage the build plan");

  DescentParams dp{};
  dp.emb = g->rows.data(); dp.norm2 = g->rows.norm2(); dp.stride = g->rows.stride(); dp.d = (uint32_t)d;
  dp.tab = d_tab; dp.deg = d_deg; dp.W = m + 1; dp.levels = d_lv;
  dp.cur_of = cur_of; dp.evals_of = evals_of;
  c.p.node_levels = d_lv;
  c.p.cur_of = cur_of;

  // the graph as the first step finds it: the old one's entry point and top layer, or node 0 alone -- entry
  // point, max_level = its level, every list empty (hnsw.rs:240-245)
  uint64_t entry = old ? old->entry_point : 0, max_level = old ? old->max_level : lv[0];
  const bool bf16 = g->rows.is_bf16();
  // (the descent over bf16 rows holds the widened query alone: what the bf16 link kernel holds)
  const size_t descent_lds = bf16 ? isl_plan::link_lds_bf16((uint32_t)d) : isl_build::link_lds(d);
  for (const isl_plan::Step& s : steps) {
    const uint32_t* ids = d_order + s.first;
    dp.node_ids = ids; dp.B = s.count; dp.entry = (uint32_t)entry; dp.max_level = (uint32_t)max_level;
    isl::by_metric(cfg.metric, [&](auto mc) {
      if (bf16)
        hipLaunchKernelGGL((insert_descent_kernel<decltype(mc)::value, uint16_t>), dim3(s.count), dim3(64), descent_lds, 0, dp);
      else
        hipLaunchKernelGGL(insert_descent_kernel<decltype(mc)::value>, dim3(s.count), dim3(64), descent_lds, 0, dp);
    });
    if (hipGetLastError() != hipSuccess) return fail(ISL_ERR_DEVICE, "descent launch failed");
    g->has_entry = true;
    g->entry_point = entry;
    uint32_t cnt = 0;  // nodes of the step that have the layer: a prefix, growing as the layer falls
    for (uint64_t L = s.top + 1; L-- > 0;) {
      while (cnt < s.count && lv[order[s.first + cnt]] >= L) ++cnt;
      if (bf16)  // the widened rows, through the flat builder's gather
        c.gather_bf16(0, cnt, ids, cur_of, evals_of);
      else
        hipLaunchKernelGGL(gather_layer_kernel, dim3((uint32_t)(((uint64_t)cnt * d + 255) / 256)), dim3(256), 0, 0,
                           g->rows.f32(), g->rows.stride(), (uint32_t)d, ids, cnt, cur_of, evals_of, c.qbuf,
                           g->build_q_entry, g->build_q_evals);
      if (hipGetLastError() != hipSuccess) return fail(ISL_ERR_DEVICE, "gather launch failed");
      ISL_TRY(c.insert(tab[L], cnt, s.count > 1, 0, ids, (uint32_t)L));
    }
    if (hipDeviceSynchronize() != hipSuccess) return fail(ISL_ERR_DEVICE, "builder kernels failed");
    if (s.top > max_level) {  // hnsw.rs:322-325 (such a node is alone in its step)
      max_level = s.top;
      entry = order[s.first];
    }
  }

  // per-layer table -> CSR; layer 0 becomes the core index (its own copy), the layers above are kept as the
  // descent's arrays: the pointer tables carry nothing for layer 0
  std::vector<const uint64_t*> offs(max_level + 1, nullptr);
  std::vector<const uint32_t*> adjs(max_level + 1, nullptr);
  for (uint64_t L = 0; L <= max_level; ++L) {
    uint64_t* d_off = nullptr;
    uint32_t* d_adj = nullptr;
    ISL_TRY(c.table_to_csr(tab[L], n, L > 0, &d_off, &d_adj));
    if (L) { offs[L] = d_off; adjs[L] = d_adj; continue; }
    ISL_TRY(isl_index_from_device_csr(&lcfg, device, n, d_off, d_adj, 1, entry, 1, d, &c.res));
  }
  c.res->is_hnsw = true;
  c.res->max_level = max_level;
  c.res->levels = levels;
  std::unique_ptr<isl_hnsw> h(new isl_hnsw());
  h->core = c.res;
  h->m = cfg.m; h->m0 = cfg.m0; h->ef_construction = cfg.ef_construction; h->dim = d;
  h->ml = cfg.ml; h->max_layers = cfg.max_layers;
  h->device = device;
  ISL_TRY(isl::attach_upper_layers(h.get(), offs, adjs));
  c.release();
  out = std::move(h);
  return ISL_OK;
}

// What isl_hnsw_insert and isl_hnsw_remove ask of a non-empty handle before they read its layers.  The kernels
// take "has the layer" from the levels: a handle made without them (all 0) or with levels that do not reach its
// top layer would quietly turn into another graph.
isl_status check_entry_and_levels(const char* call, const isl_index* core) {
  using isl::fail;
  const uint64_t n0 = core->num_nodes;
  if (!core->has_entry) return fail(ISL_ERR_UNSUPPORTED, "%s: the graph has nodes and no entry point", call);
  if (core->levels.size() != n0 || core->entry_point >= n0 || core->levels[core->entry_point] != core->max_level ||
      *std::max_element(core->levels.begin(), core->levels.end()) != core->max_level)
    return fail(ISL_ERR_UNSUPPORTED, "%s: the nodes' levels do not match the graph's layers (max_level "
                "%llu; the entry point's level must equal it and no level may exceed it) -- was the handle made "
                "without levels?", call, (unsigned long long)core->max_level);
  return ISL_OK;
}

// The graph of `from` without the nodes `remap` marks kGone (include/islands_amd.h, isl_hnsw_remove), every layer
// in one pass of the removal routine (isl_build::shrink_import / shrink_finish): layer 0 is the core index's CSR,
// the layers above are the descent's arrays, and the levels say which node has which layer.  `from` (non-empty,
// resident f32 or bf16 rows, levels that match its layers, at least one survivor) is only read; the shrunk graph leaves in
// `out`, built beside it.
isl_status shrink(const isl_build_options& opts, const isl_hnsw* from, const std::vector<uint32_t>& remap,
                  const std::vector<uint32_t>& survivors, std::unique_ptr<isl_hnsw>& out) {
  using isl::fail;
  const isl_index* old = from->core;
  const uint64_t n0 = old->num_nodes, n = survivors.size(), layers = old->max_level + 1;
  const uint32_t m = (uint32_t)from->m, m0 = (uint32_t)from->m0;
  if (from->layer_off.size() < layers || from->layer_adj.size() < layers)
    return fail(ISL_ERR_UNSUPPORTED, "isl_hnsw_remove: the graph holds %llu layers and max_level is %llu",
                (unsigned long long)from->layer_off.size(), (unsigned long long)old->max_level);
  ISL_TRY(isl::use_device(old->device));
  std::vector<isl_build::ShrinkLayer> ly(layers);
  ly[0] = {old->d_off.get(), old->d_adj.get(), old->nnz, m0};
  for (uint64_t L = 1; L < layers; ++L) {
    ly[L] = {from->layer_off[L], from->layer_adj[L], 0, isl_plan::layer_cap((uint32_t)L, m, m0)};
    if (!ly[L].off || !ly[L].adj) return fail(ISL_ERR_UNSUPPORTED, "isl_hnsw_remove: layer %llu is not on the device",
                                               (unsigned long long)L);
    if (hipMemcpy(&ly[L].nnz, ly[L].off + n0, 8, hipMemcpyDeviceToHost) != hipSuccess)
      return fail(ISL_ERR_DEVICE, "cannot read the offsets of layer %llu", (unsigned long long)L);
  }
  isl_build::Scaffold c;  // the staging buffers alone: no construction graph
  isl_build::ShrinkTables t;
  ISL_TRY(isl_build::shrink_import(c, ly, n0, t));
  ISL_TRY(check_import("isl_hnsw_remove", t.d_flag, from));
  isl_build::Shrunk r;
  ISL_TRY(isl_build::shrink_finish(c, t, old->rows, old->cfg.metric, opts, remap, survivors, old->levels, old->has_entry,
                                   old->entry_point, old->max_level, true, "isl_hnsw_remove", r));
  if (getenv("ISL_DEBUG")) {
    std::string per;
    for (uint64_t L = 0; L < layers; ++L) per += (L ? " " : "") + std::to_string(r.counts[1 + L]);
    fprintf(stderr, "[isl] isl_hnsw_remove: %llu of %llu nodes removed, layers %llu -> %llu, touched %u (per layer: %s), "
            "candidates %llu, repair kernel %.3f ms\n", (unsigned long long)(n0 - n), (unsigned long long)n0,
            (unsigned long long)layers, (unsigned long long)r.off.size(), r.counts[0], per.c_str(), r.candidates,
            r.repair_ms);
  }
  // layer 0 becomes the new core as grow() makes it (its own copy); the layers above are attached as the builder's
  // are: the pointer tables carry nothing for layer 0
  const isl_leann_config lcfg = old->cfg;
  ISL_TRY(isl_index_from_device_csr(&lcfg, old->device, n, r.off[0], r.adj[0], r.entry.has ? 1 : 0, r.entry.id, 1,
                                    old->rows.d(), &c.res));
  r.off[0] = nullptr;
  r.adj[0] = nullptr;
  c.res->is_hnsw = true;
  c.res->max_level = r.entry.max_level;
  c.res->levels = std::move(r.levels);
  c.res->rows = std::move(r.rows);
  c.res->nvec = n;
  std::unique_ptr<isl_hnsw> h(new isl_hnsw());
  h->core = c.res;
  h->m = from->m; h->m0 = from->m0; h->ef_construction = from->ef_construction; h->dim = from->dim;
  h->ml = from->ml; h->max_layers = from->max_layers;
  h->device = old->device;
  ISL_TRY(isl::attach_upper_layers(h.get(), r.off, r.adj));
  for (auto& b : c.keep) c.res->hnsw_owned.push_back(std::move(b));
  c.keep.clear();
  c.res = nullptr;
  out = std::move(h);
  return ISL_OK;
}

// What isl_hnsw_insert and isl_hnsw_remove do to the handle once the new graph stands beside the old one, which
// nothing has touched so far: the core and the layer tables are swapped, the host mirrors reset and the old core
// freed.  `verb` words the refusal beside a search ("grow", "shrink"), which frees the new core instead.  Either way
// `fresh` is left for its owner to delete, without a core of its own.
isl_status install_core(isl_hnsw* h, isl_hnsw* fresh, uint64_t dim, int32_t device, const char* verb) {
  std::lock_guard<std::mutex> host_lock(h->host_mu);
  isl_index* old = h->core;
  {
    std::lock_guard<std::mutex> lock(old->mu);
    if (isl::any_lane_busy(old)) {
      isl_index_free(fresh->core);
      return isl::fail(ISL_ERR_SEARCH, "Search error: the graph cannot %s while searches are in flight", verb);
    }
  }
  h->core = fresh->core;
  h->layer_off.swap(fresh->layer_off);
  h->layer_adj.swap(fresh->layer_adj);
  h->dim = dim;
  h->device = device;
  h->host_valid = false;
  h->h_off.clear();
  h->h_adj.clear();
  isl_index_free(old);  // with its lanes and padded adjacency; the new core sets its own up at the first search
  return ISL_OK;
}

}  // namespace

extern "C" {

isl_status isl_hnsw_random_levels(uint64_t seed, uint64_t n, double ml, uint64_t max_layers, uint64_t* out) {
  return random_levels_at(seed, 0, n, ml, max_layers, out);
}

isl_status isl_hnsw_build(const isl_hnsw_config* cfg_in, const isl_build_options* opts_in, const float* vectors,
                          uint64_t n, uint64_t d, const uint64_t* levels_in, uint64_t level_seed, int32_t mem,
                          int32_t device, isl_hnsw** out) {
  return isl_hnsw_build_rows(cfg_in, opts_in, vectors, ISL_DTYPE_F32, n, d, levels_in, level_seed, mem, device, out);
}

isl_status isl_hnsw_build_rows(const isl_hnsw_config* cfg_in, const isl_build_options* opts_in, const void* vectors,
                               int32_t dtype, uint64_t n, uint64_t d, const uint64_t* levels_in, uint64_t level_seed,
                               int32_t mem, int32_t device, isl_hnsw** out) {
  using isl::fail;
  if (!out || (!vectors && n)) return fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  isl_build_options opts;
  ISL_TRY(isl_build::resolve_build_options(opts_in, true, opts));
  ISL_TRY(isl::hnsw_row_dtype(dtype));
  isl_hnsw_config cfg;
  if (cfg_in) cfg = *cfg_in;
  else isl_hnsw_config_default(&cfg);
  ISL_TRY(isl::hnsw_config_validate(cfg.m, cfg.m0, cfg.ef_construction, cfg.metric));
  if (n == 0) {  // HnswGraph::new: no nodes, no entry point, no dimension
    ISL_TRY(isl_hnsw_from_layers(cfg.m, cfg.m0, cfg.ef_construction, (int32_t)cfg.metric, 0, 0, 0, nullptr, nullptr,
                                 nullptr, 0, 0, 0, nullptr, device, out));
    (*out)->ml = cfg.ml;
    (*out)->max_layers = cfg.max_layers;
    return ISL_OK;
  }
  if (d == 0) return fail(ISL_ERR_EMPTY_COLLECTION, "Empty vector collection");
  std::vector<uint64_t> levels;
  uint64_t top = 0;
  ISL_TRY(all_levels(nullptr, cfg, n, levels_in, level_seed, levels, top));
  std::unique_ptr<isl_hnsw> h;
  ISL_TRY(grow(cfg, opts, nullptr, vectors, dtype, n, d, levels, top, mem, device, h));  // insert into nothing
  *out = h.release();
  return ISL_OK;
}

isl_status isl_hnsw_insert(isl_hnsw* h, const isl_build_options* opts_in, const float* vectors, uint64_t n_new,
                           uint64_t d, const uint64_t* levels_in, uint64_t level_seed, int32_t mem,
                           uint64_t* first_id) {
  return isl_hnsw_insert_rows(h, opts_in, vectors, ISL_DTYPE_F32, n_new, d, levels_in, level_seed, mem, first_id);
}

isl_status isl_hnsw_insert_rows(isl_hnsw* h, const isl_build_options* opts_in, const void* vectors, int32_t dtype,
                                uint64_t n_new, uint64_t d, const uint64_t* levels_in, uint64_t level_seed,
                                int32_t mem, uint64_t* first_id) {
  using isl::fail;
  if (!h || !h->core || (!vectors && n_new)) return fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  isl_build_options opts;
  ISL_TRY(isl_build::resolve_build_options(opts_in, true, opts));
  ISL_TRY(isl::hnsw_row_dtype(dtype));
  const isl_index* core = h->core;
  const uint64_t n0 = core->num_nodes;
  if (n_new == 0) {
    if (first_id) *first_id = n0;
    return ISL_OK;
  }
  if (n0 && d != h->dim) return isl::fail_dim(h->dim, d);  // hnsw.rs:216-222
  if (d == 0) return fail(ISL_ERR_EMPTY_COLLECTION, "Empty vector collection");
  isl_hnsw_config cfg;
  cfg.m = h->m; cfg.m0 = h->m0; cfg.ef_construction = h->ef_construction;
  cfg.ml = h->ml; cfg.metric = core->cfg.metric; cfg.max_layers = h->max_layers;
  std::vector<uint64_t> levels;
  uint64_t top = 0;
  ISL_TRY(all_levels(n0 ? core : nullptr, cfg, n0 + n_new, levels_in, level_seed, levels, top));
  if (n0) {
    if (core->recompute || !(core->rows.f32() || core->rows.bf16()) || !core->rows.norm2() || core->nvec != n0 ||
        core->rows.d() != d || core->device < 0)
      return fail(ISL_ERR_UNSUPPORTED, "isl_hnsw_insert needs the graph's float32 or bf16 rows resident on the device");
    if (core->rows.dtype() != dtype)  // isl_index_insert's rule
      return fail(ISL_ERR_UNSUPPORTED, "isl_hnsw_insert: the graph stores %s rows and takes no other type",
                  core->rows.is_bf16() ? "bf16" : "float32");
    ISL_TRY(check_entry_and_levels("isl_hnsw_insert", core));
    if (core->max_degree > h->m0)
      return fail(ISL_ERR_UNSUPPORTED, "isl_hnsw_insert: a layer-0 list of %u ids is longer than m0 = %llu",
                  core->max_degree, (unsigned long long)h->m0);
    if (isl_build::device_lists_differ(core))
      return fail(ISL_ERR_UNSUPPORTED,
                  "isl_hnsw_insert: the device copy of layer 0 is not the lists verbatim (ids repeated inside a list "
                  "were removed at upload)");
  }
  {  // the &mut self of the reference: not beside a search on the same handle
    std::lock_guard<std::mutex> lock(core->mu);
    if (isl::any_lane_busy(core))
      return fail(ISL_ERR_SEARCH, "Search error: the graph cannot grow while searches are in flight");
  }
  std::unique_ptr<isl_hnsw> grown;
  ISL_TRY(grow(cfg, opts, n0 ? h : nullptr, vectors, dtype, n_new, d, levels, top, mem, n0 ? core->device : h->device,
               grown));
  ISL_TRY(install_core(h, grown.get(), d, grown->core->device, "grow"));
  if (first_id) *first_id = n0;
  return ISL_OK;
}

isl_status isl_hnsw_remove(isl_hnsw* h, const isl_build_options* opts_in, const uint64_t* ids, uint64_t n_ids,
                           uint64_t* out_remap, uint64_t* out_len) {
  using isl::fail;
  if (!h || !h->core || (!ids && n_ids)) return fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  isl_build_options opts;
  ISL_TRY(isl_build::resolve_build_options(opts_in, true, opts));
  const isl_index* core = h->core;
  const uint64_t n0 = core->num_nodes;
  if (n_ids == 0) {
    isl_build::write_remap(nullptr, n0, out_remap);
    if (out_len) *out_len = n0;
    return ISL_OK;
  }
  uint64_t bad = 0;
  if (isl_plan::first_unknown_id(ids, n_ids, n0, &bad)) return isl::fail_node(bad);
  // (an id below len exists: the graph is not empty)
  if (core->recompute || !(core->rows.f32() || core->rows.bf16()) || !core->rows.norm2() || core->rows.n() != n0 ||
      core->nvec != n0 || core->device < 0 || !core->d_off)
    return fail(ISL_ERR_UNSUPPORTED, "isl_hnsw_remove needs the graph's float32 or bf16 rows resident on the device");
  ISL_TRY(check_entry_and_levels("isl_hnsw_remove", core));
  if (h->m0 > isl_plan::kMaxM0 || h->m > isl_plan::kMaxM0)
    return fail(ISL_ERR_UNSUPPORTED, "%s", isl_plan::shape_limit(isl_plan::kMaxM0 + 1, 0, 0));
  if (core->max_level >= isl_plan::kMaxLayers) return fail(ISL_ERR_UNSUPPORTED, "the device builder keeps up to 64 layers");
  {  // the &mut self of the reference: not beside a search on the same handle
    std::lock_guard<std::mutex> lock(core->mu);
    if (isl::any_lane_busy(core))
      return fail(ISL_ERR_SEARCH, "Search error: the graph cannot shrink while searches are in flight");
  }
  std::vector<uint32_t> remap, survivors;
  const uint64_t n = isl_plan::build_remap(n0, ids, n_ids, remap, survivors);
  std::unique_ptr<isl_hnsw> shrunk;
  if (n == 0) {  // every node gone: what isl_hnsw_build gives for n == 0 under the handle's config
    isl_hnsw* empty = nullptr;
    ISL_TRY(isl_hnsw_from_layers(h->m, h->m0, h->ef_construction, (int32_t)core->cfg.metric, 0, 0, 0, nullptr, nullptr,
                                 nullptr, 0, 0, 0, nullptr, h->device, &empty));
    shrunk.reset(empty);
  } else {
    ISL_TRY(shrink(opts, h, remap, survivors, shrunk));
  }
  ISL_TRY(install_core(h, shrunk.get(), n ? h->dim : 0, n ? shrunk->core->device : h->device, "shrink"));
  isl_build::write_remap(&remap, n0, out_remap);
  if (out_len) *out_len = n;
  return ISL_OK;
}

}  // extern "C"
