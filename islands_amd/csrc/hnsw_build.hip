// HnswGraph::insert on the device (src/core/hnsw.rs:214-329) and the read-back side of isl_hnsw.
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
//      the selection (build.hip: truncation or select()) and link_kernel's HNSW mode.
// The steps follow from `levels` alone (a node above the current top layer is alone in its step), so the
// whole plan is laid out once: the nodes of a step sorted by level, highest first -- the nodes that have
// layer L are then a prefix of the step.
// With batch = 1 and ISL_SELECT_REFERENCE this is the reference's construction, list by list.
#include "device_common.hip.h"
#include "build_internal.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

using namespace isl_dev;
using isl_build::BuildParams;

struct DescentParams {
  const float* emb;
  const float* norm2;
  uint64_t stride;
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
template <int METRIC_API>
__global__ __launch_bounds__(64) void insert_descent_kernel(DescentParams p) {
  constexpr int METRIC = METRIC_API == ISL_METRIC_COSINE ? METRIC_COSINE_PRE : METRIC_API;
  extern __shared__ __align__(16) unsigned char smem[];
  float* tile = reinterpret_cast<float*>(smem);
  float* qs = tile + TILE_ROWS * TILE_LD;
  const uint32_t lane = threadIdx.x, b = blockIdx.x;
  if (b >= p.B) return;
  const uint32_t node = p.node_ids[b];
  const uint32_t level = p.levels[node];
  const float q_norm = load_query<METRIC>(p.emb + (uint64_t)node * p.stride, p.d, qs);
  uint32_t cur = p.entry, cV = 1;
  const float e_aux = METRIC == METRIC_COSINE_PRE ? p.norm2[cur] : 0.0f;
  float cd = rl_f(wave_distances<METRIC>(p.emb, p.stride, p.d, cur, 1, qs, tile, q_norm, e_aux), 0);
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
        const float gd = wave_distances<METRIC>(p.emb, p.stride, p.d, gid, R, qs, tile, q_norm, aux);
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

void launch_descent(int metric, uint32_t grid, size_t lds, const DescentParams& p) {
  switch (metric) {
    case ISL_METRIC_COSINE: hipLaunchKernelGGL(insert_descent_kernel<ISL_METRIC_COSINE>, dim3(grid), dim3(64), lds, 0, p); break;
    case ISL_METRIC_EUCLIDEAN: hipLaunchKernelGGL(insert_descent_kernel<ISL_METRIC_EUCLIDEAN>, dim3(grid), dim3(64), lds, 0, p); break;
    case ISL_METRIC_DOT: hipLaunchKernelGGL(insert_descent_kernel<ISL_METRIC_DOT>, dim3(grid), dim3(64), lds, 0, p); break;
    default: hipLaunchKernelGGL(insert_descent_kernel<ISL_METRIC_MANHATTAN>, dim3(grid), dim3(64), lds, 0, p); break;
  }
}

// One step of the plan: nodes order[first .. first + count), sorted by level (highest first).
struct Step {
  uint64_t first;
  uint32_t count;
  uint32_t top;  // the step's highest level
};

// min(batch, n - id0, max(1, id0 / 8)) nodes per step (the LeannIndex builder's ramp), cut so that a node
// above the current top layer is the only node of its step.
void plan_steps(const std::vector<uint32_t>& lv, uint64_t batch, std::vector<Step>& steps, std::vector<uint32_t>& order) {
  const uint64_t n = lv.size();
  order.resize(n);
  for (uint64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
  uint32_t max_level = n ? lv[0] : 0;
  for (uint64_t id0 = 1; id0 < n;) {
    uint64_t nb = std::min<uint64_t>(std::min<uint64_t>(batch, n - id0), std::max<uint64_t>(1, id0 / 8));
    if (lv[id0] > max_level) {
      nb = 1;
    } else {
      for (uint64_t j = 1; j < nb; ++j)
        if (lv[id0 + j] > max_level) { nb = j; break; }
    }
    uint32_t top = 0;
    for (uint64_t j = 0; j < nb; ++j) top = std::max(top, lv[id0 + j]);
    if (nb > 1)
      std::stable_sort(order.begin() + id0, order.begin() + id0 + nb, [&](uint32_t a, uint32_t b) { return lv[a] > lv[b]; });
    steps.push_back(Step{id0, (uint32_t)nb, top});
    max_level = std::max(max_level, top);
    id0 += nb;
  }
}

// every layer of `h` in CSR form on the host (under h->host_mu)
isl_status ensure_host_layers(const isl_hnsw* h) {
  if (h->host_valid) return ISL_OK;
  const isl_index* c = h->core;
  const uint64_t n = c->num_nodes;
  std::vector<std::vector<uint64_t>> off, adj;
  if (n) {
    ISL_TRY(isl::materialise_host_csr(c));
    const uint64_t layers = std::max<uint64_t>(c->hnsw_layers, 1);
    off.resize(layers);
    adj.resize(layers);
    off[0] = c->node_offsets;
    adj[0] = c->neighbors;
    if (layers > 1) ISL_TRY(isl::use_device(c->device));
    std::vector<uint32_t> tmp;
    for (uint64_t L = 1; L < layers; ++L) {
      off[L].assign(n + 1, 0);
      ISL_HIP(hipMemcpy(off[L].data(), h->layer_off[L], (n + 1) * 8, hipMemcpyDeviceToHost));
      const uint64_t nnz = off[L][n];
      tmp.resize(nnz);
      if (nnz) ISL_HIP(hipMemcpy(tmp.data(), h->layer_adj[L], nnz * 4, hipMemcpyDeviceToHost));
      adj[L].assign(tmp.begin(), tmp.end());
    }
  }
  h->h_off.swap(off);
  h->h_adj.swap(adj);
  h->host_valid = true;
  return ISL_OK;
}

// HnswNode::level: what the caller supplied, or 0 for all where a handle came without levels
uint64_t level_of(const isl_index* c, uint64_t i) { return i < c->levels.size() ? c->levels[i] : 0; }

// node rows [i0, i0 + cnt) of the handle's f32 provider -> host
isl_status read_rows(const isl_index* c, uint64_t i0, uint64_t cnt, float* out) {
  if (!cnt || !c->emb_d) return ISL_OK;
  if (!c->d_emb) return isl::fail(ISL_ERR_EMBEDDING, "Embedding error: no embedding provider attached");
  ISL_TRY(isl::use_device(c->device));
  ISL_HIP(hipMemcpy2D(out, c->emb_d * 4, c->d_emb + i0 * c->emb_stride, c->emb_stride * 4, c->emb_d * 4, cnt,
                      hipMemcpyDeviceToHost));
  return ISL_OK;
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

isl_status isl_hnsw_random_levels(uint64_t seed, uint64_t n, double ml, uint64_t max_layers, uint64_t* out) {
  if (!out && n) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  if (max_layers == 0 || !std::isfinite(ml) || ml < 0.0)
    return isl::fail(ISL_ERR_INVALID_ARGUMENT, "isl_hnsw_random_levels: max_layers >= 1 and a finite ml >= 0");
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;  // splitmix64
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const double r = ((double)(z >> 11) + 0.5) * (1.0 / 9007199254740992.0);  // in (0, 1)
    const double lv = std::floor(-std::log(r) * ml);                          // hnsw.rs:209
    out[i] = lv >= (double)(max_layers - 1) ? max_layers - 1 : (uint64_t)lv;
  }
  return ISL_OK;
}

isl_status isl_hnsw_build(const isl_hnsw_config* cfg_in, const isl_build_options* opts_in, const float* vectors,
                          uint64_t n, uint64_t d, const uint64_t* levels_in, uint64_t level_seed, int32_t mem,
                          int32_t device, isl_hnsw** out) {
  using isl::fail;
  if (!out || (!vectors && n)) return fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  isl_build_options opts;
  isl_build_options_default(&opts);
  if (opts_in) {
    ISL_TRY(isl_build::check_build_options(opts_in, true));
    opts = *opts_in;
  }
  isl_hnsw_config cfg;
  if (cfg_in) cfg = *cfg_in;
  else isl_hnsw_config_default(&cfg);
  // HnswConfig::validate, hnsw.rs:72-85
  if (cfg.m == 0) return fail(ISL_ERR_INVALID_CONFIG, "Invalid configuration: M must be > 0");
  if (cfg.m0 < cfg.m) return fail(ISL_ERR_INVALID_CONFIG, "Invalid configuration: M0 must be >= M");
  if (cfg.ef_construction < cfg.m)
    return fail(ISL_ERR_INVALID_CONFIG, "Invalid configuration: ef_construction must be >= M");
  if (cfg.metric > ISL_METRIC_MANHATTAN) return fail(ISL_ERR_INVALID_ARGUMENT, "unknown metric");
  if (n == 0) {  // HnswGraph::new: no nodes, no entry point, no dimension
    ISL_TRY(isl_hnsw_from_layers(cfg.m, cfg.m0, cfg.ef_construction, (int32_t)cfg.metric, 0, 0, 0, nullptr, nullptr,
                                 nullptr, 0, 0, 0, nullptr, device, out));
    (*out)->ml = cfg.ml;
    (*out)->max_layers = cfg.max_layers;
    return ISL_OK;
  }
  if (d == 0) return fail(ISL_ERR_EMPTY_COLLECTION, "Empty vector collection");
  std::vector<uint64_t> drawn;
  if (!levels_in) {
    drawn.resize(n);
    ISL_TRY(isl_hnsw_random_levels(level_seed, n, cfg.ml, cfg.max_layers, drawn.data()));
    levels_in = drawn.data();
  }
  uint64_t top = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (levels_in[i] >= cfg.max_layers)
      return fail(ISL_ERR_INVALID_ARGUMENT, "levels[%llu] = %llu is not below max_layers = %llu", (unsigned long long)i,
                  (unsigned long long)levels_in[i], (unsigned long long)cfg.max_layers);
    top = std::max(top, levels_in[i]);
  }
  if (cfg.m0 > 128) return fail(ISL_ERR_UNSUPPORTED, "the device builder keeps lists of up to 129 ids: m0 <= 128");
  if (cfg.ef_construction > 512) return fail(ISL_ERR_UNSUPPORTED, "ef_construction <= 512 on the device");
  if (n >= 0x7FFFFFF0ull) return fail(ISL_ERR_UNSUPPORTED, "num_nodes exceeds the device id range");
  if (top >= 64) return fail(ISL_ERR_UNSUPPORTED, "the device builder keeps up to 64 layers");
  const bool diverse = opts.select_rule == ISL_SELECT_DIVERSE;
  const uint64_t batch = opts.batch ? opts.batch : 1;
  ISL_TRY(isl::use_device(device));

  std::vector<uint32_t> lv(n);
  for (uint64_t i = 0; i < n; ++i) lv[i] = (uint32_t)levels_in[i];
  std::vector<Step> steps;
  std::vector<uint32_t> order;
  plan_steps(lv, batch, steps, order);
  uint64_t B = 1;
  for (const Step& s : steps) B = std::max<uint64_t>(B, s.count);

  const uint32_t m = (uint32_t)cfg.m, m0 = (uint32_t)cfg.m0, ef = (uint32_t)cfg.ef_construction;
  const uint64_t layers = top + 1;
  // the graph under construction: an index whose adjacency is the table of the layer being searched
  isl_leann_config lcfg;
  isl_leann_config_paper_default(&lcfg);
  lcfg.metric = cfg.metric;
  lcfg.prune_ratio = 0.0f;
  isl_index* g = nullptr;
  ISL_TRY(isl_index_new(&lcfg, &g));
  std::vector<void*> tmp;      // freed on every way out
  std::vector<void*> keep;     // handed to the finished graph
  isl_index* res = nullptr;
  auto cleanup = [&]() {
    for (void* q : tmp) (void)hipFree(q);
    g->d_ell = nullptr; g->d_ell_deg = nullptr;
    g->build_q_entry = nullptr; g->build_q_evals = nullptr;
    isl_index_free(g);
  };
  auto bail = [&](isl_status st) {
    const isl::ErrorRecord rec = isl::last_error();
    for (void* q : keep) (void)hipFree(q);
    if (res) { res->hnsw_owned.clear(); isl_index_free(res); }
    cleanup();
    isl::last_error() = rec;
    return st;
  };
  auto dalloc = [&](size_t bytes, std::vector<void*>& owner) -> void* {
    void* q = nullptr;
    if (hipMalloc(&q, bytes ? bytes : 4) != hipSuccess) return nullptr;
    owner.push_back(q);
    return q;
  };
  g->is_hnsw = true;  // HnswGraph heap order: distance alone
  g->host_csr_valid = false;
  g->num_nodes = n;
  g->device = device;
  g->has_dimension = true;
  g->dimension = d;
  g->max_degree = m0;  // the widest list a construction search can meet, on any layer
  isl_status st = isl_set_embeddings(g, vectors, n, d, ISL_DTYPE_F32, mem);
  if (st != ISL_OK) return bail(st);

  std::vector<uint32_t*> tab(layers), deg(layers);
  bool ok = true;
  for (uint64_t L = 0; L < layers && ok; ++L) {
    const uint64_t W = (L ? m : m0) + 1;
    tab[L] = (uint32_t*)dalloc(n * W * 4, tmp);
    deg[L] = (uint32_t*)dalloc(n * 4, tmp);
    ok = tab[L] && deg[L] && hipMemset(deg[L], 0, n * 4) == hipSuccess;
  }
  uint32_t** d_tab = (uint32_t**)dalloc(layers * sizeof(void*), tmp);
  uint32_t** d_deg = (uint32_t**)dalloc(layers * sizeof(void*), tmp);
  uint32_t* lock = (uint32_t*)dalloc(n * 4, tmp);
  uint32_t* d_lv = (uint32_t*)dalloc(n * 4, tmp);
  uint32_t* d_order = (uint32_t*)dalloc(n * 4, tmp);
  uint32_t* cur_of = (uint32_t*)dalloc(n * 4, tmp);
  uint32_t* evals_of = (uint32_t*)dalloc(n * 4, tmp);
  float* qbuf = (float*)dalloc(B * d * 4, tmp);
  uint32_t* q_entry = (uint32_t*)dalloc(B * 2 * 4, tmp);
  uint64_t* cand_ids = (uint64_t*)dalloc(B * ef * 8, tmp);
  float* cand_dist = (float*)dalloc(B * ef * 4, tmp);
  uint32_t* cand_cnt = (uint32_t*)dalloc(B * 4, tmp);
  uint32_t* sel = (uint32_t*)dalloc(B * m0 * 4, tmp);
  uint32_t* sel_cnt = (uint32_t*)dalloc(B * 4, tmp);
  if (!ok || !d_tab || !d_deg || !lock || !d_lv || !d_order || !cur_of || !evals_of || !qbuf || !q_entry || !cand_ids ||
      !cand_dist || !cand_cnt || !sel || !sel_cnt)
    return bail(fail(ISL_ERR_DEVICE, "hipMalloc failed for the HnswGraph builder (%llu layer tables)",
                     (unsigned long long)layers));
  if (hipMemset(lock, 0, n * 4) != hipSuccess || hipMemset(cur_of, 0, n * 4) != hipSuccess ||
      hipMemset(evals_of, 0, n * 4) != hipSuccess ||
      hipMemcpy(d_lv, lv.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_order, order.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_tab, tab.data(), layers * sizeof(void*), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_deg, deg.data(), layers * sizeof(void*), hipMemcpyHostToDevice) != hipSuccess)
    return bail(fail(ISL_ERR_DEVICE, "cannot stage the build plan"));

  DescentParams dp{};
  dp.emb = g->d_emb; dp.norm2 = g->d_norm2; dp.stride = g->emb_stride; dp.d = (uint32_t)d;
  dp.tab = d_tab; dp.deg = d_deg; dp.W = m + 1; dp.levels = d_lv;
  dp.cur_of = cur_of; dp.evals_of = evals_of;
  BuildParams p{};
  p.emb = g->d_emb; p.norm2 = g->d_norm2; p.stride = g->emb_stride; p.d = (uint32_t)d;
  p.lock = lock; p.ef = ef;
  p.cand_ids = cand_ids; p.cand_dist = cand_dist; p.cand_cnt = cand_cnt; p.sel = sel; p.sel_cnt = sel_cnt;
  p.alpha = opts.alpha; p.keep_pruned = opts.keep_pruned ? 1u : 0u;
  p.node_levels = d_lv; p.cur_of = cur_of;
  g->build_q_entry = q_entry;
  g->build_q_evals = q_entry + B;
  const int metric = (int)cfg.metric;

  // node 0: entry point, max_level = its level, every list empty (hnsw.rs:240-245)
  uint64_t entry = 0, max_level = lv[0];
  for (const Step& s : steps) {
    const uint32_t* ids = d_order + s.first;
    dp.node_ids = ids; dp.B = s.count; dp.entry = (uint32_t)entry; dp.max_level = (uint32_t)max_level;
    launch_descent(metric, s.count, isl_build::link_lds(d), dp);
    if (hipGetLastError() != hipSuccess) return bail(fail(ISL_ERR_DEVICE, "descent launch failed"));
    g->has_entry = true;
    g->entry_point = entry;
    uint32_t cnt = 0;  // nodes of the step that have the layer: a prefix, growing as the layer falls
    for (uint64_t L = s.top + 1; L-- > 0;) {
      while (cnt < s.count && lv[order[s.first + cnt]] >= L) ++cnt;
      const uint32_t M = L ? m : m0;
      hipLaunchKernelGGL(gather_layer_kernel, dim3((uint32_t)(((uint64_t)cnt * d + 255) / 256)), dim3(256), 0, 0,
                         g->d_emb, g->emb_stride, (uint32_t)d, ids, cnt, cur_of, evals_of, qbuf, g->build_q_entry,
                         g->build_q_evals);
      if (hipGetLastError() != hipSuccess) return bail(fail(ISL_ERR_DEVICE, "gather launch failed"));
      g->d_ell = tab[L];
      g->d_ell_deg = deg[L];
      g->ell_w = M + 1;
      st = isl::search_device_sync(g, qbuf, cnt, d, ef, ef, cand_ids, cand_dist, cand_cnt, nullptr);
      if (st != ISL_OK) return bail(st);
      p.ell = tab[L]; p.ell_deg = deg[L]; p.W = M + 1; p.m0 = M;
      p.layer = (uint32_t)L; p.node_ids = ids; p.B = cnt; p.id0 = 0;
      p.locking = s.count > 1;
      if (diverse) {
        isl_build::select_diverse(metric, cnt, isl_build::select_lds(d, ef, M), p);
        isl_build::link_hnsw(metric, true, cnt, isl_build::select_lds(d, M + 1, M), p);
      } else {
        isl_build::select_truncate(cnt, p);
        isl_build::link_hnsw(metric, false, cnt, isl_build::link_lds(d), p);
      }
      if (hipGetLastError() != hipSuccess) return bail(fail(ISL_ERR_DEVICE, "builder launch failed"));
    }
    if (hipDeviceSynchronize() != hipSuccess) return bail(fail(ISL_ERR_DEVICE, "builder kernels failed"));
    if (s.top > max_level) {  // hnsw.rs:322-325 (such a node is alone in its step)
      max_level = s.top;
      entry = order[s.first];
    }
  }

  // per-layer table -> CSR; layer 0 becomes the core index, the layers above the descent's arrays
  std::vector<const uint64_t*> offs(max_level + 1, nullptr);
  std::vector<const uint32_t*> adjs(max_level + 1, nullptr);
  std::vector<uint32_t> hdeg(n);
  std::vector<uint64_t> off(n + 1, 0);
  for (uint64_t L = 0; L <= max_level; ++L) {
    if (hipMemcpy(hdeg.data(), deg[L], n * 4, hipMemcpyDeviceToHost) != hipSuccess)
      return bail(fail(ISL_ERR_DEVICE, "cannot read the degrees back"));
    for (uint64_t i = 0; i < n; ++i) off[i + 1] = off[i] + hdeg[i];
    std::vector<void*>& owner = L ? keep : tmp;
    uint64_t* d_off = (uint64_t*)dalloc((n + 1) * 8, owner);
    uint32_t* d_adj = (uint32_t*)dalloc((off[n] ? off[n] : 1) * 4, owner);
    if (!d_off || !d_adj || hipMemcpy(d_off, off.data(), (n + 1) * 8, hipMemcpyHostToDevice) != hipSuccess)
      return bail(fail(ISL_ERR_DEVICE, "hipMalloc failed for the CSR of layer %llu", (unsigned long long)L));
    isl_build::ell_to_csr(tab[L], deg[L], (uint32_t)((L ? m : m0) + 1), d_off, n, d_adj);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)
      return bail(fail(ISL_ERR_DEVICE, "CSR compaction failed"));
    offs[L] = d_off;
    adjs[L] = d_adj;
  }
  st = isl_index_from_device_csr(&lcfg, device, n, offs[0], adjs[0], 1, entry, 1, d, &res);
  if (st != ISL_OK) return bail(st);
  res->is_hnsw = true;
  res->max_level = max_level;
  res->levels.assign(levels_in, levels_in + n);
  offs[0] = nullptr;  // layer 0 lives in the core index (its own copy): the tables carry no pointer for it
  adjs[0] = nullptr;
  if (hipMalloc((void**)&res->d_layer_off, (max_level + 1) * sizeof(void*)) != hipSuccess ||
      hipMalloc((void**)&res->d_layer_adj, (max_level + 1) * sizeof(void*)) != hipSuccess ||
      hipMemcpy((void*)res->d_layer_off, offs.data(), (max_level + 1) * sizeof(void*), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy((void*)res->d_layer_adj, adjs.data(), (max_level + 1) * sizeof(void*), hipMemcpyHostToDevice) != hipSuccess)
    return bail(fail(ISL_ERR_DEVICE, "layer table upload failed"));
  res->hnsw_layers = max_level + 1;
  res->hnsw_owned = keep;
  // the finished graph takes over the rows (and their norms) of the construction graph
  res->d_emb = g->d_emb; res->d_norm2 = g->d_norm2;
  res->nvec = g->nvec; res->emb_d = g->emb_d; res->emb_stride = g->emb_stride;
  g->d_emb = nullptr; g->d_norm2 = nullptr;
  cleanup();
  isl_hnsw* h = new isl_hnsw();
  h->core = res;
  h->m = cfg.m; h->m0 = cfg.m0; h->ef_construction = cfg.ef_construction; h->dim = d;
  h->ml = cfg.ml; h->max_layers = cfg.max_layers;
  h->layer_off = offs;
  h->layer_adj = adjs;
  *out = h;
  return ISL_OK;
}

isl_status isl_hnsw_info(const isl_hnsw* h, int32_t* has_entry, uint64_t* entry, uint64_t* max_level, uint64_t* dim) {
  if (!h || !h->core) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "hnsw handle is NULL");
  if (has_entry) *has_entry = h->core->has_entry ? 1 : 0;
  if (entry) *entry = h->core->has_entry ? h->core->entry_point : 0;
  if (max_level) *max_level = h->core->max_level;
  if (dim) *dim = h->dim;
  return ISL_OK;
}

isl_status isl_hnsw_levels(const isl_hnsw* h, uint64_t* out) {
  if (!h || !h->core) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "hnsw handle is NULL");
  const uint64_t n = h->core->num_nodes;
  if (n && !out) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  for (uint64_t i = 0; i < n; ++i) out[i] = level_of(h->core, i);
  return ISL_OK;
}

isl_status isl_hnsw_get_neighbors(const isl_hnsw* h, uint64_t node, uint64_t layer, uint64_t* out, uint64_t cap,
                                  uint64_t* count, int32_t* has_layer) {
  if (!h || !h->core || !count || (cap && !out)) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  if (node >= h->core->num_nodes) return isl::fail_node(node);
  std::lock_guard<std::mutex> lock(h->host_mu);
  ISL_TRY(ensure_host_layers(h));
  *count = 0;
  if (has_layer) *has_layer = layer <= level_of(h->core, node) ? 1 : 0;
  if (layer > level_of(h->core, node) || layer >= h->h_off.size()) return ISL_OK;
  const uint64_t s = h->h_off[layer][node], e = h->h_off[layer][node + 1];
  *count = e - s;
  for (uint64_t i = 0; i < e - s && i < cap; ++i) out[i] = h->h_adj[layer][s + i];
  return ISL_OK;
}

isl_status isl_hnsw_get_vector(const isl_hnsw* h, uint64_t node, float* out) {
  if (!h || !h->core || !out) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  if (node >= h->core->num_nodes) return isl::fail_node(node);
  return read_rows(h->core, node, 1, out);
}

isl_status isl_hnsw_to_bytes(const isl_hnsw* h, uint8_t** out, size_t* len) {
  if (!h || !h->core || !out || !len) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  const isl_index* c = h->core;
  const uint64_t n = c->num_nodes, d = n ? c->emb_d : 0;
  try {
    std::lock_guard<std::mutex> lock(h->host_mu);
    ISL_TRY(ensure_host_layers(h));
    std::vector<float> rows((size_t)n * d);
    ISL_TRY(read_rows(c, 0, n, rows.data()));
    std::vector<uint8_t> b;
    auto raw = [&](const void* q, size_t bytes) { const uint8_t* s = (const uint8_t*)q; b.insert(b.end(), s, s + bytes); };
    auto u64 = [&](uint64_t v) { raw(&v, 8); };
    // layout: hnsw.hip, above hnsw_from_bytes_impl
    u64(h->m); u64(h->m0); u64(h->ef_construction);
    raw(&h->ml, 8);
    const uint32_t metric = c->cfg.metric;
    raw(&metric, 4);
    u64(h->max_layers);
    u64(n);
    for (uint64_t i = 0; i < n; ++i) {
      u64(i); u64(i); u64(d);
      raw(rows.data() + (size_t)i * d, d * 4);
      const uint64_t lvl = level_of(c, i);
      u64(lvl + 1);
      for (uint64_t L = 0; L <= lvl; ++L) {
        if (L >= h->h_off.size()) { u64(0); continue; }
        const uint64_t s = h->h_off[L][i], e = h->h_off[L][i + 1];
        u64(e - s);
        raw(h->h_adj[L].data() + s, (e - s) * 8);
      }
      u64(lvl);
    }
    const uint8_t one = 1, zero = 0;
    if (c->has_entry) { raw(&one, 1); u64(c->entry_point); } else raw(&zero, 1);
    u64(c->max_level);
    if (c->has_dimension) { raw(&one, 1); u64(c->dimension); } else raw(&zero, 1);
    u64(n);  // next_id
    uint8_t* buf = (uint8_t*)malloc(b.size() ? b.size() : 1);
    if (!buf) return isl::fail(ISL_ERR_SERIALIZATION, "Serialization error: out of memory");
    memcpy(buf, b.data(), b.size());
    *out = buf;
    *len = b.size();
    return ISL_OK;
  } catch (const std::exception& e) {
    return isl::fail(ISL_ERR_SERIALIZATION, "Serialization error: %s", e.what());
  }
}

}  // extern "C"
