// HnswGraph facade (src/core/hnsw.rs:149-515) on gfx950: everything about a finished graph -- handing one
// over (from_layers, from_bytes), searching it, reading it back (info, levels, neighbours, rows, to_bytes).
// The graph is handed over layer by layer in CSR form; layer 0 and the node vectors live in an
// internal LeannIndex-like handle (so the same exact kernel, visited bitmap and row staging are
// used), the upper layers are kept as device CSR arrays for the greedy descent.  isl_hnsw_build
// (hnsw_build.hip) constructs one on the device and installs its layers through attach_upper_layers.
#include "common.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

__global__ void hnsw_convert_adj(const uint64_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n,
                                 uint32_t* __restrict__ flag) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint64_t v = in[i];
    if (v > 0x7FFFFFF0ull) { atomicOr(flag, 1u); v = 0x7FFFFFF0ull; }
    out[i] = (uint32_t)v;
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

// node rows [i0, i0 + cnt) of the handle's provider -> host, as f32: the rows themselves, or the exact images of
// bf16 rows -- their bits staged on the host a chunk at a time and widened there (nothing is allocated on the device)
isl_status read_rows(const isl_index* c, uint64_t i0, uint64_t cnt, float* out) {
  const uint64_t d = c->rows.d(), stride = c->rows.stride();
  if (!cnt || !d) return ISL_OK;
  if (!c->rows.f32() && !c->rows.bf16())
    return isl::fail(ISL_ERR_EMBEDDING, "Embedding error: no embedding provider attached");
  ISL_TRY(isl::use_device(c->device));
  if (c->rows.f32()) {
    ISL_HIP(hipMemcpy2D(out, d * 4, c->rows.f32() + i0 * stride, stride * 4, d * 4, cnt, hipMemcpyDeviceToHost));
    return ISL_OK;
  }
  const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(cnt, ((uint64_t)16 << 20) / d));  // 32 MiB of bits
  std::vector<uint16_t> bits((size_t)(chunk * d));
  for (uint64_t o = 0; o < cnt; o += chunk) {
    const uint64_t rows = std::min(chunk, cnt - o);
    ISL_HIP(hipMemcpy2D(bits.data(), d * 2, c->rows.bf16() + (i0 + o) * stride, stride * 2, d * 2, rows,
                        hipMemcpyDeviceToHost));
    uint32_t* w = reinterpret_cast<uint32_t*>(out + (size_t)(o * d));
    for (uint64_t j = 0; j < rows * d; ++j) w[j] = (uint32_t)bits[j] << 16;
  }
  return ISL_OK;
}

}  // namespace

isl_status isl::hnsw_config_validate(uint64_t m, uint64_t m0, uint64_t ef_construction, int64_t metric) {
  // HnswConfig::validate, hnsw.rs:72-85
  if (m == 0) return fail(ISL_ERR_INVALID_CONFIG, "Invalid configuration: M must be > 0");
  if (m0 < m) return fail(ISL_ERR_INVALID_CONFIG, "Invalid configuration: M0 must be >= M");
  if (ef_construction < m) return fail(ISL_ERR_INVALID_CONFIG, "Invalid configuration: ef_construction must be >= M");
  if (metric < 0 || metric > ISL_METRIC_MANHATTAN) return fail(ISL_ERR_INVALID_ARGUMENT, "unknown metric");
  return ISL_OK;
}

isl_status isl::hnsw_row_dtype(int32_t dtype) {
  if (dtype == ISL_DTYPE_FP8_E4M3) return fail(ISL_ERR_UNSUPPORTED, "an HnswGraph keeps float32 or bf16 rows, not fp8");
  if (dtype != ISL_DTYPE_F32 && dtype != ISL_DTYPE_BF16) return fail(ISL_ERR_INVALID_ARGUMENT, "unknown row dtype");
  return ISL_OK;
}

isl_status isl::attach_upper_layers(isl_hnsw* h, const std::vector<const uint64_t*>& offs,
                                    const std::vector<const uint32_t*>& adjs) {
  isl_index* c = h->core;
  const size_t bytes = offs.size() * sizeof(void*);
  if (c->d_layer_off.reserve(offs.size()) != ISL_OK || c->d_layer_adj.reserve(offs.size()) != ISL_OK ||
      hipMemcpy(c->d_layer_off, offs.data(), bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->d_layer_adj, adjs.data(), bytes, hipMemcpyHostToDevice) != hipSuccess)
    return fail(ISL_ERR_DEVICE, "layer table upload failed");
  c->hnsw_layers = offs.size();
  h->layer_off = offs;
  h->layer_adj = adjs;
  return ISL_OK;
}

extern "C" {

void isl_hnsw_free(isl_hnsw* h) {
  if (!h) return;
  isl_index_free(h->core);
  delete h;
}

uint64_t isl_hnsw_len(const isl_hnsw* h) { return h && h->core ? h->core->num_nodes : 0; }

isl_status isl_hnsw_last_stats(const isl_hnsw* h, isl_search_stats* out) {
  if (!h || !h->core) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "hnsw handle is NULL");
  return isl_search_last_stats(h->core, out);
}

isl_status isl_hnsw_from_layers(uint64_t m, uint64_t m0, uint64_t ef_construction, int32_t metric,
                                uint64_t num_nodes, uint64_t d, uint64_t num_layers,
                                const uint64_t* const* layer_offsets,
                                const uint64_t* const* layer_neighbors, const uint64_t* levels,
                                int32_t has_entry, uint64_t entry_point, uint64_t max_level,
                                const float* vectors, int32_t device, isl_hnsw** out) {
  return isl_hnsw_from_layers_rows(m, m0, ef_construction, metric, num_nodes, d, num_layers, layer_offsets,
                                   layer_neighbors, levels, has_entry, entry_point, max_level, vectors, ISL_DTYPE_F32,
                                   device, out);
}

isl_status isl_hnsw_from_layers_rows(uint64_t m, uint64_t m0, uint64_t ef_construction, int32_t metric,
                                     uint64_t num_nodes, uint64_t d, uint64_t num_layers,
                                     const uint64_t* const* layer_offsets,
                                     const uint64_t* const* layer_neighbors, const uint64_t* levels,
                                     int32_t has_entry, uint64_t entry_point, uint64_t max_level,
                                     const void* rows, int32_t dtype, int32_t device, isl_hnsw** out) {
  if (!out) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "out is NULL");
  ISL_TRY(isl::hnsw_row_dtype(dtype));
  ISL_TRY(isl::hnsw_config_validate(m, m0, ef_construction, metric));
  if (num_nodes && (num_layers == 0 || max_level >= num_layers || !layer_offsets || !layer_neighbors))
    return isl::fail(ISL_ERR_INVALID_ARGUMENT, "layers do not cover max_level");
  isl_hnsw* h = new isl_hnsw();
  h->m = m; h->m0 = m0; h->ef_construction = ef_construction; h->dim = d;
  h->ml = 1.0 / std::log(16.0);  // HnswConfig::default(), hnsw.rs:37-48 (from_bytes: as parsed)
  h->max_layers = 16;
  h->device = device;
  auto bail = [&](isl_status st) { isl_hnsw_free(h); return st; };
  isl_leann_config cfg;
  isl_leann_config_paper_default(&cfg);
  cfg.metric = (uint32_t)metric;
  cfg.prune_ratio = 0.0f;
  isl_status st = isl_index_from_csr(&cfg, num_nodes, num_nodes ? layer_offsets[0] : nullptr,
                                     num_nodes ? layer_neighbors[0] : nullptr, levels, nullptr,
                                     has_entry, entry_point, max_level, num_nodes ? 1 : 0, d, &h->core);
  if (st != ISL_OK) return bail(st);
  if (num_nodes == 0) { h->core->is_hnsw = true; *out = h; return ISL_OK; }
  st = isl_index_upload(h->core, device);
  if (st != ISL_OK) return bail(st);
  // (the rows go in before the core becomes a facade's: isl_set_embeddings refuses a caller who swaps a facade's
  // rows for another type, as Scaffold::open of the builder has it)
  st = isl_set_embeddings(h->core, rows, num_nodes, d, dtype, ISL_MEM_HOST);
  if (st != ISL_OK) return bail(st);
  h->core->is_hnsw = true;
  // upper layers -> device CSR (u64 offsets, u32 ids)
  isl_index* c = h->core;
  std::vector<const uint64_t*> offs(max_level + 1, nullptr);
  std::vector<const uint32_t*> adjs(max_level + 1, nullptr);
  isl::DeviceBuffer<uint32_t> d_flag;
  if (d_flag.reserve(1) != ISL_OK || hipMemset(d_flag, 0, 4) != hipSuccess)
    return bail(isl::fail(ISL_ERR_DEVICE, "hipMalloc failed"));
  for (uint64_t L = 1; L <= max_level; ++L) {
    const uint64_t* off = layer_offsets[L];
    uint64_t nnz = off[num_nodes];
    auto layer_array = [&](uint64_t bytes) -> void* {  // owned by the index from the start
      auto& b = c->hnsw_owned.emplace_back();
      return b.reserve(bytes) == ISL_OK ? b.get() : nullptr;
    };
    uint64_t* d_off = static_cast<uint64_t*>(layer_array((num_nodes + 1) * 8));
    uint32_t* d_adj = static_cast<uint32_t*>(layer_array((nnz ? nnz : 1) * 4));
    isl::DeviceBuffer<uint64_t> d_tmp;
    if (!d_off || !d_adj || d_tmp.reserve(nnz ? nnz : 1) != ISL_OK)
      return bail(isl::fail(ISL_ERR_DEVICE, "hipMalloc failed for layer %llu", (unsigned long long)L));
    hipError_t e = hipMemcpy(d_off, off, (num_nodes + 1) * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz) e = hipMemcpy(d_tmp, layer_neighbors[L], nnz * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz) {
      hipLaunchKernelGGL(hnsw_convert_adj, dim3(256), dim3(256), 0, 0, d_tmp.get(), d_adj, nnz, d_flag.get());
      e = hipDeviceSynchronize();
    }
    if (e != hipSuccess) return bail(isl::fail(ISL_ERR_DEVICE, "layer upload failed: %s", hipGetErrorString(e)));
    offs[L] = d_off;
    adjs[L] = d_adj;
  }
  uint32_t flag = 0;
  (void)hipMemcpy(&flag, d_flag, 4, hipMemcpyDeviceToHost);
  if (flag) return bail(isl::fail(ISL_ERR_UNSUPPORTED, "node ids above the device id range"));
  st = isl::attach_upper_layers(h, offs, adjs);
  if (st != ISL_OK) return bail(st);
  *out = h;
  return ISL_OK;
}

// HnswGraph::from_bytes, hnsw.rs:511-514: bincode of the derive(Serialize) struct (hnsw.rs:150-164).
// bincode 1.x default layout as in api_index.hip (little-endian, fixed-width, usize = u64, Vec and
// HashMap = u64 length + items, Option = u8 tag, C-like enum = u32 variant index):
//   config { m, m0, ef_construction: u64; ml: f64; metric: u32; max_layers: u64 }          hnsw.rs:15-28
//   nodes: u64 count, then (key: u64, HnswNode { id: u64; vector: Vec<f32>; connections:
//          Vec<Vec<u64>>; level: u64 }) in the writer's HashMap order                      hnsw.rs:90-99
//   entry_point: Option<u64>; max_level: u64; dimension: Option<u64>; next_id: u64
// The byte layout is unpinned by the reference (tests round-trip only, hnsw.rs:689-709) and the
// pinned bincode is 3.0.0 (Cargo.lock:838-841); this is the documented 1.x-compatible intent.
// Node ids must be 0..n-1 (insert assigns them from next_id, hnsw.rs:218-219), in any order.
static isl_status hnsw_from_bytes_impl(const uint8_t* bytes, size_t len, int32_t device, isl_hnsw** out);

isl_status isl_hnsw_from_bytes(const uint8_t* bytes, size_t len, int32_t device, isl_hnsw** out) {
  if (!out || (!bytes && len)) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  // every length in the buffer is untrusted: nothing may throw across the C boundary
  try {
    return hnsw_from_bytes_impl(bytes, len, device, out);
  } catch (const std::exception& e) {
    return isl::fail(ISL_ERR_DESERIALIZATION, "Deserialization error: %s", e.what());
  }
}

static isl_status hnsw_from_bytes_impl(const uint8_t* bytes, size_t len, int32_t device, isl_hnsw** out) {
  size_t pos = 0;
  bool ok = true;
  auto need = [&](size_t n) { if (ok && len - pos < n) ok = false; return ok; };
  auto u64 = [&]() -> uint64_t { uint64_t v = 0; if (need(8)) { memcpy(&v, bytes + pos, 8); pos += 8; } return v; };
  auto u32 = [&]() -> uint32_t { uint32_t v = 0; if (need(4)) { memcpy(&v, bytes + pos, 4); pos += 4; } return v; };
  auto u8 = [&]() -> uint8_t { uint8_t v = 0; if (need(1)) { v = bytes[pos]; pos += 1; } return v; };
  auto bad = [&](const char* what) {
    return isl::fail(ISL_ERR_DESERIALIZATION, "Deserialization error: %s (offset %llu of %llu)", what,
                     (unsigned long long)pos, (unsigned long long)len);
  };
  const uint64_t m = u64(), m0 = u64(), efc = u64();
  const uint64_t ml_bits = u64();  // ml: f64, only used by random_level (hnsw.rs:196-200); kept for to_bytes
  const uint32_t metric = u32();
  const uint64_t max_layers = u64();
  const uint64_t n = u64();
  if (!ok) return bad("truncated header");
  if (metric > ISL_METRIC_MANHATTAN) return bad("unknown DistanceMetric variant");
  if (n > (len - pos) / 32) return bad("node count exceeds the buffer");  // >= 32 bytes per node
  std::vector<uint64_t> levels(n, 0);
  std::vector<float> vectors;
  std::vector<uint8_t> seen(n, 0);
  std::vector<std::vector<std::vector<uint64_t>>> conn(n);
  uint64_t d = 0;
  for (uint64_t e = 0; e < n && ok; ++e) {
    const uint64_t key = u64(), id = u64(), vlen = u64();
    if (!ok) break;
    if (key != id) return bad("HashMap key differs from HnswNode::id");
    if (id >= n || seen[id]) return isl::fail(ISL_ERR_UNSUPPORTED, "HnswGraph node ids must be 0..n-1 (id %llu of %llu nodes)",
                                              (unsigned long long)id, (unsigned long long)n);
    seen[id] = 1;
    // vlen * 4 and n * d must not wrap: every node carries its vector inside the buffer
    if (vlen > (len - pos) / 4) return bad("vector length exceeds the buffer");
    if (e == 0) {
      d = vlen;
      if (d && n > (len / 4) / d) return bad("node count times vector length exceeds the buffer");
      vectors.assign((size_t)n * d, 0.0f);
    }
    if (vlen != d) return bad("nodes with different vector lengths");
    if (!need(vlen * 4)) break;
    memcpy(vectors.data() + (size_t)id * d, bytes + pos, vlen * 4);
    pos += vlen * 4;
    const uint64_t nl = u64();
    if (!ok || nl > (len - pos) / 8 + 1) { ok = false; break; }
    conn[id].resize(nl);
    for (uint64_t L = 0; L < nl && ok; ++L) {
      const uint64_t c = u64();
      if (!ok || c > (len - pos) / 8) { ok = false; break; }
      conn[id][L].resize(c);
      if (c) memcpy(conn[id][L].data(), bytes + pos, c * 8);
      pos += c * 8;
    }
    levels[id] = u64();
    // (to_bytes writes level + 1 lists per node; the layer count below bounds every list that exists)
    if (ok && levels[id] >= 64) return bad("implausible node level");
  }
  const uint8_t has_entry = u8();
  const uint64_t entry = has_entry ? u64() : 0;
  const uint64_t max_level = u64();
  const uint8_t has_dim = u8();
  const uint64_t dim = has_dim ? u64() : 0;
  (void)u64();  // next_id
  if (!ok) return bad("truncated input");
  if (has_entry > 1 || has_dim > 1) return bad("invalid Option tag");
  if (pos != len) return bad("trailing bytes");
  if (n && has_dim && dim != d) return bad("dimension differs from the node vectors");
  // per-layer CSR over all nodes
  uint64_t num_layers = max_level + 1;
  for (uint64_t i = 0; i < n; ++i) num_layers = std::max<uint64_t>(num_layers, conn[i].size());
  if (num_layers > 64) return bad("implausible layer count");
  std::vector<std::vector<uint64_t>> offs(num_layers, std::vector<uint64_t>(n + 1, 0)), adjs(num_layers);
  for (uint64_t L = 0; L < num_layers; ++L) {
    for (uint64_t i = 0; i < n; ++i) {
      if (L < conn[i].size()) adjs[L].insert(adjs[L].end(), conn[i][L].begin(), conn[i][L].end());
      offs[L][i + 1] = adjs[L].size();
    }
    if (adjs[L].empty()) adjs[L].push_back(0);
  }
  std::vector<const uint64_t*> po(num_layers), pa(num_layers);
  for (uint64_t L = 0; L < num_layers; ++L) { po[L] = offs[L].data(); pa[L] = adjs[L].data(); }
  ISL_TRY(isl_hnsw_from_layers(m, m0, efc, (int32_t)metric, n, n ? d : dim, num_layers, po.data(), pa.data(),
                               levels.data(), has_entry, entry, max_level, vectors.data(), device, out));
  memcpy(&(*out)->ml, &ml_bits, 8);
  (*out)->max_layers = max_layers;
  return ISL_OK;
}

// ---- reading a graph back: HnswGraph::to_bytes (hnsw.rs:506-509) and the accessors
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

isl_status isl_hnsw_row_storage(const isl_hnsw* h, int32_t* dtype, uint64_t* block_bytes) {
  if (!h || !h->core) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "hnsw handle is NULL");
  return isl_index_row_storage(h->core, dtype, nullptr, block_bytes);
}

isl_status isl_hnsw_to_bytes(const isl_hnsw* h, uint8_t** out, size_t* len) {
  if (!h || !h->core || !out || !len) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  const isl_index* c = h->core;
  const uint64_t n = c->num_nodes, d = n ? c->rows.d() : 0;
  try {
    std::lock_guard<std::mutex> lock(h->host_mu);
    ISL_TRY(ensure_host_layers(h));
    std::vector<float> rows((size_t)n * d);
    ISL_TRY(read_rows(c, 0, n, rows.data()));
    std::vector<uint8_t> b;
    auto raw = [&](const void* q, size_t bytes) { const uint8_t* s = (const uint8_t*)q; b.insert(b.end(), s, s + bytes); };
    auto u64 = [&](uint64_t v) { raw(&v, 8); };
    // the layout hnsw_from_bytes_impl reads (above it)
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

isl_status isl_hnsw_search_batch(const isl_hnsw* h, const float* queries, uint64_t nq, uint64_t d,
                                 uint64_t k, uint64_t ef, uint64_t* out_ids, float* out_dist,
                                 uint32_t* out_count) {
  if (!h || !h->core) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "hnsw handle is NULL");
  // is_empty -> Ok(vec![]), dimension check, ef = max(ef, k): hnsw.rs:459-471, :500 -- all
  // shared with the LeannIndex entry point
  return isl_search_batch(h->core, queries, nq, d, k, ef, out_ids, out_dist, out_count);
}

}  // extern "C"
