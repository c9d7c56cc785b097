// Host side of the C ABI: error records, LeannConfig, LeannIndex lifecycle,
// bincode (de)serialisation, device upload of the CSR graph and of the
// in-memory embedding provider.  Mirrors src/core/leann.rs of the reference;
// each function cites the lines it replaces.
#include "device_common.hip.h"
#include "encoder.hpp"

#include <algorithm>
#include <cmath>
#include <new>

namespace isl {

ErrorRecord& last_error() {
  thread_local ErrorRecord rec;
  return rec;
}

isl_status fail(isl_status st, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  last_error().message = buf;
  return st;
}

// CoreError::DimensionMismatch display text, error.rs:11
isl_status fail_dim(uint64_t expected, uint64_t actual) {
  ErrorRecord& r = last_error();
  r.expected = expected;
  r.actual = actual;
  return fail(ISL_ERR_DIMENSION_MISMATCH, "Vector dimension mismatch: expected %llu, got %llu",
              (unsigned long long)expected, (unsigned long long)actual);
}

// CoreError::NodeNotFound display text, error.rs:31
isl_status fail_node(uint64_t node) {
  last_error().node = node;
  return fail(ISL_ERR_NODE_NOT_FOUND, "Node not found: %llu", (unsigned long long)node);
}

// The device checks (count, architecture) are made once per device and process; later calls only
// select the device -- the search entry points run this on every call.
namespace {
struct DeviceInfo { int state = 0; int ncu = 256; };  // state: 0 unknown, 1 verified gfx950
DeviceInfo g_devices[64];
std::mutex g_devices_mu;
}  // namespace

isl_status use_device(int32_t device) {
  if (device >= 0 && device < 64 && g_devices[device].state == 1) {
    ISL_HIP(hipSetDevice(device));
    return ISL_OK;
  }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    return fail(ISL_ERR_DEVICE, "no HIP device visible (the gfx950 compute path has no CPU fallback)");
  }
  if (device < 0 || device >= n)
    return fail(ISL_ERR_DEVICE, "device %d out of range (%d visible)", device, n);
  ISL_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  ISL_HIP(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(ISL_ERR_DEVICE, "device %d is %s; this library is built for gfx950 only", device,
                prop.gcnArchName);
  if (device < 64) {
    std::lock_guard<std::mutex> lock(g_devices_mu);
    g_devices[device].ncu = prop.multiProcessorCount;
    g_devices[device].state = 1;
  }
  return ISL_OK;
}

int device_cu_count(int32_t device) {
  return (device >= 0 && device < 64 && g_devices[device].state == 1) ? g_devices[device].ncu : 256;
}

void free_workspace(SearchWorkspace& ws) {
  if (ws.ev0) (void)hipEventDestroy(ws.ev0);
  if (ws.ev1) (void)hipEventDestroy(ws.ev1);
  if (ws.ev_in) (void)hipEventDestroy(ws.ev_in);
  if (ws.ev_done) (void)hipEventDestroy(ws.ev_done);
  // (ws.stream belongs to the device's stream pool; the reset frees every buffer of the lane)
  ws = SearchWorkspace{};
}

}  // namespace isl

using namespace isl;

// Up to kSearchLanes searches overlap on their own streams; the runtime's default of 4 hardware
// queues per process would make them share queues and serialise.  Effective when the library is
// loaded before the HIP runtime initialises (an explicit setting in the environment wins).
static int g_hw_queues_at_load = 4;
__attribute__((constructor)) static void isl_default_hw_queues() {
  if (const char* e = getenv("GPU_MAX_HW_QUEUES")) {
    const int v = atoi(e);
    if (v > 0) g_hw_queues_at_load = v;
  }
  setenv("GPU_MAX_HW_QUEUES", "32", 0);
}
int isl::hw_queues_at_load() { return g_hw_queues_at_load; }

extern "C" {

const char* isl_last_error_message(void) { return last_error().message.c_str(); }
uint64_t isl_last_error_expected(void) { return last_error().expected; }
uint64_t isl_last_error_actual(void) { return last_error().actual; }
uint64_t isl_last_error_node(void) { return last_error().node; }
uint32_t isl_abi_version(void) { return ISL_ABI_VERSION; }

const char* isl_status_name(isl_status s) {
  switch (s) {
    case ISL_OK: return "Ok";
    case ISL_ERR_DIMENSION_MISMATCH: return "DimensionMismatch";
    case ISL_ERR_EMPTY_COLLECTION: return "EmptyCollection";
    case ISL_ERR_INVALID_CONFIG: return "InvalidConfig";
    case ISL_ERR_INDEX_NOT_BUILT: return "IndexNotBuilt";
    case ISL_ERR_NODE_NOT_FOUND: return "NodeNotFound";
    case ISL_ERR_SERIALIZATION: return "Serialization";
    case ISL_ERR_DESERIALIZATION: return "Deserialization";
    case ISL_ERR_IO: return "Io";
    case ISL_ERR_HNSW: return "HnswError";
    case ISL_ERR_PQ: return "PQError";
    case ISL_ERR_SEARCH: return "SearchError";
    case ISL_ERR_EMBEDDING: return "EmbeddingError";
    case ISL_ERR_DEVICE: return "Device";
    case ISL_ERR_INVALID_ARGUMENT: return "InvalidArgument";
    case ISL_ERR_UNSUPPORTED: return "Unsupported";
    default: return "Unknown";
  }
}

int32_t isl_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  int ok = 0;
  for (int i = 0; i < n; i++) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, i) == hipSuccess &&
        strncmp(prop.gcnArchName, "gfx950", 6) == 0)
      ok++;
  }
  return ok;
}

// ---------------------------------------------------------------- LeannConfig
void isl_leann_config_paper_default(isl_leann_config* c) {  // leann.rs:386-403
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->m = 30;
  c->m0 = 60;
  c->ef_construction = 128;
  c->ml = 1.0 / std::log(30.0);
  c->max_layers = 16;
  c->metric = ISL_METRIC_COSINE;
  c->ef_search = 64;
  c->beam_width = 1;
  c->prune_ratio = 0.0f;
  c->pruning_strategy = ISL_PRUNE_GLOBAL;
  c->high_degree_pruning = 1;
  c->hub_percentile = 0.02f;
  c->is_compact = 1;
  c->is_recompute = 1;
}

void isl_leann_config_fast(isl_leann_config* c) {  // leann.rs:406-416
  if (!c) return;
  isl_leann_config_paper_default(c);
  c->m = 16;
  c->m0 = 32;
  c->ef_construction = 100;
  c->ef_search = 32;
  c->beam_width = 1;
  c->prune_ratio = 0.3f;
}

void isl_leann_config_accurate(isl_leann_config* c) {  // leann.rs:419-429
  if (!c) return;
  isl_leann_config_paper_default(c);
  c->m = 48;
  c->m0 = 96;
  c->ef_construction = 400;
  c->ef_search = 128;
  c->beam_width = 1;
  c->prune_ratio = 0.0f;
}

isl_status isl_leann_config_validate(const isl_leann_config* c) {  // leann.rs:432-460
  if (!c) return fail(ISL_ERR_INVALID_ARGUMENT, "config is NULL");
  if (c->m == 0) return fail(ISL_ERR_INVALID_CONFIG, "Invalid configuration: M must be > 0");
  if (c->m0 < c->m) return fail(ISL_ERR_INVALID_CONFIG, "Invalid configuration: M0 must be >= M");
  if (c->ef_construction < c->m)
    return fail(ISL_ERR_INVALID_CONFIG, "Invalid configuration: ef_construction must be >= M");
  if (c->prune_ratio < 0.0f || c->prune_ratio > 1.0f)
    return fail(ISL_ERR_INVALID_CONFIG, "Invalid configuration: prune_ratio must be in [0.0, 1.0]");
  if (c->beam_width == 0)
    return fail(ISL_ERR_INVALID_CONFIG, "Invalid configuration: beam_width must be > 0");
  if (c->hub_percentile < 0.0f || c->hub_percentile > 1.0f)
    return fail(ISL_ERR_INVALID_CONFIG,
                "Invalid configuration: hub_percentile must be in [0.0, 1.0]");
  if (c->metric > ISL_METRIC_MANHATTAN || c->pruning_strategy > ISL_PRUNE_PROPORTIONAL)
    return fail(ISL_ERR_INVALID_ARGUMENT, "metric / pruning_strategy out of range");
  return ISL_OK;
}

// ----------------------------------------------------------------- LeannIndex
isl_status isl_index_new(const isl_leann_config* cfg, isl_index** out) {  // leann.rs:504-511
  if (!out) return fail(ISL_ERR_INVALID_ARGUMENT, "out is NULL");
  isl_leann_config c;
  if (cfg) c = *cfg; else isl_leann_config_paper_default(&c);
  ISL_TRY(isl_leann_config_validate(&c));
  isl_index* idx = new (std::nothrow) isl_index();
  if (!idx) return fail(ISL_ERR_IO, "out of memory");
  idx->cfg = c;
  *out = idx;
  return ISL_OK;
}

isl_status isl_index_from_csr(const isl_leann_config* cfg, uint64_t num_nodes,
                              const uint64_t* node_offsets, const uint64_t* neighbors,
                              const uint64_t* levels, const uint64_t* degree_counts,
                              int32_t has_entry, uint64_t entry_point, uint64_t max_level,
                              int32_t has_dimension, uint64_t dimension, isl_index** out) {
  if (!out || (!node_offsets && num_nodes))
    return fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  isl_index* idx = nullptr;
  ISL_TRY(isl_index_new(cfg, &idx));
  idx->num_nodes = num_nodes;
  if (num_nodes) {
    idx->node_offsets.assign(node_offsets, node_offsets + num_nodes + 1);
    for (uint64_t i = 0; i < num_nodes; i++)
      if (idx->node_offsets[i + 1] < idx->node_offsets[i]) {
        delete idx;
        return fail(ISL_ERR_INVALID_ARGUMENT, "node_offsets must be non-decreasing");
      }
    uint64_t nnz = idx->node_offsets[num_nodes];
    if (nnz && !neighbors) {
      delete idx;
      return fail(ISL_ERR_INVALID_ARGUMENT, "neighbors is NULL");
    }
    idx->neighbors.assign(neighbors, neighbors + nnz);
    if (levels) idx->levels.assign(levels, levels + num_nodes);
    else idx->levels.assign(num_nodes, 0);
    if (degree_counts) idx->degree_counts.assign(degree_counts, degree_counts + num_nodes);
    else {
      idx->degree_counts.resize(num_nodes);
      for (uint64_t i = 0; i < num_nodes; i++)
        idx->degree_counts[i] = idx->node_offsets[i + 1] - idx->node_offsets[i];
    }
  }
  idx->has_entry = has_entry != 0;
  idx->entry_point = has_entry ? entry_point : 0;
  idx->max_level = max_level;
  idx->has_dimension = has_dimension != 0;
  idx->dimension = has_dimension ? dimension : 0;
  *out = idx;
  return ISL_OK;
}

void isl_index_free(isl_index* idx) {
  if (!idx) return;
  if (idx->device >= 0) {
    (void)hipSetDevice(idx->device);
    join_lane_workers(idx);
    if (idx->group) free_group_state(idx);  // (held calls go out first: their lanes are drained below)
    for (auto& w : idx->ws)
      if (w.busy && w.st_inflight) (void)hipStreamSynchronize(w.st_inflight);
    for (auto& w : idx->ws) free_workspace(w);  // (their events)
  }
  delete idx;  // every device array is a member that frees itself
}

uint64_t isl_index_len(const isl_index* idx) { return idx ? idx->num_nodes : 0; }
int32_t isl_index_is_empty(const isl_index* idx) { return !idx || idx->num_nodes == 0; }
int32_t isl_index_dimension(const isl_index* idx, uint64_t* dim) {
  if (!idx || !idx->has_dimension) return 0;
  if (dim) *dim = idx->dimension;
  return 1;
}
int32_t isl_index_is_recompute(const isl_index* idx) { return idx && idx->cfg.is_recompute; }
int32_t isl_index_is_compact(const isl_index* idx) { return idx && idx->cfg.is_compact; }
isl_status isl_index_config(const isl_index* idx, isl_leann_config* out) {
  if (!idx || !out) return fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  *out = idx->cfg;
  return ISL_OK;
}
int32_t isl_index_entry_point(const isl_index* idx, uint64_t* entry) {
  if (!idx || !idx->has_entry) return 0;
  if (entry) *entry = idx->entry_point;
  return 1;
}
uint64_t isl_index_max_level(const isl_index* idx) { return idx ? idx->max_level : 0; }

// CsrGraph::storage_bytes, leann.rs:296-301 (usize = u64 = 8 bytes each)
uint64_t isl_index_storage_bytes(const isl_index* idx) {
  if (!idx) return 0;
  if (materialise_host_csr(idx) != ISL_OK) return 0;
  return 8ull * (idx->node_offsets.size() + idx->neighbors.size() + idx->levels.size() +
                 idx->degree_counts.size());
}

int32_t isl_index_get_neighbors(const isl_index* idx, uint64_t node, const uint64_t** ptr,
                                size_t* len) {  // leann.rs:225-233
  if (!idx || !ptr || !len) return 0;
  if (node >= idx->num_nodes) return 0;
  if (materialise_host_csr(idx) != ISL_OK) return 0;
  uint64_t s = idx->node_offsets[node], e = idx->node_offsets[node + 1];
  *ptr = idx->neighbors.data() + s;
  *len = (size_t)(e - s);
  return 1;
}

// ------------------------------------------------------------------- bincode
// bincode 1.x default options: little-endian, fixed-width integers, usize as
// u64, Vec<T> = u64 length + items, Option<T> = u8 tag + payload, C-like enum =
// u32 variant index, bool = u8.  LeannIndex field order: config, graph,
// dimension (leann.rs:493-500).  The reference pins `bincode = "3.0.0"`
// (Cargo.toml:64) yet calls the 1.x free functions (leann.rs:1060,1065); the
// reference tests only round-trip (leann.rs:1347-1384) -> byte layout unpinned.
namespace {
struct Writer {
  std::vector<uint8_t> b;
  void raw(const void* p, size_t n) {
    const uint8_t* s = (const uint8_t*)p;
    b.insert(b.end(), s, s + n);
  }
  void u8(uint8_t v) { b.push_back(v); }
  void u32(uint32_t v) { raw(&v, 4); }
  void u64(uint64_t v) { raw(&v, 8); }
  void f32(float v) { raw(&v, 4); }
  void f64(double v) { raw(&v, 8); }
  void vec64(const std::vector<uint64_t>& v) {
    u64(v.size());
    raw(v.data(), v.size() * 8);
  }
};
struct Reader {
  const uint8_t* p;
  size_t n, off = 0;
  bool ok = true;
  bool take(void* dst, size_t k) {
    if (!ok || n - off < k) { ok = false; return false; }
    memcpy(dst, p + off, k);
    off += k;
    return true;
  }
  uint8_t u8() { uint8_t v = 0; take(&v, 1); return v; }
  uint32_t u32() { uint32_t v = 0; take(&v, 4); return v; }
  uint64_t u64() { uint64_t v = 0; take(&v, 8); return v; }
  float f32() { float v = 0; take(&v, 4); return v; }
  double f64() { double v = 0; take(&v, 8); return v; }
  bool vec64(std::vector<uint64_t>& v) {
    uint64_t len = u64();
    if (!ok || len > (n - off) / 8) { ok = false; return false; }
    v.resize(len);
    return take(v.data(), len * 8);
  }
};
}  // namespace

isl_status isl_index_to_bytes(const isl_index* idx, uint8_t** out, size_t* len) {  // leann.rs:1059
  if (!idx || !out || !len) return fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  ISL_TRY(materialise_host_csr(idx));
  Writer w;
  const isl_leann_config& c = idx->cfg;
  w.u64(c.m); w.u64(c.m0); w.u64(c.ef_construction); w.f64(c.ml); w.u64(c.max_layers);
  w.u32(c.metric); w.u64(c.ef_search); w.u64(c.beam_width); w.f32(c.prune_ratio);
  w.u32(c.pruning_strategy); w.u8(c.high_degree_pruning ? 1 : 0); w.f32(c.hub_percentile);
  w.u8(c.is_compact ? 1 : 0); w.u8(c.is_recompute ? 1 : 0);
  w.vec64(idx->node_offsets);
  w.vec64(idx->neighbors);
  w.vec64(idx->levels);
  if (idx->has_entry) { w.u8(1); w.u64(idx->entry_point); } else w.u8(0);
  w.u64(idx->max_level);
  w.u64(idx->num_nodes);
  w.vec64(idx->degree_counts);
  if (idx->has_dimension) { w.u8(1); w.u64(idx->dimension); } else w.u8(0);
  uint8_t* buf = (uint8_t*)malloc(w.b.size() ? w.b.size() : 1);
  if (!buf) return fail(ISL_ERR_SERIALIZATION, "Serialization error: out of memory");
  memcpy(buf, w.b.data(), w.b.size());
  *out = buf;
  *len = w.b.size();
  return ISL_OK;
}

void isl_free_bytes(uint8_t* p) { free(p); }

static isl_status index_from_bytes_impl(const uint8_t* bytes, size_t len, isl_index** out);

isl_status isl_index_from_bytes(const uint8_t* bytes, size_t len, isl_index** out) {  // leann.rs:1064
  if (!bytes || !out) return fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  // lengths inside the buffer are untrusted: nothing may throw across the C boundary
  try {
    return index_from_bytes_impl(bytes, len, out);
  } catch (const std::exception& e) {
    return fail(ISL_ERR_DESERIALIZATION, "Deserialization error: %s", e.what());
  }
}

static isl_status index_from_bytes_impl(const uint8_t* bytes, size_t len, isl_index** out) {
  Reader r{bytes, len};
  isl_index* idx = new (std::nothrow) isl_index();
  if (!idx) return fail(ISL_ERR_IO, "out of memory");
  isl_leann_config& c = idx->cfg;
  c.m = r.u64(); c.m0 = r.u64(); c.ef_construction = r.u64(); c.ml = r.f64();
  c.max_layers = r.u64(); c.metric = r.u32(); c.ef_search = r.u64(); c.beam_width = r.u64();
  c.prune_ratio = r.f32(); c.pruning_strategy = r.u32(); c.high_degree_pruning = r.u8();
  c.hub_percentile = r.f32(); c.is_compact = r.u8(); c.is_recompute = r.u8();
  bool enum_ok = c.metric <= ISL_METRIC_MANHATTAN && c.pruning_strategy <= ISL_PRUNE_PROPORTIONAL &&
                 c.high_degree_pruning <= 1 && c.is_compact <= 1 && c.is_recompute <= 1;
  r.vec64(idx->node_offsets);
  r.vec64(idx->neighbors);
  r.vec64(idx->levels);
  uint8_t tag = r.u8();
  if (tag == 1) { idx->has_entry = true; idx->entry_point = r.u64(); }
  else if (tag != 0) enum_ok = false;
  idx->max_level = r.u64();
  idx->num_nodes = r.u64();
  r.vec64(idx->degree_counts);
  uint8_t dtag = r.u8();
  if (dtag == 1) { idx->has_dimension = true; idx->dimension = r.u64(); }
  else if (dtag != 0) enum_ok = false;
  if (!r.ok || !enum_ok) {
    delete idx;
    return fail(ISL_ERR_DESERIALIZATION, "Deserialization error: %s",
                r.ok ? "invalid enum/option tag" : "unexpected end of input");
  }
  // bincode itself accepts trailing bytes with deserialize(); structural sanity below is
  // ours: get_neighbors (leann.rs:230-232) would index out of bounds otherwise.
  // (num_nodes is untrusted: num_nodes + 1 must not wrap before it is compared)
  if (idx->num_nodes >= (1ull << 61) || idx->node_offsets.size() != idx->num_nodes + 1 ||
      (idx->num_nodes && idx->node_offsets[idx->num_nodes] > idx->neighbors.size())) {
    delete idx;
    return fail(ISL_ERR_DESERIALIZATION,
                "Deserialization error: node_offsets inconsistent with num_nodes/neighbors");
  }
  for (uint64_t i = 0; i < idx->num_nodes; i++)
    if (idx->node_offsets[i + 1] < idx->node_offsets[i]) {
      delete idx;
      return fail(ISL_ERR_DESERIALIZATION, "Deserialization error: node_offsets not monotonic");
    }
  *out = idx;
  return ISL_OK;
}

}  // extern "C"

// ------------------------------------------------------------ device upload
namespace {

constexpr uint32_t kMaxDeviceId = 0x7FFFFFF0u;  // ids above this cannot carry the flag bit

__global__ void convert_adj_kernel(const uint64_t* __restrict__ in, uint32_t* __restrict__ out,
                                   uint64_t n, uint32_t* __restrict__ flags) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (; i < n; i += stride) {
    uint64_t v = in[i];
    if (v > kMaxDeviceId) { bad = true; v = kMaxDeviceId; }
    out[i] = (uint32_t)v;
  }
  if (bad) atomicOr(flags, 1u);
}

// bf16 bit patterns -> their exact f32 images
__global__ void widen_bf16_kernel(const uint16_t* __restrict__ src, uint64_t sstride, uint32_t d, uint64_t n,
                                  float* __restrict__ dst, uint64_t dstride) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * d) return;
  const uint64_t r = i / d, c = i % d;
  dst[r * dstride + c] = __uint_as_float((uint32_t)src[r * sstride + c] << 16);
}

// fp8 e4m3 codes -> their exact f32 images e4m3(c) * scale (scale = 2^scale_exp of the table)
__global__ void widen_fp8_kernel(const uint8_t* __restrict__ src, uint64_t sstride, uint32_t d, uint64_t n,
                                 float scale, float* __restrict__ dst, uint64_t dstride) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * d) return;
  const uint64_t r = i / d, c = i % d;
  dst[r * dstride + c] = isl_dev::fp8_image(src[r * sstride + c], scale);
}

// norm2[i] = sum_j rows[i][j]^2, sequential in j (one lane per row, rows staged through LDS).
__global__ __launch_bounds__(64) void row_norm2_kernel(const float* __restrict__ rows, uint64_t n,
                                                       uint32_t d, uint64_t stride,
                                                       float* __restrict__ norm2) {
  extern __shared__ __align__(16) unsigned char smem[];
  float* tile = reinterpret_cast<float*>(smem);
  const int lane = threadIdx.x;
  for (uint64_t base = (uint64_t)blockIdx.x * 64; base < n; base += (uint64_t)gridDim.x * 64) {
    uint32_t R = (uint32_t)(n - base < 64 ? n - base : 64);
    // the query operand is ignored by SUMSQ_RAW; `tile` only serves as a valid LDS address
    float v = isl_dev::wave_distances<isl_dev::METRIC_SUMSQ_RAW>(rows + base * stride, stride, d,
                                                                  (uint32_t)lane, R, tile, tile, 0.f);
    if ((uint32_t)lane < R) norm2[base + lane] = v;
  }
}

// One thread per row: max degree, duplicate ids within a row (flag bit 1).
__global__ void row_stats_kernel(const uint64_t* __restrict__ off, const uint32_t* __restrict__ adj,
                                 uint64_t num_nodes, uint32_t* __restrict__ flags,
                                 uint32_t* __restrict__ max_degree) {
  uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= num_nodes) return;
  uint64_t s = off[row], e = off[row + 1];
  uint64_t deg = e - s;
  atomicMax(max_degree, (uint32_t)(deg > 0xFFFFFFFFull ? 0xFFFFFFFFu : deg));
  if (deg > 4096) { atomicOr(flags, 4u); return; }  // checked on the host instead
  bool dup = false;
  for (uint64_t i = s + 1; i < e && !dup; i++) {
    uint32_t v = adj[i];
    for (uint64_t j = s; j < i; j++)
      if (adj[j] == v) { dup = true; break; }
  }
  if (dup) atomicOr(flags, 2u);
}

}  // namespace

namespace isl {

isl_status materialise_host_csr(const isl_index* cidx) {
  isl_index* idx = const_cast<isl_index*>(cidx);
  if (idx->host_csr_valid) return ISL_OK;
  std::lock_guard<std::mutex> lock(idx->mu);
  if (idx->host_csr_valid) return ISL_OK;
  ISL_TRY(use_device(idx->device));
  idx->node_offsets.resize(idx->num_nodes + 1);
  ISL_HIP(hipMemcpy(idx->node_offsets.data(), idx->d_off, (idx->num_nodes + 1) * 8,
                    hipMemcpyDeviceToHost));
  std::vector<uint32_t> tmp(idx->nnz);
  if (idx->nnz)
    ISL_HIP(hipMemcpy(tmp.data(), idx->d_adj, idx->nnz * 4, hipMemcpyDeviceToHost));
  idx->neighbors.assign(tmp.begin(), tmp.end());
  if (idx->levels.size() != idx->num_nodes) idx->levels.assign(idx->num_nodes, 0);
  idx->degree_counts.resize(idx->num_nodes);
  for (uint64_t i = 0; i < idx->num_nodes; i++)
    idx->degree_counts[i] = idx->node_offsets[i + 1] - idx->node_offsets[i];
  idx->host_csr_valid = true;
  return ISL_OK;
}

static isl_status scan_device_csr(isl_index* idx, const uint64_t* d_off, const uint32_t* d_adj, uint32_t* d_flags,
                                  uint32_t* flags_out) {
  uint32_t* d_maxdeg = d_flags + 1;
  if (idx->num_nodes) {
    uint32_t blocks = (uint32_t)((idx->num_nodes + 255) / 256);
    hipLaunchKernelGGL(row_stats_kernel, dim3(blocks), dim3(256), 0, 0, d_off, d_adj, idx->num_nodes, d_flags,
                       d_maxdeg);
    ISL_HIP(hipGetLastError());
  }
  uint32_t host[2] = {0, 0};
  ISL_HIP(hipMemcpy(host, d_flags, 8, hipMemcpyDeviceToHost));
  *flags_out = host[0];
  idx->max_degree = host[1];
  return ISL_OK;
}

}  // namespace isl

extern "C" {

isl_status isl_index_upload(isl_index* idx, int32_t device) {
  if (!idx) return fail(ISL_ERR_INVALID_ARGUMENT, "index is NULL");
  ISL_TRY(use_device(device));
  std::lock_guard<std::mutex> lock(idx->mu);
  if (idx->device >= 0 && idx->device != device)
    return fail(ISL_ERR_UNSUPPORTED, "index already resident on device %d", idx->device);
  if (idx->d_off) return ISL_OK;  // already uploaded
  if (!idx->host_csr_valid) return fail(ISL_ERR_INVALID_ARGUMENT, "no host CSR to upload");
  idx->seeds = {};  // a table belongs to the rows of one residency
  if (idx->num_nodes >= kMaxDeviceId)
    return fail(ISL_ERR_UNSUPPORTED, "num_nodes %llu exceeds the device id range",
                (unsigned long long)idx->num_nodes);
  uint64_t nnz = idx->num_nodes ? idx->node_offsets[idx->num_nodes] : 0;

  // Duplicate ids inside one adjacency row are always "already visited" at their
  // second occurrence (visited.insert, leann.rs:933-937), so the device copy keeps
  // only the first occurrence; the host CSR is left untouched.
  std::vector<uint64_t> off = idx->node_offsets;
  const uint64_t* nb_src = idx->neighbors.data();
  std::vector<uint64_t> dedup;

  // the copy joins the handle only once it is complete: a failed upload leaves the index not uploaded
  DeviceBuffer<uint64_t> d_off;
  DeviceBuffer<uint32_t> d_adj, d_flags;
  ISL_TRY(d_flags.reserve(4));
  for (int pass = 0; pass < 2; pass++) {
    ISL_HIP(hipMemset(d_flags, 0, 16));
    ISL_TRY(d_off.reserve(idx->num_nodes + 1));
    ISL_HIP(hipMemcpy(d_off, off.data(), (idx->num_nodes + 1) * 8, hipMemcpyHostToDevice));
    ISL_TRY(d_adj.reserve(nnz ? nnz : 1));
    if (nnz) {
      DeviceBuffer<uint64_t> d_tmp;
      ISL_TRY(d_tmp.reserve(nnz));
      ISL_HIP(hipMemcpy(d_tmp, nb_src, nnz * 8, hipMemcpyHostToDevice));
      hipLaunchKernelGGL(convert_adj_kernel, dim3(2048), dim3(256), 0, 0, d_tmp.get(), d_adj.get(), nnz,
                         d_flags.get());
      ISL_HIP(hipGetLastError());
      ISL_HIP(hipDeviceSynchronize());
    }
    uint32_t flags = 0;
    ISL_TRY(scan_device_csr(idx, d_off, d_adj, d_flags, &flags));
    if (flags & 1u)
      return fail(ISL_ERR_UNSUPPORTED, "neighbour ids above 0x%x are not representable on device",
                  kMaxDeviceId);
    if (!(flags & 6u) || pass == 1) break;
    // rebuild without in-row duplicates on the host, then upload again
    d_off.reset();
    d_adj.reset();
    dedup.clear();
    dedup.reserve(nnz);
    std::vector<uint64_t> row;
    for (uint64_t i = 0; i < idx->num_nodes; i++) {
      uint64_t s = idx->node_offsets[i], e = idx->node_offsets[i + 1];
      row.assign(idx->neighbors.begin() + s, idx->neighbors.begin() + e);
      std::vector<uint64_t> sorted = row;
      std::sort(sorted.begin(), sorted.end());
      bool has_dup = std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end();
      off[i] = dedup.size();
      if (!has_dup) {
        dedup.insert(dedup.end(), row.begin(), row.end());
      } else {
        size_t base = dedup.size();
        for (uint64_t v : row) {
          bool seen = false;
          for (size_t j = base; j < dedup.size(); j++)
            if (dedup[j] == v) { seen = true; break; }
          if (!seen) dedup.push_back(v);
        }
      }
    }
    off[idx->num_nodes] = dedup.size();
    nnz = dedup.size();
    nb_src = dedup.data();
  }
  idx->d_off = std::move(d_off);
  idx->d_adj = std::move(d_adj);
  idx->nnz = nnz;
  idx->device = device;
  return ensure_padded_adjacency(idx);
}

isl_status isl_index_from_device_csr(const isl_leann_config* cfg, int32_t device,
                                     uint64_t num_nodes, const uint64_t* d_node_offsets,
                                     const uint32_t* d_neighbors, int32_t has_entry,
                                     uint64_t entry_point, int32_t has_dimension,
                                     uint64_t dimension, isl_index** out) {
  if (!out || !d_node_offsets) return fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  ISL_TRY(use_device(device));
  if (num_nodes >= kMaxDeviceId)
    return fail(ISL_ERR_UNSUPPORTED, "num_nodes exceeds the device id range");
  isl_index* idx = nullptr;
  ISL_TRY(isl_index_new(cfg, &idx));
  idx->host_csr_valid = false;
  idx->node_offsets.clear();
  idx->num_nodes = num_nodes;
  idx->has_entry = has_entry != 0;
  idx->entry_point = has_entry ? entry_point : 0;
  idx->has_dimension = has_dimension != 0;
  idx->dimension = has_dimension ? dimension : 0;
  idx->device = device;
  auto bail = [&](isl_status st) { isl_index_free(idx); return st; };
  uint64_t nnz = 0;
  if (hipMemcpy(&nnz, d_node_offsets + num_nodes, 8, hipMemcpyDeviceToHost) != hipSuccess)
    return bail(fail(ISL_ERR_DEVICE, "cannot read node_offsets[num_nodes] from the device"));
  idx->nnz = nnz;
  if (idx->d_off.reserve(num_nodes + 1) != ISL_OK || idx->d_adj.reserve(nnz ? nnz : 1) != ISL_OK)
    return bail(fail(ISL_ERR_DEVICE, "hipMalloc failed for the CSR copy"));
  if (hipMemcpy(idx->d_off, d_node_offsets, (num_nodes + 1) * 8, hipMemcpyDeviceToDevice) !=
          hipSuccess ||
      (nnz && hipMemcpy(idx->d_adj, d_neighbors, nnz * 4, hipMemcpyDeviceToDevice) != hipSuccess))
    return bail(fail(ISL_ERR_DEVICE, "device copy of the CSR failed"));
  DeviceBuffer<uint32_t> d_flags;
  if (d_flags.reserve(4) != ISL_OK || hipMemset(d_flags, 0, 16) != hipSuccess)
    return bail(fail(ISL_ERR_DEVICE, "hipMalloc failed"));
  uint32_t flags = 0;
  isl_status st = scan_device_csr(idx, idx->d_off, idx->d_adj, d_flags, &flags);
  if (st != ISL_OK) return bail(st);
  if (flags & 6u)
    return bail(fail(ISL_ERR_UNSUPPORTED,
                     "device-born CSR rows must not repeat a neighbour id (or exceed 4096 ids)"));
  if ((st = ensure_padded_adjacency(idx)) != ISL_OK) return bail(st);
  *out = idx;
  return ISL_OK;
}

}  // extern "C"

// norm_b of cosine_distance (distance.rs:79) depends on the row alone: computed once, in the reference's
// left-to-right order, and reused by every search
static void launch_row_norm2(const float* rows, uint64_t cnt, uint64_t d, uint64_t stride, float* norm2) {
  using namespace isl_dev;
  const size_t lds = (size_t)TILE_ROWS * TILE_LD * 4 + 64;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((cnt + 63) / 64, 8192);
  hipLaunchKernelGGL(row_norm2_kernel, dim3(grid), dim3(64), lds, 0, rows, cnt, (uint32_t)d, stride, norm2);
}

isl_status isl::RowTable::fill(uint64_t first, uint64_t count, const void* src, int32_t mem) {
  const uint64_t es = isl_rows::elem_size(dtype_), d = d_, stride = stride_;
  unsigned char* at = block_ + first * stride * es;
  const uint64_t slack = isl_rows::fill_tail_elems(dtype_, capacity_, first, count);
  if (stride != d) ISL_HIP(hipMemset(at, 0, (size_t)((count * stride + slack) * es)));
  else if (slack) ISL_HIP(hipMemset(at + count * stride * es, 0, (size_t)(slack * es)));
  const hipMemcpyKind kind = mem == ISL_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (stride == d) ISL_HIP(hipMemcpy(at, src, (size_t)(count * d * es), kind));
  else ISL_HIP(hipMemcpy2D(at, stride * es, src, d * es, d * es, count, kind));
  return norms(first, count);
}

isl_status isl::RowTable::norms(uint64_t first, uint64_t count) {
  const uint64_t d = d_, stride = stride_;
  if (dtype_ == ISL_DTYPE_F32) {
    launch_row_norm2(f32() + first * stride, count, d, stride, norm2_ + first);
  } else {
    // bf16 rows are bit patterns, fp8 rows codes, and the provider's vectors their exact f32 images: widen a
    // chunk of rows to f32 and reuse the f32 kernel
    const uint64_t stride32 = isl_rows::stride(ISL_DTYPE_F32, d), chunk = isl_rows::norm_chunk_rows(count, d);
    DeviceBuffer<float> tmp;
    ISL_TRY(tmp.reserve(isl_rows::norm_chunk_floats(chunk, d)));
    ISL_HIP(hipMemset(tmp, 0, (size_t)isl_rows::norm_chunk_floats(chunk, d) * 4));
    for (uint64_t o = 0; o < count; o += chunk) {
      const uint64_t c = std::min(chunk, count - o);
      const dim3 wgrid((uint32_t)((c * d + 255) / 256));
      if (is_fp8())
        hipLaunchKernelGGL(widen_fp8_kernel, wgrid, dim3(256), 0, 0, fp8() + (first + o) * stride, stride, (uint32_t)d, c,
                           std::ldexp(1.0f, scale_exp_), tmp.get(), stride32);
      else
        hipLaunchKernelGGL(widen_bf16_kernel, wgrid, dim3(256), 0, 0, bf16() + (first + o) * stride, stride, (uint32_t)d,
                           c, tmp.get(), stride32);
      launch_row_norm2(tmp, c, d, stride32, norm2_ + first + o);
    }
  }
  ISL_HIP(hipGetLastError());
  ISL_HIP(hipDeviceSynchronize());  // (also: tmp goes when this returns)
  return ISL_OK;
}

isl_status isl::RowTable::zero() {
  return zero_from(0);
}

isl_status isl::RowTable::zero_from(uint64_t first) {
  const uint64_t es = isl_rows::elem_size(dtype_);
  ISL_HIP(hipMemset(block_ + first * stride_ * es, 0, (size_t)(isl_rows::tail_elems(dtype_, capacity_, d_, first) * es)));
  if (capacity_ > first) ISL_HIP(hipMemset(norm2_ + first, 0, (size_t)(capacity_ - first) * 4));
  return ISL_OK;
}

// InMemoryEmbeddingProvider::new, leann.rs:111-120, over rows of any stored type (scale_exp: fp8 rows only)
static isl_status set_embeddings(isl_index* idx, const void* rows, uint64_t n, uint64_t d, int32_t dtype,
                                 int32_t scale_exp, int32_t mem) {
  if (!idx || (!rows && n)) return fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  if (n == 0) return fail(ISL_ERR_EMPTY_COLLECTION, "Empty vector collection");
  if (dtype != ISL_DTYPE_F32 && dtype != ISL_DTYPE_BF16 && dtype != ISL_DTYPE_FP8_E4M3)
    return fail(ISL_ERR_INVALID_ARGUMENT, "unknown row dtype");
  if (scale_exp < isl_rows::kMinScaleExp || scale_exp > isl_rows::kMaxScaleExp)
    return fail(ISL_ERR_INVALID_ARGUMENT, "fp8 rows: scale_exp = %d is outside [%d, %d]", scale_exp, isl_rows::kMinScaleExp,
                isl_rows::kMaxScaleExp);
  if (d == 0 || d > 65536) return fail(ISL_ERR_INVALID_ARGUMENT, "dimension out of range");
  if (idx->device < 0)
    return fail(ISL_ERR_DEVICE, "call isl_index_upload before attaching embeddings");
  ISL_TRY(use_device(idx->device));
  std::lock_guard<std::mutex> lock(idx->mu);
  if (any_lane_busy(idx))  // their kernels read the tables freed below
    return fail(ISL_ERR_SEARCH, "Search error: the embedding provider cannot be swapped while searches are in flight");
  if (dtype != ISL_DTYPE_F32 && idx->is_hnsw) return fail(ISL_ERR_UNSUPPORTED, "the HnswGraph facade keeps f32 vectors");
  // every check is above: from here on the old provider goes
  idx->seeds = {};  // copies of rows that are about to go
  free_exact_pool(idx->pool);  // sized by the row count: rebuilt by the next prepare / search
  idx->recompute = false;  // back to the in-memory provider
  ISL_TRY(idx->rows.allocate(dtype, n, d));  // (a reservation goes with the table it was made for)
  ++idx->row_allocations;
  idx->rows.set_scale_exp(dtype == ISL_DTYPE_FP8_E4M3 ? scale_exp : 0);  // (before the fill: the norms are the images')
  idx->nvec = n;
  return idx->rows.fill(0, n, rows, mem);
}

extern "C" {

isl_status isl_set_embeddings(isl_index* idx, const void* rows, uint64_t n, uint64_t d,
                              int32_t dtype, int32_t mem) {
  return set_embeddings(idx, rows, n, d, dtype, 0, mem);
}

isl_status isl_set_embeddings_fp8(isl_index* idx, const void* codes, uint64_t n, uint64_t d, int32_t scale_exp,
                                  int32_t mem) {
  return set_embeddings(idx, codes, n, d, ISL_DTYPE_FP8_E4M3, scale_exp, mem);
}

isl_status isl_index_row_storage(const isl_index* idx, int32_t* dtype, int32_t* scale_exp, uint64_t* block_bytes) {
  if (!idx) return fail(ISL_ERR_INVALID_ARGUMENT, "index is NULL");
  std::lock_guard<std::mutex> lock(idx->mu);
  const RowTable& t = idx->rows;
  const bool held = t.resident() && !idx->recompute;
  // (type and scale are those of the rows stored: a reserved table that holds none, before its first insert or after
  // the last row left, answers here as a handle without rows does)
  const bool stored = held && t.n() > 0;
  if (dtype) *dtype = stored ? t.dtype() : ISL_DTYPE_F32;
  if (scale_exp) *scale_exp = stored ? t.scale_exp() : 0;
  if (block_bytes) *block_bytes = held ? t.block_bytes() : 0;
  return ISL_OK;
}

isl_status isl_index_capacity(const isl_index* idx, uint64_t* capacity_rows, uint64_t* row_allocations) {
  if (!idx) return fail(ISL_ERR_INVALID_ARGUMENT, "index is NULL");
  std::lock_guard<std::mutex> lock(idx->mu);
  const bool held = idx->rows.resident() && !idx->recompute;
  if (capacity_rows) *capacity_rows = held ? idx->rows.capacity() : 0;
  if (row_allocations) *row_allocations = idx->row_allocations;
  return ISL_OK;
}

isl_status isl_index_reserve(isl_index* idx, uint64_t capacity, uint64_t d, int32_t dtype) {
  static const char* who = "isl_index_reserve";
  if (!idx) return fail(ISL_ERR_INVALID_ARGUMENT, "index is NULL");
  if (dtype != ISL_DTYPE_F32 && dtype != ISL_DTYPE_BF16 && dtype != ISL_DTYPE_FP8_E4M3)
    return fail(ISL_ERR_INVALID_ARGUMENT, "unknown row dtype");
  if (idx->is_hnsw)
    return fail(ISL_ERR_UNSUPPORTED, "%s: this is the core index of an HnswGraph, whose rows are not reserved", who);
  if (idx->recompute)
    return fail(ISL_ERR_UNSUPPORTED, "%s: an index on the recompute provider stores no rows", who);
  const uint64_t n0 = idx->num_nodes;
  const RowTable& old = idx->rows;
  if (n0 && (idx->device < 0 || !old.resident() || !old.norm2() || old.n() != n0 || idx->nvec != n0))
    return fail(ISL_ERR_UNSUPPORTED, "%s needs the index's rows resident on the device (isl_index_upload, "
                "isl_set_embeddings)", who);
  if (!n0 && d == 0) return fail(ISL_ERR_EMPTY_COLLECTION, "Empty vector collection");
  if (capacity >= kMaxDeviceId)
    return fail(ISL_ERR_UNSUPPORTED, "%s: a capacity of %llu rows exceeds the device id range", who,
                (unsigned long long)capacity);
  if (n0) {
    if (old.d() != d) return fail_dim(old.d(), d);
    if (old.dtype() != dtype)
      return fail(ISL_ERR_UNSUPPORTED, "%s: the index stores %s rows and reserves no other type", who,
                  old.is_fp8() ? "fp8" : old.is_bf16() ? "bf16" : "float32");
  } else {
    if (d > 65536) return fail(ISL_ERR_INVALID_ARGUMENT, "dimension out of range");
    if (dtype == ISL_DTYPE_FP8_E4M3)
      return fail(ISL_ERR_UNSUPPORTED, "%s: an empty index takes its rows through isl_index_insert, which takes no fp8 rows",
                  who);
    if (idx->has_dimension && idx->dimension != d) return fail_dim(idx->dimension, d);
  }
  capacity = std::max(capacity, n0);
  const bool same_shape = old.resident() && old.d() == d && old.dtype() == dtype;
  {  // the block's address changes: not beside a search on the same handle
    std::lock_guard<std::mutex> lock(idx->mu);
    if (any_lane_busy(idx))
      return fail(ISL_ERR_SEARCH, "Search error: rows cannot be reserved while searches are in flight");
    if (same_shape && capacity <= old.capacity()) return ISL_OK;  // a reservation never shrinks
  }
  // (an empty handle: where isl_index_insert would put the rows)
  const int32_t device = idx->device >= 0 ? idx->device : 0;
  ISL_TRY(use_device(device));
  // the new table beside the old one, which nothing below writes: the one copy a reservation costs
  RowTable fresh;
  if (fresh.allocate(dtype, n0, d, capacity, true) != ISL_OK)
    return fail(ISL_ERR_DEVICE, "%s: hipMalloc failed for %llu rows", who, (unsigned long long)capacity);
  fresh.set_scale_exp(n0 ? old.scale_exp() : 0);
  if (n0) {
    ISL_HIP(hipMemcpy(fresh.as<unsigned char>(), old.data(), (size_t)(n0 * old.stride() * isl_rows::elem_size(dtype)),
                      hipMemcpyDeviceToDevice));
    ISL_HIP(hipMemcpy(fresh.norm2(), old.norm2(), (size_t)n0 * 4, hipMemcpyDeviceToDevice));
  }
  ISL_TRY(fresh.zero_from(n0));
  ISL_HIP(hipDeviceSynchronize());
  std::lock_guard<std::mutex> lock(idx->mu);
  if (any_lane_busy(idx))
    return fail(ISL_ERR_SEARCH, "Search error: rows cannot be reserved while searches are in flight");
  idx->rows = std::move(fresh);
  ++idx->row_allocations;
  idx->device = device;
  return ISL_OK;
}

// (re)allocates the recompute provider's row cache: slot map, owners and, last, the slab of `rows` rows of d
// floats with its per-slot norms -- idx->rows holds slots only once everything beside them is there
static isl_status alloc_recompute_cache(isl_index* idx, uint64_t rows, uint64_t d) {
  // the old cache goes before the new one is allocated: the slab may be most of the card
  idx->rows.reset(); idx->d_slot_of.reset();
  idx->d_owner.reset(); idx->d_stamp.reset(); idx->d_slab_head.reset();
  // a block of `count` elements, every byte `fill`
  auto fresh = [](auto& buf, uint64_t count, int fill) -> isl_status {
    ISL_TRY(buf.reserve(count));
    ISL_HIP(hipMemset(buf, fill, count * sizeof(*buf.get())));
    return ISL_OK;
  };
  ISL_TRY(fresh(idx->d_slot_of, idx->nvec + 1, 0xFF));
  ISL_TRY(fresh(idx->d_owner, rows, 0xFF));
  ISL_TRY(fresh(idx->d_stamp, rows, 0));
  ISL_TRY(fresh(idx->d_slab_head, 2, 0));  // [0] clock hand, [1] slots used so far
  ISL_TRY(idx->rows.allocate(ISL_DTYPE_F32, rows, d));
  ++idx->row_allocations;
  return idx->rows.zero();
}

isl_status isl_index_set_recompute_cache_rows(isl_index* idx, uint64_t rows) {
  if (!idx) return fail(ISL_ERR_INVALID_ARGUMENT, "index is NULL");
  if (!idx->recompute) return fail(ISL_ERR_INVALID_ARGUMENT, "the index has no recompute provider");
  ISL_TRY(use_device(idx->device));
  std::lock_guard<std::mutex> lock(idx->mu);
  if (any_lane_busy(idx))
    return fail(ISL_ERR_SEARCH, "Search error: the row cache cannot be resized while searches are in flight");
  // a hop of one query needs up to 128 rows at once (plus the entry point): that is the floor
  rows = std::min<uint64_t>(idx->nvec, std::max<uint64_t>(rows, 256));
  return alloc_recompute_cache(idx, rows, idx->enc->cfg.hidden);
}

uint64_t isl_index_recompute_cache_bytes(const isl_index* idx) {
  if (!idx || !idx->recompute) return 0;
  return isl_rows::recompute_cache_bytes(idx->rows.n(), idx->rows.d(), idx->nvec);
}

// EmbeddingProvider backed by the encoder (recompute mode), see islands_amd.h.
isl_status isl_set_recompute_provider(isl_index* idx, isl_encoder* enc, const uint16_t* tokens,
                                      const uint16_t* lengths, uint64_t n, uint64_t L,
                                      int32_t normalize, int32_t keep_rows, int32_t mem) {
  if (!idx || !enc || (!tokens && n)) return fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  if (n == 0) return fail(ISL_ERR_EMPTY_COLLECTION, "Empty vector collection");
  if (idx->device < 0) return fail(ISL_ERR_DEVICE, "call isl_index_upload before attaching a provider");
  if (enc->device != idx->device) return fail(ISL_ERR_INVALID_ARGUMENT, "encoder and index live on different devices");
  if (idx->is_hnsw) return fail(ISL_ERR_UNSUPPORTED, "the HnswGraph facade stores its vectors (hnsw.rs:97-112)");
  if (L == 0 || L > enc->cfg.max_position)
    return fail(ISL_ERR_EMBEDDING, "Embedding error: %llu token slots per node, the model takes 1..%u",
                (unsigned long long)L, enc->cfg.max_position);
  if (n > 0x7FFFFFF0ull) return fail(ISL_ERR_UNSUPPORTED, "node ids above the device id range");
  ISL_TRY(use_device(idx->device));
  std::lock_guard<std::mutex> lock(idx->mu);
  if (any_lane_busy(idx))
    return fail(ISL_ERR_SEARCH, "Search error: the embedding provider cannot be swapped while searches are in flight");
  idx->seeds = {};  // the seeds' rows were the old provider's
  const uint64_t d = enc->cfg.hidden;
  idx->d_tokens.reset();
  idx->d_lens.reset();
  free_exact_pool(idx->pool);
  idx->recompute = false;
  // Recompute mode does not store embeddings (leann.rs:366-371): what is resident is the token
  // table plus a BOUNDED row cache -- a slab of rows.n() rows, 4 bytes of slot map per node.  The
  // default slab (2^20 rows, or every node of a smaller index) holds what a batch of a thousand
  // queries visits; isl_index_set_recompute_cache_rows changes it.
  idx->nvec = n;
  ISL_TRY(alloc_recompute_cache(idx, std::min<uint64_t>(n, 1ull << 20), d));
  hipMemcpyKind kind = mem == ISL_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  ISL_TRY(idx->d_tokens.reserve(n * L));
  ISL_HIP(hipMemcpy(idx->d_tokens, tokens, (size_t)n * L * 2, kind));
  if (lengths) {
    ISL_TRY(idx->d_lens.reserve(n));
    ISL_HIP(hipMemcpy(idx->d_lens, lengths, (size_t)n * 2, kind));
  }
  idx->enc = enc;
  idx->tok_L = (uint32_t)L;
  idx->enc_normalize = normalize;
  idx->keep_rows = keep_rows != 0;
  idx->recompute = true;
  idx->cfg.is_recompute = 1;
  if (!idx->has_dimension) { idx->has_dimension = true; idx->dimension = d; }
  return ISL_OK;
}

}  // extern "C"

// The in-memory provider of a graph that grows (Scaffold::open over rows from two sources): one table of
// old's rows + n_new of old's stored type, the first of them copied on the device from `old` together with their
// norms (a row's norm is a function of the row alone: the copied value is the bits a recomputation would give),
// the rest taken from `rows` as isl_set_embeddings takes them (RowTable::fill).  `idx` is a fresh construction graph.
isl_status isl::set_grown_embeddings(isl_index* idx, const isl_index* old, const void* rows, int32_t dtype,
                                     uint64_t n_new, uint64_t d, int32_t mem) {
  const RowTable& o = old->rows;
  const uint64_t n0 = o.n(), n = n0 + n_new;
  if (!o.resident() || !o.norm2() || o.d() != d || o.dtype() != dtype)
    return fail(ISL_ERR_UNSUPPORTED, "the graph's rows are not resident rows of this type and dimension");
  ISL_TRY(use_device(idx->device));
  std::lock_guard<std::mutex> lock(idx->mu);
  ISL_TRY(idx->rows.allocate(dtype, n, d));
  ISL_HIP(hipMemcpy(idx->rows.as<unsigned char>(), o.data(), (size_t)(n0 * o.stride() * isl_rows::elem_size(dtype)),
                    hipMemcpyDeviceToDevice));
  ISL_HIP(hipMemcpy(idx->rows.norm2(), o.norm2(), (size_t)n0 * 4, hipMemcpyDeviceToDevice));
  idx->nvec = n;
  return idx->rows.fill(n0, n_new, rows, mem);
}
