// Refined search: a second, wider row table beside the provider's rows, and the kernel that re-scores the
// candidates of a search against it.
//   table      isl_index_set_refine_rows: f32 or bf16 rows in a device row table, or in one pinned, device-mapped
//              host block of the same layout that the kernel reads across the bus; the norms are on the device
//   rescoring  one wave per query: the query in LDS, the candidates 64 at a time through direct_distances (the
//              chain of the search kernel, dterm / dfinish; this unit is built -ffp-contract=off), then a
//              rank-by-counting pass over (ordkey << 32 | position) keys -- no sort network, no atomics, and the
//              answer does not depend on the order of execution
//   refined    isl_search_batch_device with k = candidates into scratch of the handle's, then the rescoring on
//              the same stream
// The host-only arithmetic and the argument checks are search_refine_plan.hpp's.
#include "device_common.hip.h"
#include "search_refine_plan.hpp"

#include <algorithm>
#include <cstring>
#include <type_traits>

namespace {

using namespace isl_dev;
using isl::fail;

struct RescoreParams {
  const float* queries;        // [nq][d]
  const void* rows;            // the refine table, [n][stride] of its row type (device memory or mapped host memory)
  const float* norm2;          // [n], device memory
  uint64_t stride, n;
  uint32_t d, pitch, k;
  const uint64_t* cand;        // [nq][pitch]
  const uint32_t* cand_count;  // [nq]
  uint64_t* out_ids;           // [nq][k]
  float* out_dist;             // [nq][k]
  uint32_t* out_count;         // [nq]
};

constexpr unsigned long long kNoKey = ~0ull;  // a candidate that names no row: above every key, never ranked

// Workgroup q = one wave = query q.  LDS: the query zero-padded to 32 floats (seed_select_pass_kernel's staging),
// then keys[pitch], then scores[pitch].
template <int METRIC, typename ROWT>
__global__ __launch_bounds__(64) void rescore_kernel(RescoreParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  const uint32_t dpad = (p.d + 31u) & ~31u;
  float* qs = reinterpret_cast<float*>(smem);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem + (size_t)dpad * 4);
  float* scores = reinterpret_cast<float*>(smem + (size_t)dpad * 4 + (size_t)p.pitch * 8);
  const int lane = threadIdx.x;
  const uint32_t q = blockIdx.x;
  const ROWT* emb = static_cast<const ROWT*>(p.rows);
  const float* qg = p.queries + (uint64_t)q * p.d;
  for (uint32_t j = lane; j < dpad; j += 64) qs[j] = j < p.d ? qg[j] : 0.0f;
  __syncthreads();
  // norm_a of cosine_distance (distance.rs:78): one sequential sum, as the entry-seed pick has it
  float q_norm = 0.0f;
  if (METRIC == METRIC_COSINE_PRE)
    for (uint32_t j = 0; j < p.d; ++j) {
      const float x = qs[j];
      q_norm += x * x;
    }
  const uint32_t have = p.cand_count[q];
  const uint32_t c = have < p.pitch ? have : p.pitch;
  const uint64_t* cand = p.cand + (uint64_t)q * p.pitch;
  uint32_t valid = 0;
  for (uint32_t base = 0; base < c; base += 64) {
    const uint32_t R = c - base < 64u ? c - base : 64u;
    const bool live = (uint32_t)lane < R;
    const uint64_t id = live ? cand[base + lane] : 0ull;
    const bool ok = live && id < p.n;
    const uint32_t rid = ok ? (uint32_t)id : 0u;  // (a lane without a row evaluates row 0 and drops the value)
    const float aux = METRIC == METRIC_COSINE_PRE ? p.norm2[rid] : 0.0f;
    const float s = direct_distances<METRIC, ROWT>(emb, p.stride, p.d, rid, R, qs, q_norm, aux);
    if (live) {
      keys[base + lane] = ok ? (((unsigned long long)ordkey(s) << 32) | (unsigned long long)(base + lane)) : kNoKey;
      scores[base + lane] = s;
    }
    valid += (uint32_t)__popcll(ballot(ok));
  }
  __syncthreads();
  // candidate i goes to slot #{j : key_j < key_i}: the keys differ in their positions, so the slots do
  for (uint32_t i = lane; i < c; i += 64) {
    const unsigned long long key = keys[i];
    if (key == kNoKey) continue;
    uint32_t rank = 0;
    for (uint32_t j = 0; j < c; ++j) rank += keys[j] < key ? 1u : 0u;
    if (rank < p.k) {
      p.out_ids[(uint64_t)q * p.k + rank] = cand[i];
      p.out_dist[(uint64_t)q * p.k + rank] = scores[i];
    }
  }
  if (lane == 0) p.out_count[q] = valid < p.k ? valid : p.k;
}

isl_refine::Handle describe(const isl_index* idx) {
  isl_refine::Handle h{};
  h.null_idx = idx == nullptr;
  if (!idx) return h;
  h.is_hnsw = idx->is_hnsw;
  h.on_device = idx->device >= 0;
  h.recompute = idx->recompute;
  h.has_dimension = idx->has_dimension;
  h.len = idx->num_nodes;
  h.dimension = idx->dimension;
  h.table_rows = idx->refine.n();
  h.table_d = idx->refine.rows().d();
  return h;
}

bool any_scratch_busy(const isl_index* idx) {
  for (const auto& s : idx->refine_scratch)
    if (s->busy) return true;
  return false;
}

// the rows of a host-placed table: a pinned, device-mapped block laid out as a device table is, padding and slack zero
isl_status fill_host_block(isl::RefineTable& t, const void* rows, uint64_t n, uint64_t d, int32_t dtype, int32_t mem) {
  const uint64_t es = isl_rows::elem_size(dtype), stride = isl_rows::stride(dtype, d);
  const uint64_t elems = isl_rows::alloc_elems(dtype, n, d);
  void* block = nullptr;
  const hipError_t e = hipHostMalloc(&block, (size_t)(elems * es), hipHostMallocMapped | hipHostMallocPortable);
  if (e != hipSuccess)
    return fail(ISL_ERR_DEVICE, "hipHostMalloc of %llu bytes failed for the refine table: %s",
                (unsigned long long)(elems * es), hipGetErrorString(e));
  t.host.adopt(static_cast<unsigned char*>(block), elems * es);
  unsigned char* at = t.host.get();
  if (stride != d) memset(at, 0, (size_t)(elems * es));
  else memset(at + n * stride * es, 0, (size_t)(isl_rows::slack(dtype) * es));
  if (mem == ISL_MEM_DEVICE) {
    ISL_HIP(hipMemcpy2D(at, stride * es, rows, d * es, d * es, n, hipMemcpyDeviceToHost));
  } else if (stride == d) {
    memcpy(at, rows, (size_t)(n * d * es));
  } else {
    const unsigned char* src = static_cast<const unsigned char*>(rows);
    for (uint64_t i = 0; i < n; ++i) memcpy(at + i * stride * es, src + i * d * es, (size_t)(d * es));
  }
  void* dptr = nullptr;
  ISL_HIP(hipHostGetDevicePointer(&dptr, block, 0));
  ISL_TRY(t.host_norm2.reserve(n));
  t.view = isl::RowTable::view_over(dptr, elems, t.host_norm2.get(), dtype, n, d);
  t.placement = ISL_REFINE_HOST;
  return t.view.norms(0, n);  // the routine isl_set_embeddings ends with, reading the block across the bus
}

// enqueues the rescoring of nq candidate rows on `st` (arguments checked)
isl_status launch_rescore(const isl_index* idx, const float* d_queries, uint64_t nq, const uint64_t* d_cand_ids,
                          const uint32_t* d_cand_count, uint64_t pitch, uint64_t k, uint64_t* d_out_ids,
                          float* d_out_dist, uint32_t* d_out_count, hipStream_t st) {
  const isl::RowTable& y = idx->refine.rows();
  RescoreParams p{};
  p.queries = d_queries;
  p.rows = y.data();
  p.norm2 = y.norm2();
  p.stride = y.stride();
  p.n = y.n();
  p.d = (uint32_t)y.d();
  p.pitch = (uint32_t)pitch;
  p.k = (uint32_t)k;
  p.cand = d_cand_ids;
  p.cand_count = d_cand_count;
  p.out_ids = d_out_ids;
  p.out_dist = d_out_dist;
  p.out_count = d_out_count;
  const size_t lds = (size_t)isl_refine::lds_bytes(y.d(), pitch);
  isl::by_metric(idx->cfg.metric, [&](auto mc) {
    constexpr int m = decltype(mc)::value == ISL_METRIC_COSINE ? METRIC_COSINE_PRE : decltype(mc)::value;
    y.with_row_type([&](auto row) {  // (isl_index_set_refine_rows refuses fp8 rows: no kernel here is built for them)
      if constexpr (!std::is_same<decltype(row), isl::fp8_e4m3>::value) {
        auto kern = rescore_kernel<m, decltype(row)>;
        if (lds > 48u * 1024u)
          (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3(isl_refine::grid(nq)), dim3(isl_refine::kBlock), lds, st, p);
      }
    });
  });
  ISL_HIP(hipGetLastError());
  return ISL_OK;
}

// the words of the refusals the refined entry points share
isl_status refuse_refined(const isl_index* idx, isl_refine::Verdict v, const char* who, uint64_t d, uint64_t k,
                          uint64_t candidates, uint64_t ef, const char* cand_name) {
  using namespace isl_refine;
  const isl_status st = v.status;
  const unsigned long long kk = k, cc = candidates;
  switch (v.why) {
    case kNull: return fail(st, "%s: NULL argument", who);
    case kNoTable: return fail(st, "%s: the index has no refine table (isl_index_set_refine_rows sets one)", who);
    case kZeroK: return fail(st, "%s: k must be at least 1", who);
    case kKAboveCandidates: return fail(st, "%s: k = %llu exceeds %s = %llu", who, kk, cand_name, cc);
    case kCandidatesAboveEf: return fail(st, "%s: candidates = %llu exceed ef = %llu", who, cc, (unsigned long long)ef);
    case kCandidateLimit:
      return fail(st, "%s: %s = %llu exceeds ISL_REFINE_MAX_CANDIDATES = %u", who, cand_name, cc, ISL_REFINE_MAX_CANDIDATES);
    case kDimMismatch: return isl::fail_dim(idx->refine.rows().d(), d);
    case kRecompute: return fail(st, "%s: an index on the recompute provider is not refined", who);
    case kHnsw: return fail(st, "%s: the core index of an HnswGraph is not refined", who);
    default: return fail(st, "%s: too many queries", who);
  }
}

// a scratch set of the handle's for one refined call: an idle one, or a new one
isl::RefineScratch* claim_scratch(const isl_index* idx) {
  std::lock_guard<std::mutex> lock(idx->mu);
  for (auto& s : idx->refine_scratch)
    if (!s->busy) {
      s->busy = true;
      return s.get();
    }
  idx->refine_scratch.emplace_back(new isl::RefineScratch);
  idx->refine_scratch.back()->busy = true;
  return idx->refine_scratch.back().get();
}
struct ScratchGuard {
  const isl_index* idx;
  isl::RefineScratch* s;
  ~ScratchGuard() {
    std::lock_guard<std::mutex> lock(idx->mu);
    s->busy = false;
  }
};

}  // namespace

extern "C" {

isl_status isl_index_set_refine_rows(isl_index* idx, const void* rows, uint64_t n, uint64_t d, int32_t dtype,
                                     int32_t mem, int32_t placement) {
  static const char* who = "isl_index_set_refine_rows";
  bool drops = false;
  const isl_refine::Verdict v = isl_refine::check_set_rows(describe(idx), rows == nullptr, n, d, dtype, mem, placement, &drops);
  switch (v.why) {
    using namespace isl_refine;
    case kPass: break;
    case kNull: return fail(v.status, "%s: NULL argument", who);
    case kUnknownEnum: return fail(v.status, "%s: unknown dtype, mem or placement", who);
    case kFp8: return fail(v.status, "%s: refine rows are f32 or bf16, not fp8", who);
    case kHnsw: return fail(v.status, "%s: this is the core index of an HnswGraph, which is not refined", who);
    case kNoDevice: return fail(v.status, "%s needs the index on a device (isl_index_upload)", who);
    case kRowCount:
      return fail(v.status, "%s: %llu rows for an index of %llu nodes", who, (unsigned long long)n,
                  (unsigned long long)idx->num_nodes);
    case kNoDim: return fail(v.status, "Empty vector collection");
    case kDimMismatch: return isl::fail_dim(idx->dimension, d);
    default: return fail(v.status, "%s takes rows of up to %llu elements", who, (unsigned long long)kMaxDim);
  }
  auto busy = [&]() { return isl::any_lane_busy(idx) || any_scratch_busy(idx); };
  if (drops) {
    std::lock_guard<std::mutex> lock(idx->mu);
    if (busy()) return fail(ISL_ERR_SEARCH, "Search error: %s while searches are in flight", who);
    idx->refine.reset();
    return ISL_OK;
  }
  {
    std::lock_guard<std::mutex> lock(idx->mu);
    if (busy()) return fail(ISL_ERR_SEARCH, "Search error: %s while searches are in flight", who);
  }
  ISL_TRY(isl::use_device(idx->device));
  // the new table beside the old one, which nothing below touches
  isl::RefineTable fresh;
  if (placement == ISL_REFINE_DEVICE) {
    if (fresh.dev.allocate(dtype, n, d) != ISL_OK)
      return fail(ISL_ERR_DEVICE, "%s: hipMalloc failed for %llu rows", who, (unsigned long long)n);
    ISL_TRY(fresh.dev.fill(0, n, rows, mem));
    fresh.placement = ISL_REFINE_DEVICE;
  } else {
    ISL_TRY(fill_host_block(fresh, rows, n, d, dtype, mem));
  }
  std::lock_guard<std::mutex> lock(idx->mu);
  if (busy()) return fail(ISL_ERR_SEARCH, "Search error: %s while searches are in flight", who);
  idx->refine.reset();
  idx->refine = std::move(fresh);
  return ISL_OK;
}

isl_status isl_index_refine_storage(const isl_index* idx, int32_t* dtype, int32_t* placement, uint64_t* rows,
                                    uint64_t* block_bytes) {
  if (!idx) return fail(ISL_ERR_INVALID_ARGUMENT, "index is NULL");
  std::lock_guard<std::mutex> lock(idx->mu);
  const isl::RowTable& t = idx->refine.rows();
  const bool held = t.n() > 0;
  if (dtype) *dtype = held ? t.dtype() : ISL_DTYPE_F32;
  if (placement) *placement = held ? idx->refine.placement : ISL_REFINE_DEVICE;
  if (rows) *rows = t.n();
  if (block_bytes) *block_bytes = held ? t.block_bytes() : 0;
  return ISL_OK;
}

isl_status isl_rescore_device(const isl_index* idx, const float* d_queries, uint64_t nq, uint64_t d,
                              const uint64_t* d_cand_ids, const uint32_t* d_cand_count, uint64_t pitch, uint64_t k,
                              uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count, void* stream) {
  static const char* who = "isl_rescore_device";
  const bool null_buf = !d_queries || !d_cand_ids || !d_cand_count || !d_out_ids || !d_out_dist || !d_out_count;
  const isl_refine::Verdict v = isl_refine::check_refined(describe(idx), null_buf, nq, d, k, pitch, pitch);
  if (v.status != ISL_OK) return refuse_refined(idx, v, who, d, k, pitch, pitch, "pitch");
  if (!nq) return ISL_OK;
  ISL_TRY(isl::use_device(idx->device));
  return launch_rescore(idx, d_queries, nq, d_cand_ids, d_cand_count, pitch, k, d_out_ids, d_out_dist, d_out_count,
                        (hipStream_t)stream);
}

isl_status isl_rescore(const isl_index* idx, const float* queries, uint64_t nq, uint64_t d, const uint64_t* cand_ids,
                       const uint32_t* cand_count, uint64_t pitch, uint64_t k, uint64_t* out_ids, float* out_dist,
                       uint32_t* out_count) {
  static const char* who = "isl_rescore";
  const bool null_buf = !queries || !cand_ids || !cand_count || !out_ids || !out_dist || !out_count;
  const isl_refine::Verdict v = isl_refine::check_refined(describe(idx), null_buf, nq, d, k, pitch, pitch);
  if (v.status != ISL_OK) return refuse_refined(idx, v, who, d, k, pitch, pitch, "pitch");
  if (!nq) return ISL_OK;
  ISL_TRY(isl::use_device(idx->device));
  isl::RefineScratch* s = claim_scratch(idx);
  ScratchGuard guard{idx, s};
  ISL_TRY(s->q_stage.reserve(nq * d));
  ISL_TRY(s->ids.reserve(nq * pitch));
  ISL_TRY(s->count.reserve(nq));
  ISL_TRY(s->out_ids.reserve(nq * k));
  ISL_TRY(s->out_dist.reserve(nq * k));
  ISL_TRY(s->out_count.reserve(nq));
  ISL_HIP(hipMemcpy(s->q_stage, queries, (size_t)(nq * d) * 4, hipMemcpyHostToDevice));
  ISL_HIP(hipMemcpy(s->ids, cand_ids, (size_t)(nq * pitch) * 8, hipMemcpyHostToDevice));
  ISL_HIP(hipMemcpy(s->count, cand_count, (size_t)nq * 4, hipMemcpyHostToDevice));
  // (rows the rescoring leaves short stay zero behind their counts)
  ISL_HIP(hipMemset(s->out_ids, 0, (size_t)(nq * k) * 8));
  ISL_HIP(hipMemset(s->out_dist, 0, (size_t)(nq * k) * 4));
  const isl_status r = launch_rescore(idx, s->q_stage, nq, s->ids, s->count, pitch, k, s->out_ids, s->out_dist,
                                      s->out_count, nullptr);
  const hipError_t es = hipStreamSynchronize(nullptr);  // (the scratch goes back to the handle when this returns)
  if (r != ISL_OK) return r;
  if (es != hipSuccess) return fail(ISL_ERR_DEVICE, "%s failed: %s", who, hipGetErrorString(es));
  ISL_HIP(hipMemcpy(out_ids, s->out_ids, (size_t)(nq * k) * 8, hipMemcpyDeviceToHost));
  ISL_HIP(hipMemcpy(out_dist, s->out_dist, (size_t)(nq * k) * 4, hipMemcpyDeviceToHost));
  ISL_HIP(hipMemcpy(out_count, s->out_count, (size_t)nq * 4, hipMemcpyDeviceToHost));
  return ISL_OK;
}

isl_status isl_search_refined_batch_device(const isl_index* idx, const float* d_queries, uint64_t nq, uint64_t d,
                                           uint64_t k, uint64_t candidates, uint64_t ef, uint64_t* d_out_ids,
                                           float* d_out_dist, uint32_t* d_out_count, void* stream) {
  static const char* who = "isl_search_refined_batch_device";
  const bool null_buf = !d_queries || !d_out_ids || !d_out_dist || !d_out_count;
  const isl_refine::Verdict v = isl_refine::check_refined(describe(idx), null_buf, nq, d, k, candidates, ef);
  if (v.status != ISL_OK) return refuse_refined(idx, v, who, d, k, candidates, ef, "candidates");
  if (!nq) return ISL_OK;
  ISL_TRY(isl::use_device(idx->device));
  isl::RefineScratch* s = claim_scratch(idx);
  ScratchGuard guard{idx, s};
  const isl_refine::Scratch need = isl_refine::scratch_elems(nq, candidates);
  uint64_t events = 0;
  ISL_TRY(s->ids.reserve(need.ids, &events));
  ISL_TRY(s->dist.reserve(need.dist, &events));
  ISL_TRY(s->count.reserve(need.count, &events));
  hipStream_t hs = (hipStream_t)stream;
  isl_status r = isl_search_batch_device(idx, d_queries, nq, d, candidates, ef, s->ids, s->dist, s->count, stream);
  isl::add_last_allocations(idx, events);
  if (r != ISL_OK) return r;
  r = launch_rescore(idx, d_queries, nq, s->ids, s->count, candidates, k, d_out_ids, d_out_dist, d_out_count, hs);
  const hipError_t es = hipStreamSynchronize(hs);  // (the scratch goes back to the handle when this returns)
  if (r != ISL_OK) return r;
  if (es != hipSuccess) return fail(ISL_ERR_DEVICE, "%s failed: %s", who, hipGetErrorString(es));
  return ISL_OK;
}

isl_status isl_search_refined_batch(const isl_index* idx, const float* queries, uint64_t nq, uint64_t d, uint64_t k,
                                    uint64_t candidates, uint64_t ef, uint64_t* out_ids, float* out_dist,
                                    uint32_t* out_count) {
  static const char* who = "isl_search_refined_batch";
  const bool null_buf = !queries || !out_ids || !out_dist || !out_count;
  const isl_refine::Verdict v = isl_refine::check_refined(describe(idx), null_buf, nq, d, k, candidates, ef);
  if (v.status != ISL_OK) return refuse_refined(idx, v, who, d, k, candidates, ef, "candidates");
  if (!nq) return ISL_OK;
  ISL_TRY(isl::use_device(idx->device));
  isl::RefineScratch* s = claim_scratch(idx);
  ScratchGuard guard{idx, s};
  uint64_t events = 0;
  ISL_TRY(s->q_stage.reserve(nq * d, &events));
  ISL_TRY(s->out_ids.reserve(nq * k, &events));
  ISL_TRY(s->out_dist.reserve(nq * k, &events));
  ISL_TRY(s->out_count.reserve(nq, &events));
  const isl_refine::Scratch need = isl_refine::scratch_elems(nq, candidates);
  ISL_TRY(s->ids.reserve(need.ids, &events));
  ISL_TRY(s->dist.reserve(need.dist, &events));
  ISL_TRY(s->count.reserve(need.count, &events));
  ISL_HIP(hipMemcpy(s->q_stage, queries, (size_t)(nq * d) * 4, hipMemcpyHostToDevice));
  isl_status r = isl_search_batch_device(idx, s->q_stage, nq, d, candidates, ef, s->ids, s->dist, s->count, nullptr);
  isl::add_last_allocations(idx, events);
  if (r != ISL_OK) return r;
  // (rows the rescoring leaves short stay zero behind their counts)
  ISL_HIP(hipMemsetAsync(s->out_ids, 0, (size_t)(nq * k) * 8, nullptr));
  ISL_HIP(hipMemsetAsync(s->out_dist, 0, (size_t)(nq * k) * 4, nullptr));
  r = launch_rescore(idx, s->q_stage, nq, s->ids, s->count, candidates, k, s->out_ids, s->out_dist, s->out_count, nullptr);
  if (r != ISL_OK) {
    (void)hipStreamSynchronize(nullptr);
    return r;
  }
  ISL_HIP(hipMemcpy(out_ids, s->out_ids, (size_t)(nq * k) * 8, hipMemcpyDeviceToHost));
  ISL_HIP(hipMemcpy(out_dist, s->out_dist, (size_t)(nq * k) * 4, hipMemcpyDeviceToHost));
  ISL_HIP(hipMemcpy(out_count, s->out_count, (size_t)nq * 4, hipMemcpyDeviceToHost));
  return ISL_OK;
}

}  // extern "C"
