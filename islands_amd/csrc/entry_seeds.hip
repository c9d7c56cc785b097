// Entry seeds of a LeannIndex: E node ids plus a contiguous copy of their rows.  While the table is set,
// every plain search starts each query at the seed nearest to it (search.hip hands the pick's answer to
// the traversal through SearchParams::q_entry); everything after that start is the unchanged traversal.
//   selection  greedy k-centre from the entry point: one pass over all rows per seed
//   pick       the nearest seed of every query: a tiled kernel in front of the traversal
// Both evaluate Distance::calculate in the reference's order -- one sequential f32 chain per pair, multiply
// and add rounded separately (dterm / dfinish of device_common.hip.h; this unit is built -ffp-contract=off).
#include "device_common.hip.h"
#include "entry_seeds_plan.hpp"
#include "query_status.hpp"

#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <vector>

namespace {

using namespace isl_dev;
using isl::fail;
using isl_seeds::PDC;
using isl_seeds::PLD;
using isl_seeds::PQT;
using isl_seeds::PST;

// (ordkey, id) of a row as one word that orders by the key first and by the SMALLER id among equal keys
// under a maximum; 0 never names a row (no key is 0: the least, -inf, maps to 0x007FFFFF)
__device__ __forceinline__ unsigned long long far_word(uint32_t key, uint32_t id) {
  return ((unsigned long long)key << 32) | (unsigned long long)(0xFFFFFFFFu - id);
}
__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }

// ------------------------------------------------------------------ selection
struct SelectParams {
  const void* emb;
  const float* norm2;
  uint64_t stride, n;
  uint32_t d;
  uint32_t* mind;            // [n] ordkey of the distance to the nearest seed so far; 0 = the row is a seed
  unsigned long long* best;  // [seeds]: far_word of seed p; best[0] is the host's, the passes write the rest
  uint32_t pass;             // measures seed `pass`, reduces the next seed into best[pass + 1]
};

// One wave per 64 consecutive rows, grid-striding.  The seed's row (a of D(a, b)) sits in LDS as the
// traversal's query does, the rows go through direct_distances: the chain of the search kernel.
template <int METRIC, typename ROWT>
__global__ __launch_bounds__(64) void seed_select_pass_kernel(SelectParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  float* qs = reinterpret_cast<float*>(smem);
  const int lane = threadIdx.x;
  const ROWT* emb = static_cast<const ROWT*>(p.emb);
  const uint32_t seed = 0xFFFFFFFFu - (uint32_t)p.best[p.pass];
  const ROWT* srow = emb + (uint64_t)seed * p.stride;
  const uint32_t dpad = (p.d + 31u) & ~31u;
  for (uint32_t j = lane; j < dpad; j += 64) qs[j] = j < p.d ? widen(srow[j]) : 0.0f;
  __syncthreads();
  // norm_a of cosine_distance is the seed row's own sum of squares: the precomputed norm is those bits
  const float q_norm = METRIC == METRIC_COSINE_PRE ? p.norm2[seed] : 0.0f;
  unsigned long long far = 0ull;
  for (uint64_t base = (uint64_t)blockIdx.x * 64; base < p.n; base += (uint64_t)gridDim.x * 64) {
    const uint32_t R = (uint32_t)(p.n - base < 64 ? p.n - base : 64);
    const bool live = (uint32_t)lane < R;
    const uint32_t rid = (uint32_t)base + (live ? (uint32_t)lane : 0u);
    const float aux = METRIC == METRIC_COSINE_PRE ? p.norm2[rid] : 0.0f;
    const float dist = direct_distances<METRIC, ROWT>(emb, p.stride, p.d, rid, R, qs, q_norm, aux);
    if (live) {
      const uint32_t old = p.pass == 0 ? 0xFFFFFFFFu : p.mind[rid];
      const uint32_t key = ordkey(dist);
      const uint32_t now = (rid == seed || old == 0u) ? 0u : (key < old ? key : old);
      p.mind[rid] = now;
      if (now) {
        const unsigned long long w = far_word(now, rid);
        far = w > far ? w : far;
      }
    }
  }
  for (int off = 32; off; off >>= 1) {
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(far >> 32), off);
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)far, off);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    far = o > far ? o : far;
  }
  if (lane == 0 && far) atomicMax(p.best + p.pass + 1, far);
}

template <typename T>
__global__ __launch_bounds__(256) void gather_seed_rows_kernel(const T* __restrict__ emb, uint64_t stride,
                                                               const float* __restrict__ norm2,
                                                               const uint32_t* __restrict__ ids, T* __restrict__ out,
                                                               float* __restrict__ out_norm2) {
  const uint32_t s = blockIdx.x;
  const uint64_t id = ids[s];
  for (uint64_t j = threadIdx.x; j < stride; j += 256) out[(uint64_t)s * stride + j] = emb[id * stride + j];
  if (threadIdx.x == 0) out_norm2[s] = norm2[id];
}

// ----------------------------------------------------------------------- pick
struct PickParams {
  const float* queries;  // [nq][d]
  const void* rows;      // the seed table, [seeds][stride] of the index's row type
  const float* norm2;    // [seeds]
  uint64_t stride;
  uint32_t nq, d, seeds, tiles_per_split;
  unsigned long long* packed;  // [nq] running minimum of (ordkey << 32 | position), all ones before
};

// A workgroup owns PQT queries and a range of seed tiles.  Per PDC elements of d it stages the tile of
// queries and the tile of seeds in LDS (coalesced 128-byte row pieces); thread (ty, tx) of 16 x 16 runs the
// four chains of queries {ty, ty + 16} x seeds {tx, tx + 16} over the chunk, so every LDS word is used by
// two chains of the thread and, as a broadcast or a conflict-free b128 read, by 16 lanes.  A chain adds its
// elements in the order 0, 1, 2, ...: the chunks follow each other in the accumulator.  The nq x seeds
// matrix is never written: each query keeps (ordkey, position) of its nearest seed so far.
template <int METRIC, typename ROWT>
__global__ __launch_bounds__(256) void seed_pick_kernel(PickParams p) {
  __shared__ __align__(16) float qt[PQT * PLD];
  __shared__ __align__(16) float st[PST * PLD];
  __shared__ float qn[PQT];
  const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
  const uint32_t q0 = blockIdx.x * PQT;
  const uint32_t ntiles = (p.seeds + PST - 1) / PST;
  const uint32_t tile0 = blockIdx.y * p.tiles_per_split;
  const uint32_t tile1 = tile0 + p.tiles_per_split < ntiles ? tile0 + p.tiles_per_split : ntiles;
  const ROWT* rows = static_cast<const ROWT*>(p.rows);
  constexpr bool COS = METRIC == METRIC_COSINE_PRE;
  unsigned long long near0 = ~0ull, near1 = ~0ull;  // queries q0 + ty, q0 + ty + 16
  float nacc = 0.0f;                                // thread tid < PQT: norm_a of query q0 + tid
  const float* qa = qt + ty * PLD;
  const float* qb = qt + (ty + 16u) * PLD;
  const float* sa = st + tx * PLD;
  const float* sb = st + (tx + 16u) * PLD;
  for (uint32_t t = tile0; t < tile1; ++t) {
    const uint32_t s0 = t * PST;
    float a00 = 0.0f, a01 = 0.0f, a10 = 0.0f, a11 = 0.0f;
    for (uint32_t c0 = 0; c0 < p.d; c0 += PDC) {
      for (uint32_t i = tid; i < PQT * PDC; i += 256) {
        const uint32_t r = i / PDC, c = i % PDC;
        const bool in = c0 + c < p.d;
        qt[r * PLD + c] = (in && q0 + r < p.nq) ? p.queries[(uint64_t)(q0 + r) * p.d + c0 + c] : 0.0f;
        st[r * PLD + c] = (in && s0 + r < p.seeds) ? widen(rows[(uint64_t)(s0 + r) * p.stride + c0 + c]) : 0.0f;
      }
      __syncthreads();
      const uint32_t cnt = p.d - c0 < PDC ? p.d - c0 : PDC;
      if (cnt == PDC) {
#pragma unroll
        for (uint32_t j = 0; j < PDC; j += 4) {
          const float4 u = *reinterpret_cast<const float4*>(qa + j);
          const float4 v = *reinterpret_cast<const float4*>(qb + j);
          const float4 x = *reinterpret_cast<const float4*>(sa + j);
          const float4 y = *reinterpret_cast<const float4*>(sb + j);
          a00 += dterm<METRIC>(u.x, x.x); a01 += dterm<METRIC>(u.x, y.x);
          a10 += dterm<METRIC>(v.x, x.x); a11 += dterm<METRIC>(v.x, y.x);
          a00 += dterm<METRIC>(u.y, x.y); a01 += dterm<METRIC>(u.y, y.y);
          a10 += dterm<METRIC>(v.y, x.y); a11 += dterm<METRIC>(v.y, y.y);
          a00 += dterm<METRIC>(u.z, x.z); a01 += dterm<METRIC>(u.z, y.z);
          a10 += dterm<METRIC>(v.z, x.z); a11 += dterm<METRIC>(v.z, y.z);
          a00 += dterm<METRIC>(u.w, x.w); a01 += dterm<METRIC>(u.w, y.w);
          a10 += dterm<METRIC>(v.w, x.w); a11 += dterm<METRIC>(v.w, y.w);
        }
      } else {
        for (uint32_t j = 0; j < cnt; ++j) {
          const float u = qa[j], v = qb[j], x = sa[j], y = sb[j];
          a00 += dterm<METRIC>(u, x); a01 += dterm<METRIC>(u, y);
          a10 += dterm<METRIC>(v, x); a11 += dterm<METRIC>(v, y);
        }
      }
      if (COS && t == tile0 && tid < PQT) {  // norm_a += x*x, distance.rs:78, while the chunk is here
        const float* qr = qt + tid * PLD;
        for (uint32_t j = 0; j < cnt; ++j) nacc += qr[j] * qr[j];
      }
      __syncthreads();
    }
    if (COS && t == tile0) {
      if (tid < PQT) qn[tid] = nacc;
      __syncthreads();
    }
    const float na0 = COS ? qn[ty] : 0.0f, na1 = COS ? qn[ty + 16u] : 0.0f;
    const uint32_t p0 = s0 + tx, p1 = s0 + tx + 16u;
    if (p0 < p.seeds) {
      const float nb = COS ? p.norm2[p0] : 0.0f;
      const unsigned long long w0 = ((unsigned long long)ordkey(dfinish<METRIC>(a00, nb, na0)) << 32) | p0;
      const unsigned long long w1 = ((unsigned long long)ordkey(dfinish<METRIC>(a10, nb, na1)) << 32) | p0;
      near0 = w0 < near0 ? w0 : near0;
      near1 = w1 < near1 ? w1 : near1;
    }
    if (p1 < p.seeds) {
      const float nb = COS ? p.norm2[p1] : 0.0f;
      const unsigned long long w0 = ((unsigned long long)ordkey(dfinish<METRIC>(a01, nb, na0)) << 32) | p1;
      const unsigned long long w1 = ((unsigned long long)ordkey(dfinish<METRIC>(a11, nb, na1)) << 32) | p1;
      near0 = w0 < near0 ? w0 : near0;
      near1 = w1 < near1 ? w1 : near1;
    }
  }
  // the 16 lanes that share a query sit side by side in the wave
  for (int off = 8; off; off >>= 1) {
    const unsigned long long o0 = ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(near0 >> 32), off) << 32) |
                                  (uint32_t)__shfl_xor((int)(uint32_t)near0, off);
    const unsigned long long o1 = ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(near1 >> 32), off) << 32) |
                                  (uint32_t)__shfl_xor((int)(uint32_t)near1, off);
    near0 = o0 < near0 ? o0 : near0;
    near1 = o1 < near1 ? o1 : near1;
  }
  if (tx == 0 && tile0 < tile1) {
    if (q0 + ty < p.nq) atomicMin(p.packed + q0 + ty, near0);
    if (q0 + ty + 16u < p.nq) atomicMin(p.packed + q0 + ty + 16u, near1);
  }
}

// position -> node id, and what the traversal expects beside a given entry: one evaluation counted, status OK
__global__ __launch_bounds__(256) void seed_pick_finish_kernel(const unsigned long long* __restrict__ packed,
                                                               const uint32_t* __restrict__ seed_ids, uint32_t seeds,
                                                               uint32_t nq, uint32_t* __restrict__ q_entry,
                                                               uint32_t* __restrict__ q_evals,
                                                               uint32_t* __restrict__ status,
                                                               uint64_t* __restrict__ out_ids) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= nq) return;
  uint32_t pos = (uint32_t)packed[q];
  if (pos >= seeds) pos = 0;
  const uint32_t id = seed_ids[pos];
  if (q_entry) q_entry[q] = id;
  if (q_evals) q_evals[q] = 1u;
  if (status) status[q] = QS_OK;
  if (out_ids) out_ids[q] = id;
}

// f(metric constant, row type tag) for the index's metric and the type of `rows`; cosine takes the precomputed norms
template <typename F>
void by_metric_rows(uint32_t metric, const isl::RowTable& rows, F&& f) {
  isl::by_metric(metric, [&](auto mc) {
    constexpr int m = decltype(mc)::value == ISL_METRIC_COSINE ? METRIC_COSINE_PRE : decltype(mc)::value;
    rows.with_row_type([&](auto row) {  // (check_seedable refuses fp8 rows: no kernel here is built for them)
      if constexpr (!std::is_same<decltype(row), isl::fp8_e4m3>::value) f(std::integral_constant<int, m>{}, row);
    });
  });
}

constexpr uint32_t kMaxSelectDim = 32768;  // the seed's row waits in LDS as f32: 128 KiB of the CU's 160

// what the four entry points ask of the handle before anything else
isl_status check_seedable(const isl_index* idx, const char* who) {
  if (idx->is_hnsw) return fail(ISL_ERR_UNSUPPORTED, "%s: entry seeds belong to a LeannIndex, not to the HnswGraph facade", who);
  if (idx->num_nodes == 0) return fail(ISL_ERR_EMPTY_COLLECTION, "%s: the index is empty", who);
  if (idx->recompute || !idx->rows.resident() || idx->device < 0)
    return fail(ISL_ERR_UNSUPPORTED, "%s needs rows resident on the device", who);
  if (idx->rows.is_fp8()) return fail(ISL_ERR_UNSUPPORTED, "%s: entry seeds are not gathered from fp8 rows", who);
  return ISL_OK;
}

// ids -> the table (under idx->mu, no search in flight, ids checked): a table is either whole or absent
isl_status install_seeds(isl_index* idx, const std::vector<uint64_t>& ids) {
  idx->seeds = {};
  const uint64_t E = ids.size();
  if (!E) return ISL_OK;
  std::vector<uint32_t> h32(E);
  for (uint64_t i = 0; i < E; ++i) h32[i] = (uint32_t)ids[i];
  const isl::RowTable& from = idx->rows;
  isl::EntrySeeds s;
  ISL_TRY(s.d_ids.reserve(E));
  ISL_TRY(s.rows.allocate(from.dtype(), E, from.d()));
  ISL_HIP(hipMemcpy(s.d_ids, h32.data(), E * 4, hipMemcpyHostToDevice));
  from.with_row_type([&](auto row) {
    using T = decltype(row);
    if constexpr (!std::is_same<T, isl::fp8_e4m3>::value)
      hipLaunchKernelGGL(gather_seed_rows_kernel<T>, dim3((uint32_t)E), dim3(256), 0, 0, from.as<const T>(), from.stride(),
                         from.norm2(), s.d_ids.get(), s.rows.as<T>(), s.rows.norm2());
  });
  ISL_HIP(hipGetLastError());
  ISL_HIP(hipDeviceSynchronize());
  s.ids = ids;
  idx->seeds = std::move(s);
  return ISL_OK;
}

// greedy k-centre over the index's rows (under idx->mu): E - 1 passes back to back on the default stream, each
// reading the seed its predecessor's reduction left in best[], one synchronisation at the end
isl_status select_seeds(isl_index* idx, uint64_t count, std::vector<uint64_t>& ids) {
  ids.clear();
  const uint64_t n = std::min<uint64_t>(idx->num_nodes, idx->nvec);
  const uint64_t E = std::min<uint64_t>(count, n);
  if (!E) return ISL_OK;
  const uint64_t entry = idx->has_entry ? idx->entry_point : 0;
  if (entry >= n) return isl::fail_node(entry);
  if (idx->rows.d() > kMaxSelectDim)
    return fail(ISL_ERR_UNSUPPORTED, "entry-seed selection takes rows of up to %u elements", kMaxSelectDim);
  isl::DeviceBuffer<uint32_t> mind;
  isl::DeviceBuffer<unsigned long long> best;
  ISL_TRY(mind.reserve(n));
  ISL_TRY(best.reserve(E));
  const unsigned long long first = 0xFFFFFFFFull - entry;
  ISL_HIP(hipMemset(best, 0, E * 8));
  ISL_HIP(hipMemcpy(best, &first, 8, hipMemcpyHostToDevice));
  SelectParams p{};
  p.emb = idx->rows.data();
  p.norm2 = idx->rows.norm2();
  p.stride = idx->rows.stride();
  p.n = n;
  p.d = (uint32_t)idx->rows.d();
  p.mind = mind;
  p.best = best;
  const size_t lds = (size_t)((p.d + 31u) & ~31u) * 4;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 63) / 64, 8192);
  by_metric_rows(idx->cfg.metric, idx->rows, [&](auto mc, auto row) {
    auto k = seed_select_pass_kernel<decltype(mc)::value, decltype(row)>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    for (uint64_t pass = 0; pass + 1 < E; ++pass) {
      p.pass = (uint32_t)pass;
      hipLaunchKernelGGL(k, dim3(grid), dim3(64), lds, 0, p);
    }
  });
  ISL_HIP(hipGetLastError());
  ISL_HIP(hipDeviceSynchronize());
  std::vector<unsigned long long> h(E);
  ISL_HIP(hipMemcpy(h.data(), best, E * 8, hipMemcpyDeviceToHost));
  ids.resize(E);
  for (uint64_t i = 0; i < E; ++i) {
    if (!h[i]) return fail(ISL_ERR_DEVICE, "entry-seed selection: pass %llu named no row", (unsigned long long)i);
    ids[i] = 0xFFFFFFFFull - (h[i] & 0xFFFFFFFFull);
  }
  return ISL_OK;
}

}  // namespace

namespace isl {

isl_status launch_entry_pick(const isl_index* idx, const float* d_queries, uint64_t nq, uint32_t* q_entry,
                             uint32_t* q_evals, unsigned long long* packed, uint32_t* status, uint64_t* d_out_ids,
                             hipStream_t st) {
  const isl::RowTable& rows = idx->seeds.rows;
  if (!nq || !rows.n()) return ISL_OK;
  PickParams p{};
  p.queries = d_queries;
  p.rows = rows.data();
  p.norm2 = rows.norm2();
  p.stride = rows.stride();
  p.nq = (uint32_t)nq;
  p.d = (uint32_t)rows.d();
  p.seeds = (uint32_t)rows.n();
  p.packed = packed;
  const isl_seeds::PickGrid g = isl_seeds::pick_grid(nq, rows.n(), (uint32_t)device_cu_count(idx->device));
  p.tiles_per_split = g.tiles_per_split;
  ISL_HIP(hipMemsetAsync(packed, 0xFF, nq * 8, st));
  by_metric_rows(idx->cfg.metric, rows, [&](auto mc, auto row) {
    hipLaunchKernelGGL((seed_pick_kernel<decltype(mc)::value, decltype(row)>), dim3(g.qtiles, g.splits), dim3(256), 0, st,
                       p);
  });
  ISL_HIP(hipGetLastError());
  hipLaunchKernelGGL(seed_pick_finish_kernel, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, st, packed,
                     idx->seeds.d_ids.get(), p.seeds, p.nq, q_entry, q_evals, status, d_out_ids);
  ISL_HIP(hipGetLastError());
  return ISL_OK;
}

isl_status check_seedable_index(const isl_index* idx, const char* who) { return check_seedable(idx, who); }
isl_status install_entry_seeds(isl_index* idx, const std::vector<uint64_t>& ids) { return install_seeds(idx, ids); }

isl_status env_entry_seeds(isl_index* idx) {
  uint64_t count = 0;
  const char* text = getenv("ISL_ENTRY_SEEDS");
  const isl_status st = isl_seeds::parse_seed_env(text, &count);
  if (st == ISL_ERR_UNSUPPORTED)
    return fail(st, "ISL_ENTRY_SEEDS exceeds ISL_MAX_ENTRY_SEEDS = %llu", (unsigned long long)ISL_MAX_ENTRY_SEEDS);
  if (st != ISL_OK) return fail(st, "ISL_ENTRY_SEEDS = \"%s\" is not a decimal count", text);
  if (!count || !idx || idx->num_nodes == 0) return ISL_OK;
  return isl_index_select_entry_seeds(idx, count, nullptr, nullptr);
}

}  // namespace isl

extern "C" {

isl_status isl_index_select_entry_seeds(isl_index* idx, uint64_t count, uint64_t* out_ids, uint64_t* out_count) {
  if (out_count) *out_count = 0;
  if (!idx) return fail(ISL_ERR_INVALID_ARGUMENT, "index is NULL");
  if (count > ISL_MAX_ENTRY_SEEDS)
    return fail(ISL_ERR_UNSUPPORTED, "%llu entry seeds exceed ISL_MAX_ENTRY_SEEDS = %llu", (unsigned long long)count,
                (unsigned long long)ISL_MAX_ENTRY_SEEDS);
  ISL_TRY(check_seedable(idx, "isl_index_select_entry_seeds"));
  ISL_TRY(isl::use_device(idx->device));
  std::lock_guard<std::mutex> lock(idx->mu);
  if (isl::any_lane_busy(idx))
    return fail(ISL_ERR_SEARCH, "Search error: isl_index_select_entry_seeds while searches are in flight");
  std::vector<uint64_t> ids;
  ISL_TRY(select_seeds(idx, count, ids));
  ISL_TRY(install_seeds(idx, ids));
  if (out_ids) std::copy(ids.begin(), ids.end(), out_ids);
  if (out_count) *out_count = ids.size();
  return ISL_OK;
}

isl_status isl_index_set_entry_seeds(isl_index* idx, const uint64_t* ids, uint64_t count) {
  if (!idx) return fail(ISL_ERR_INVALID_ARGUMENT, "index is NULL");
  if (count > ISL_MAX_ENTRY_SEEDS)
    return fail(ISL_ERR_UNSUPPORTED, "%llu entry seeds exceed ISL_MAX_ENTRY_SEEDS = %llu", (unsigned long long)count,
                (unsigned long long)ISL_MAX_ENTRY_SEEDS);
  if (count && !ids) return fail(ISL_ERR_INVALID_ARGUMENT, "ids is NULL");
  if (count) {
    ISL_TRY(check_seedable(idx, "isl_index_set_entry_seeds"));
    uint64_t bad = 0;
    if (isl_seeds::check_seed_ids(ids, count, idx->num_nodes, idx->nvec, &bad) == ISL_ERR_NODE_NOT_FOUND)
      return isl::fail_node(bad);
    ISL_TRY(isl::use_device(idx->device));
  }
  std::lock_guard<std::mutex> lock(idx->mu);
  if (isl::any_lane_busy(idx))
    return fail(ISL_ERR_SEARCH, "Search error: isl_index_set_entry_seeds while searches are in flight");
  return install_seeds(idx, std::vector<uint64_t>(ids, ids + count));
}

isl_status isl_index_entry_seeds(const isl_index* idx, uint64_t* out, uint64_t cap, uint64_t* count) {
  if (count) *count = 0;
  if (!idx) return fail(ISL_ERR_INVALID_ARGUMENT, "index is NULL");
  if (cap && !out) return fail(ISL_ERR_INVALID_ARGUMENT, "out is NULL");
  std::lock_guard<std::mutex> lock(idx->mu);
  const uint64_t E = idx->seeds.count();
  if (count) *count = E;
  std::copy(idx->seeds.ids.begin(), idx->seeds.ids.begin() + std::min(cap, E), out);
  return ISL_OK;
}

isl_status isl_index_pick_entries(const isl_index* idx, const float* queries, uint64_t nq, uint64_t d,
                                  uint64_t* out_ids, int32_t mem, void* stream) {
  if (!idx) return fail(ISL_ERR_INVALID_ARGUMENT, "index is NULL");
  if (nq && (!queries || !out_ids)) return fail(ISL_ERR_INVALID_ARGUMENT, "NULL buffer");
  if (mem != ISL_MEM_HOST && mem != ISL_MEM_DEVICE) return fail(ISL_ERR_INVALID_ARGUMENT, "unknown memory space");
  if (nq > 0x7FFFFFFFull) return fail(ISL_ERR_INVALID_ARGUMENT, "too many queries");
  ISL_TRY(check_seedable(idx, "isl_index_pick_entries"));
  if (!idx->seeds.count()) return fail(ISL_ERR_INVALID_ARGUMENT, "isl_index_pick_entries: the index has no entry seeds");
  if (d != idx->rows.d()) return isl::fail_dim(idx->rows.d(), d);
  if (!nq) return ISL_OK;
  ISL_TRY(isl::use_device(idx->device));
  hipStream_t st = (hipStream_t)stream;
  isl::TempScope tmp;
  unsigned long long* packed = tmp.alloc<unsigned long long>(nq);
  const float* dq = queries;
  uint64_t* dout = out_ids;
  if (mem == ISL_MEM_HOST) {
    float* stage = tmp.alloc<float>(nq * d);
    dout = tmp.alloc<uint64_t>(nq);
    if (!stage || !dout) return fail(ISL_ERR_DEVICE, "hipMalloc failed in isl_index_pick_entries");
    ISL_HIP(hipMemcpyAsync(stage, queries, (size_t)nq * d * 4, hipMemcpyHostToDevice, st));
    dq = stage;
  }
  if (!packed) return fail(ISL_ERR_DEVICE, "hipMalloc failed in isl_index_pick_entries");
  isl_status r = isl::launch_entry_pick(idx, dq, nq, nullptr, nullptr, packed, nullptr, dout, st);
  // (the temporaries go when this returns: whatever was enqueued is drained first, also after a failure)
  hipError_t e = hipSuccess;
  if (r == ISL_OK && mem == ISL_MEM_HOST) e = hipMemcpyAsync(out_ids, dout, nq * 8, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);
  if (r != ISL_OK) return r;
  if (e != hipSuccess || es != hipSuccess)
    return fail(ISL_ERR_DEVICE, "isl_index_pick_entries failed: %s", hipGetErrorString(e != hipSuccess ? e : es));
  return ISL_OK;
}

}  // extern "C"
