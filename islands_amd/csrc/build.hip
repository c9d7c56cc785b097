// LeannIndex::build on the device (src/core/leann.rs:560-833), the step in front of the search
// path: nodes are inserted in id order; each insertion searches the graph built so far with
// ef_construction (search_layer_with_adjacency, :692-749 -- the search kernels of search.hip over
// fixed-width adjacency rows), selects neighbours with the high-degree-preserving rule
// (prune_with_degree_preservation_temp, :761-833) or plain truncation (:685), links them both
// ways (:592-607) and re-sorts a row by distance when it outgrows m0 (prune_neighbors_temp,
// :634-658).  `batch` nodes are inserted per step: with batch = 1 this IS the reference's
// sequential construction and the resulting CsrGraph is identical field by field (levels are
// an input because random_level draws from thread_rng, :549-554); with larger batches the
// searches of a step see the graph as of the step's start and the links of a step are applied
// under per-row locks in an unspecified order -- a throughput mode, same rules, no parity claim.
//
// ISL_SELECT_DIVERSE (isl_index_build_ex) swaps the two selections of that loop -- the new node's
// row and the re-selection of a row that outgrew m0 -- for the occlusion rule defined in
// include/islands_amd.h; everything else (order, construction search, locks, step ramp) is shared.
//
// isl_index_build_rows is the same construction over rows of either stored type.  bf16 rows (ISL_DTYPE_BF16)
// stay bf16 in the construction graph and in the finished index; the selection and link kernels take the row
// type as a template parameter and measure bf16 rows with the tile-free routine of device_common.hip.h over
// the exact f32 images, so the graph is the one built from the widened rows.
//
// isl_index_insert continues that loop at node `len` of a finished index, in place: the index's CSR returns to the
// construction table (csr_to_table_kernel), the rows of all nodes are the old table copied on the device plus the new
// rows, and the grown graph, built beside the old one, moves into the caller's handle at the end (adopt_grown).
// Build and insert are argument checks around one function, grow_flat.
//
// isl_index_remove takes nodes out of a finished index, in place: the lists return to the same table, one wave per
// survivor that lost a neighbour rebuilds its row from the OLD CSR (repair_kernel: the removed neighbours' own lists
// stand in for them; past m0 ids the builder's sort and selection decide), and the survivors' lists, rows and norms
// are compacted into a graph built beside the old one, which moves in as a grown one does.  The remap, the
// entry-point rule and the LDS size are remove_plan.hpp's.  The removal kernels read their graph as an array of
// layers (RemoveLayer, build_internal.hpp) -- one for a flat index -- and one host routine drives them
// (isl_build::shrink_import / shrink_finish, below the kernels): isl_index_remove calls it with its one layer,
// isl_hnsw_remove (hnsw_build.hip) with every layer of an HnswGraph, and each makes its own handle from the result.
//
// The HnswGraph builder (hnsw_build.hip) runs the same selection kernels and link_kernel's HNSW mode
// over one fixed-width table per layer.  Both go through one host path, isl_build::Scaffold
// (build_internal.hpp, defined below the kernels): the construction graph and everything allocated for
// it, "insert these nodes on this table", table -> CSR, one way out on failure.  The steps and the LDS
// sizes are build_plan.hpp's.
#include "device_common.hip.h"
#include "build_internal.hpp"
#include "hnsw_remove_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace {

using namespace isl_dev;

using isl_build::BuildParams;

// ---------------------------------------------------------------- ISL_SELECT_DIVERSE
// What a selection reads besides its lists: the rows and the rule's two parameters.
// ROWT = float, or uint16_t for bf16 bit patterns (stride in elements of it; norm2 is of the widened values).
template <typename ROWT>
struct SelCtxT {
  const ROWT* emb;
  const float* norm2;
  uint64_t stride;
  uint32_t d;
  float alpha;
  uint32_t keep_pruned;
};
using SelCtx = SelCtxT<float>;
template <typename ROWT>
constexpr bool kBf16 = sizeof(ROWT) == 2;

// LDS lists of one selection over up to `nmax` candidates, laid out behind the query.
struct SelState {
  uint32_t* cid;   // [nmax] candidate ids in ascending d(b, c), ties in their given order
  float* cd;       // [nmax] d(b, c)
  uint32_t* lst;   // [nmax] positions still undecided, ascending
  uint32_t* kept;  // [nmax] 1 = kept
  uint32_t* out;   // [M] the row: kept, then the fillers
};
using isl_plan::query_floats;  // (constexpr: the figure the host reserves is the one the kernels lay out by)
using isl_plan::query_floats_bf16;
template <typename ROWT = float>
__device__ __forceinline__ SelState sel_state(float* qs, uint32_t d, uint32_t nmax) {
  uint32_t* w = reinterpret_cast<uint32_t*>(qs + (kBf16<ROWT> ? query_floats_bf16(d) : query_floats(d)));
  SelState s;
  s.cid = w;
  s.cd = reinterpret_cast<float*>(w + nmax);
  s.lst = w + 2 * nmax;
  s.kept = w + 3 * nmax;
  s.out = w + 4 * nmax;
  return s;
}

// The row of node `id` as the query of the distance routines.  norm_a of cosine_distance
// (distance.rs:78) is the row's own sum of squares in element order, which the index keeps per row
// (norm2, the value load_query would add up again over d dependent steps).
template <int METRIC>
__device__ __forceinline__ float load_row_query(const SelCtx& c, uint32_t id, float* qs) {
  const float* q = c.emb + (uint64_t)id * c.stride;
  for (uint32_t j = threadIdx.x; j < c.d; j += 64) qs[j] = q[j];
  __syncthreads();
  return (METRIC == ISL_METRIC_COSINE || METRIC == METRIC_COSINE_PRE) ? c.norm2[id] : 0.0f;
}
// The same for a bf16 row: widened (exactly) into the f32 query area (widen_row_query, device_common.hip.h, which
// the HnswGraph builder's descent shares)
template <int METRIC>
__device__ __forceinline__ float load_row_query(const SelCtxT<uint16_t>& c, uint32_t id, float* qs) {
  widen_row_query(c.emb + (uint64_t)id * c.stride, c.d, qs);
  return (METRIC == ISL_METRIC_COSINE || METRIC == METRIC_COSINE_PRE) ? c.norm2[id] : 0.0f;
}

// select(b, C, M) of include/islands_amd.h for one wave, turned inside out: a candidate is kept
// iff no EARLIER KEPT one occludes it, so the head of the undecided list is always kept, its row
// becomes the query, and one pass of the exact-order distance routine over the rest of the list
// strikes what it occludes (ballot + prefix count compact the list in place).  At most M rounds
// over a shrinking list; a round costs what a hop of the search costs per 16 rows.  d(s, c) is
// calculate(vec[s], vec[c]) through the same chain as every other distance of the library.
// In: s.cid / s.cd [n] (written by the caller, not yet synchronised).  Out: s.out, count returned.
template <int METRIC, typename ROWT = float>
__device__ __forceinline__ uint32_t diverse_select(const SelCtxT<ROWT>& c, uint32_t n, uint32_t M,
                                                   const SelState& s, float* qs, float* tile) {
  const uint32_t lane = threadIdx.x;
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint32_t i = lane; i < n; i += 64) { s.lst[i] = i; s.kept[i] = 0u; }
  __syncthreads();
  uint32_t nl = n, nk = 0;
  while (nl > 0 && nk < M) {
    const uint32_t a = s.lst[0];
    const uint32_t aid = s.cid[a];
    if (lane == 0) { s.out[nk] = aid; s.kept[a] = 1u; }
    nk += 1;
    if (nk == M) break;
    if (nl == 1) { nl = 0; break; }
    __syncthreads();
    const float q_norm = load_row_query<METRIC>(c, aid, qs);
    uint32_t nn = 0;
    for (uint32_t base = 1; base < nl; base += 64) {
      const uint32_t cnt = nl - base < 64u ? nl - base : 64u;
      const bool valid = lane < cnt;
      const uint32_t pos = valid ? s.lst[base + lane] : 0u;
      const uint32_t rid = valid ? s.cid[pos] : aid;
      const float aux = (METRIC == METRIC_COSINE_PRE && valid) ? c.norm2[rid] : 0.0f;
      float ds;
      // bf16 rows: the tile-free routine (quad-owned rows, 16-byte loads of 8 elements, guarded tail) -- the
      // same contract, lane j < cnt gets row rid(j), and no tile
      if constexpr (kBf16<ROWT>) ds = direct_distances<METRIC, uint16_t>(c.emb, c.stride, c.d, rid, cnt, qs, q_norm, aux);
      else ds = wave_distances<METRIC>(c.emb, c.stride, c.d, rid, cnt, qs, tile, q_norm, aux);
      // occluded: alpha * d(s, c) <= d(b, c), separate roundings; false for a NaN on either side
      const bool stays = valid && !(c.alpha * ds <= s.cd[pos]);
      const uint64_t m = ballot(stays);
      // survivors of list slots 1 .. base + lane land at or below slot base + lane - 1, and every
      // lane has read its slot already: the list is compacted in place
      if (stays) s.lst[nn + (uint32_t)__popcll(m & below)] = pos;
      nn += (uint32_t)__popcll(m);
      __syncthreads();
    }
    nl = nn;
  }
  if (c.keep_pruned && nk < M) {
    // the list ran empty, so every candidate is decided: `dropped` is whatever is not kept
    __syncthreads();
    for (uint32_t base = 0; base < n && nk < M; base += 64) {
      const uint32_t i = base + lane;
      const bool dr = i < n && s.kept[i] == 0u;
      const uint64_t m = ballot(dr);
      const uint32_t at = nk + (uint32_t)__popcll(m & below);
      if (dr && at < M) s.out[at] = s.cid[i];
      nk += (uint32_t)__popcll(m);
      nk = nk < M ? nk : M;
    }
  }
  __syncthreads();
  return nk;
}

// prune_with_degree_preservation_temp, leann.rs:761-833, for one new node per wave.
__global__ __launch_bounds__(64) void select_kernel(BuildParams p) {
  extern __shared__ uint32_t sm[];
  const uint32_t lane = threadIdx.x, b = blockIdx.x;
  const uint32_t n = p.cand_cnt[b] < p.ef ? p.cand_cnt[b] : p.ef;
  const uint64_t* cid = p.cand_ids + (uint64_t)b * p.ef;
  uint32_t* ids = sm;            // [ef]
  uint32_t* deg = sm + p.ef;     // [ef]
  uint32_t* pos = sm + 2 * p.ef; // [ef] final position in the selection, or ~0
  uint32_t* out = p.sel + (uint64_t)b * p.m0;
  const uint64_t node = p.id0 + b;
  for (uint32_t i = lane; i < n; i += 64) {
    ids[i] = (uint32_t)cid[i];
    // degrees of the candidates in the graph built so far, :768-771 (0 for unknown ids)
    deg[i] = cid[i] < node ? p.ell_deg[cid[i]] : 0u;
  }
  __syncthreads();
  uint32_t nsel = 0;
  if (n <= p.m0 || !p.high_degree) {  // :764-766 / :685 truncate(max_connections)
    nsel = n < p.m0 ? n : p.m0;
    for (uint32_t i = lane; i < nsel; i += 64) out[i] = ids[i];
  } else {
    // hub threshold = degree at the top hub_percentile of the candidate degrees, :774-785
    const uint32_t hub_count = (uint32_t)ceilf((float)n * p.hub_percentile);
    uint32_t thr = 0xFFFFFFFFu;
    if (hub_count > 0 && hub_count < n) {
      // the hub_count-th largest value v: #{> v} < hub_count <= #{>= v}
      uint32_t found = 0xFFFFFFFFu;
      for (uint32_t i = lane; i < n; i += 64) {
        uint32_t gt = 0, ge = 0;
        for (uint32_t j = 0; j < n; ++j) { gt += deg[j] > deg[i]; ge += deg[j] >= deg[i]; }
        if (gt < hub_count && hub_count <= ge) found = deg[i];
      }
      for (int o = 32; o >= 1; o >>= 1) { uint32_t t = (uint32_t)__shfl_xor((int)found, o); found = found < t ? found : t; }
      thr = found;
    }
    const bool have = thr != 0xFFFFFFFFu;
    // hubs keep candidate order, then a stable sort by degree descending (:788-800); regular
    // candidates stay in ascending distance (:802, already sorted; ties keep their order)
    uint32_t nh = 0;
    for (uint32_t i = 0; i < n; ++i) nh += (have && deg[i] >= thr);  // uniform loop, n <= 512
    const uint32_t hub_slots = p.m0 / 4 > 1 ? p.m0 / 4 : 1;  // :807
    const uint32_t first_hubs = nh < hub_slots ? nh : hub_slots;
    for (uint32_t i = lane; i < n; i += 64) {
      const bool hub = have && deg[i] >= thr;
      uint32_t r = 0;
      if (hub) {  // rank among the hubs: larger degree first, equal degree in candidate order
        for (uint32_t j = 0; j < n; ++j)
          if (have && deg[j] >= thr) r += (deg[j] > deg[i]) || (deg[j] == deg[i] && j < i);
        // first hub_slots hubs lead, the rest follow every regular candidate (:808-830)
        pos[i] = r < hub_slots ? r : r + (n - nh);
      } else {
        for (uint32_t j = 0; j < i; ++j) r += !(have && deg[j] >= thr);
        pos[i] = first_hubs + r;
      }
    }
    __syncthreads();
    nsel = n < p.m0 ? n : p.m0;
    for (uint32_t i = lane; i < n; i += 64)
      if (pos[i] < p.m0) out[pos[i]] = ids[i];
  }
  if (lane == 0) p.sel_cnt[b] = nsel;
}

template <typename ROWT = float>
__device__ __forceinline__ SelCtxT<ROWT> sel_ctx(const BuildParams& p) {
  if constexpr (kBf16<ROWT>) return SelCtxT<ROWT>{p.emb16, p.norm2, p.stride, p.d, p.alpha, p.keep_pruned};
  else return SelCtxT<ROWT>{p.emb, p.norm2, p.stride, p.d, p.alpha, p.keep_pruned};
}

// ISL_SELECT_DIVERSE for one new node per wave: select(node, search result, m0), with the search's
// distances as d(node, c).  Over bf16 rows (ROWT = uint16_t) there is no tile: the query leads the LDS.
template <int METRIC_API, typename ROWT = float>
__global__ __launch_bounds__(64) void select_diverse_kernel(BuildParams p) {
  constexpr int METRIC = METRIC_API == ISL_METRIC_COSINE ? METRIC_COSINE_PRE : METRIC_API;
  extern __shared__ __align__(16) unsigned char smem[];
  float* tile = reinterpret_cast<float*>(smem);
  float* qs = tile + (kBf16<ROWT> ? 0 : TILE_ROWS * TILE_LD);
  const SelState s = sel_state<ROWT>(qs, p.d, p.ef);
  const uint32_t lane = threadIdx.x, b = blockIdx.x;
  const uint32_t n = p.cand_cnt[b] < p.ef ? p.cand_cnt[b] : p.ef;
  const uint64_t* cid = p.cand_ids + (uint64_t)b * p.ef;
  const float* cdist = p.cand_dist + (uint64_t)b * p.ef;
  for (uint32_t i = lane; i < n; i += 64) {
    s.cid[i] = (uint32_t)cid[i];
    s.cd[i] = cdist[i];
  }
  const uint32_t nsel = diverse_select<METRIC>(sel_ctx<ROWT>(p), n, p.m0, s, qs, tile);
  uint32_t* out = p.sel + (uint64_t)b * p.m0;
  for (uint32_t i = lane; i < nsel; i += 64) out[i] = s.out[i];
  if (lane == 0) p.sel_cnt[b] = nsel;
}

// isl_select_neighbors: d(base, c) for the candidates as given, a stable sort by it (the total
// order of ordkey: NaN last, -0 == +0), then the builder's routine.
struct SelectNeighborsParams {
  SelCtx c;
  const uint32_t* base_ids;  // [nb]
  const uint32_t* cand;      // [nb][pitch]
  const uint32_t* cand_cnt;  // [nb]
  uint32_t pitch, cap, nmax;
  uint32_t* out;             // [nb][cap]
  uint32_t* out_cnt;         // [nb]
};
template <int METRIC_API>
__global__ __launch_bounds__(64) void select_neighbors_kernel(SelectNeighborsParams p) {
  constexpr int METRIC = METRIC_API == ISL_METRIC_COSINE ? METRIC_COSINE_PRE : METRIC_API;
  extern __shared__ __align__(16) unsigned char smem[];
  float* tile = reinterpret_cast<float*>(smem);
  float* qs = tile + TILE_ROWS * TILE_LD;
  const SelState s = sel_state(qs, p.c.d, p.nmax);
  const uint32_t lane = threadIdx.x, b = blockIdx.x;
  const uint32_t n = p.cand_cnt[b] < p.nmax ? p.cand_cnt[b] : p.nmax;
  const uint32_t* cand = p.cand + (uint64_t)b * p.pitch;
  // the two lists the selection initialises itself hold the unsorted entries until then
  uint32_t* raw_id = s.lst;
  float* raw_d = reinterpret_cast<float*>(s.kept);
  const float q_norm = load_row_query<METRIC>(p.c, p.base_ids[b], qs);
  for (uint32_t base = 0; base < n; base += 64) {
    const uint32_t cnt = n - base < 64u ? n - base : 64u;
    const bool valid = lane < cnt;
    const uint32_t rid = valid ? cand[base + lane] : p.base_ids[b];
    const float aux = (METRIC == METRIC_COSINE_PRE && valid) ? p.c.norm2[rid] : 0.0f;
    const float ds = wave_distances<METRIC>(p.c.emb, p.c.stride, p.c.d, rid, cnt, qs, tile, q_norm, aux);
    if (valid) { raw_id[base + lane] = rid; raw_d[base + lane] = ds; }
  }
  __syncthreads();
  for (uint32_t i = lane; i < n; i += 64) {
    const uint32_t ki = ordkey(raw_d[i]);
    uint32_t r = 0;
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t kj = ordkey(raw_d[j]);
      r += (kj < ki) || (kj == ki && j < i);
    }
    s.cid[r] = raw_id[i];
    s.cd[r] = raw_d[i];
  }
  __syncthreads();
  const uint32_t nsel = diverse_select<METRIC>(p.c, n, p.cap, s, qs, tile);
  uint32_t* out = p.out + (uint64_t)b * p.cap;
  for (uint32_t i = lane; i < nsel; i += 64) out[i] = s.out[i];
  if (lane == 0) p.out_cnt[b] = nsel;
}

// adjacency.push(neighbors) + bidirectional links + prune_neighbors_temp, leann.rs:592-607, 634-658
// DIVERSE: a row that outgrew m0 is re-selected by the occlusion rule instead of cut at m0.
// HNSW: insert_node of HnswGraph on one layer (hnsw.rs:295-318): the step's nodes come from node_ids, a
// selected neighbour takes the back link only if it has the layer, the new id is appended without a
// `contains` test, and the reference rule's re-sort (prune_connections, :405-446) leaves the new id out --
// it looks every id up in the node map, which the node being inserted has not entered yet.
// ROWT = uint16_t: either builder over bf16 rows (no tile; norm_a of a row is its norm2, the bits the
// d-step sum over the widened values gives).
template <int METRIC_API, bool DIVERSE = false, bool HNSW = false, typename ROWT = float>
__global__ __launch_bounds__(64) void link_kernel(BuildParams p) {
  constexpr int METRIC = METRIC_API == ISL_METRIC_COSINE ? METRIC_COSINE_PRE : METRIC_API;
  extern __shared__ __align__(16) unsigned char smem[];
  float* tile = reinterpret_cast<float*>(smem);
  float* qs = tile + (kBf16<ROWT> ? 0 : TILE_ROWS * TILE_LD);
  const uint32_t lane = threadIdx.x, b = blockIdx.x;
  const uint32_t node = HNSW ? p.node_ids[b] : (uint32_t)(p.id0 + b);
  const uint32_t nsel = p.sel_cnt[b];
  const uint32_t* sel = p.sel + (uint64_t)b * p.m0;
  // adjacency.push(neighbors.clone()), :592
  for (uint32_t i = lane; i < nsel; i += 64) p.ell[(uint64_t)node * p.W + i] = sel[i];
  if (lane == 0) p.ell_deg[node] = nsel;
  if (HNSW && lane == 0 && nsel) p.cur_of[node] = sel[0];  // current = selected[0], hnsw.rs:316-318
  for (uint32_t t = 0; t < nsel; ++t) {
    const uint32_t nid = sel[t];
    if (HNSW && p.node_levels[nid] < p.layer) continue;  // hnsw.rs:305: no such layer, no back link
    if (p.locking) {
      if (lane == 0) while (atomicCAS(&p.lock[nid], 0u, 1u) != 0u) __builtin_amdgcn_s_sleep(1);
      __threadfence();
      __syncthreads();
    }
    uint32_t* row = p.ell + (uint64_t)nid * p.W;
    uint32_t dg = *((volatile uint32_t*)&p.ell_deg[nid]);
    bool has = false;
    if (!HNSW)
      for (uint32_t i = lane; i < dg; i += 64) has |= ((volatile uint32_t*)row)[i] == node;
    if (HNSW || !ballot(has)) {  // :596 if !adjacency[nid].contains(&id); HnswGraph pushes unconditionally
      if (lane == 0) row[dg] = node;
      dg += 1;
      if (dg > p.m0) {
        if (HNSW && !DIVERSE) dg = p.m0;  // the id just pushed (the last slot) is not a candidate
        // prune_neighbors_temp: distances from nid to every neighbour, stable sort, keep m0
        __threadfence_block();
        __syncthreads();
        float q_norm;
        if constexpr (kBf16<ROWT>) q_norm = load_row_query<METRIC>(sel_ctx<ROWT>(p), nid, qs);
        else q_norm = load_query<METRIC>(p.emb + (uint64_t)nid * p.stride, p.d, qs);
        // the row holds dg = m0 + 1 <= 129 ids: up to three slices of 64, one id per lane each
        constexpr int CH = 3;
        uint32_t rid[CH];
        float dist[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const uint32_t base = 64u * c;
          const uint32_t cnt = dg > base ? (dg - base < 64u ? dg - base : 64u) : 0u;
          rid[c] = lane < cnt ? ((volatile uint32_t*)row)[base + lane] : 0u;
          dist[c] = 0.0f;
          if (cnt) {
            const float aux = (METRIC == METRIC_COSINE_PRE && lane < cnt) ? p.norm2[rid[c]] : 0.0f;
            if constexpr (kBf16<ROWT>)
              dist[c] = direct_distances<METRIC, uint16_t>(p.emb16, p.stride, p.d, rid[c], cnt, qs, q_norm, aux);
            else
              dist[c] = wave_distances<METRIC>(p.emb, p.stride, p.d, rid[c], cnt, qs, tile, q_norm, aux);
          }
        }
        // stable sort by distance (`<` only, leann.rs:650): rank of every entry among all dg.
        // The diverse rule scatters by rank, so there the ranks must be a permutation whatever
        // the values: it compares through ordkey (the same order, with NaN as one greatest value).
        auto lt = [](float x, float y) {
          if constexpr (DIVERSE) return ordkey(x) < ordkey(y);
          else return x < y;
        };
        uint32_t rank[CH] = {0, 0, 0};
#pragma unroll
        for (int ci = 0; ci < CH; ++ci) {
          const uint32_t basei = 64u * ci;
          const uint32_t cnti = dg > basei ? (dg - basei < 64u ? dg - basei : 64u) : 0u;
          for (uint32_t l = 0; l < cnti; ++l) {
            const float di = rl_f(dist[ci], (int)l);
            const uint32_t i = basei + l;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
              const uint32_t me = 64u * c + lane;
              rank[c] += lt(di, dist[c]) || (!lt(dist[c], di) && !lt(di, dist[c]) && i < me);
            }
          }
        }
        __syncthreads();
        if constexpr (DIVERSE) {
          const SelState s = sel_state<ROWT>(qs, p.d, p.W);
#pragma unroll
          for (int c = 0; c < CH; ++c)
            if (64u * c + lane < dg) { s.cid[rank[c]] = rid[c]; s.cd[rank[c]] = dist[c]; }
          const uint32_t nk = diverse_select<METRIC>(sel_ctx<ROWT>(p), dg, p.m0, s, qs, tile);
          for (uint32_t i = lane; i < nk; i += 64) row[i] = s.out[i];
          dg = nk;
        } else {
#pragma unroll
          for (int c = 0; c < CH; ++c)
            if (64u * c + lane < dg && rank[c] < p.m0) row[rank[c]] = rid[c];
          dg = p.m0;
        }
      }
      if (lane == 0) *((volatile uint32_t*)&p.ell_deg[nid]) = dg;
    }
    if (p.locking) {
      __threadfence();
      __syncthreads();
      if (lane == 0) atomicExch(&p.lock[nid], 0u);
    }
  }
}

__global__ void ell_to_csr_kernel(const uint32_t* __restrict__ ell, const uint32_t* __restrict__ deg,
                                  uint32_t W, const uint64_t* __restrict__ off, uint64_t n,
                                  uint32_t* __restrict__ adj) {
  const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (row >= n) return;
  for (uint32_t i = lane; i < deg[row]; i += 64) adj[off[row] + i] = ell[row * W + i];
}

// The inverse, for a finished graph that takes more nodes (isl_index_insert, isl_hnsw_insert): one wave per row reads the
// row's CSR slice, lane after lane, into its table row and leaves the degree.  Lists of up to 128 ids take
// two slices of 64.  Nothing is written outside the row: what does not fit raises a flag instead.
__global__ __launch_bounds__(256) void csr_to_table_kernel(const uint64_t* __restrict__ off,
                                                           const uint32_t* __restrict__ adj, uint64_t nnz,
                                                           uint64_t n0, uint32_t W, uint32_t* __restrict__ ell,
                                                           uint32_t* __restrict__ deg, uint32_t* __restrict__ flag) {
  const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (row >= n0) return;
  const uint64_t s = off[row], e = off[row + 1];
  uint32_t dg = 0, bad = 0;
  if (e < s || e > nnz) bad = 2u;
  else if (e - s > W - 1) { bad = 1u; dg = W - 1; }
  else dg = (uint32_t)(e - s);
  for (uint32_t i = lane; i < dg; i += 64) {
    uint32_t id = adj[s + i];
    if (id >= n0) { bad |= 4u; id = 0; }
    ell[row * W + i] = id;
  }
  if (bad) atomicOr(flag, bad);
  if (lane == 0) deg[row] = dg;
}

__global__ void gather_rows_kernel(const float* __restrict__ emb, uint64_t stride, uint32_t d,
                                   uint64_t id0, uint32_t B, float* __restrict__ out) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)B * d) return;
  out[i] = emb[(id0 + i / d) * stride + i % d];
}
// ... from bf16 rows: the queries of a step are the widened rows.  One kernel for both builders: query i is node
// id0 + i (LeannIndex::build; node_ids NULL) or node_ids[i] (one layer of an HnswGraph under construction, which
// also takes where each query starts, as gather_layer_kernel of hnsw_build.hip leaves it for f32 rows)
__global__ void gather_rows_bf16_kernel(const uint16_t* __restrict__ emb, uint64_t stride, uint32_t d,
                                        uint64_t id0, const uint32_t* __restrict__ node_ids, uint32_t B,
                                        const uint32_t* __restrict__ cur_of, const uint32_t* __restrict__ evals_of,
                                        float* __restrict__ out, uint32_t* __restrict__ q_entry,
                                        uint32_t* __restrict__ q_evals) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (node_ids && i < B) {
    q_entry[i] = cur_of[node_ids[i]];
    q_evals[i] = evals_of[node_ids[i]];
  }
  if (i >= (uint64_t)B * d) return;
  const uint64_t node = node_ids ? node_ids[i / d] : id0 + i / d;
  out[i] = __uint_as_float((uint32_t)emb[node * stride + i % d] << 16);
}

// ---------------------------------------------------------------- isl_index_remove
using isl_plan::kGone;

using isl_build::RemoveLayer;
using isl_build::RepairParams;

// Survivors with at least one removed neighbour on a layer, as (layer, node) pairs in no particular order: one wave
// per row of every layer's old CSR (blockIdx.y = layer; a flat index is one layer without levels).  Runs after the
// import kernel has found every offset and id of the CSRs in range.  counts[0] = all pairs, counts[1 + L] = those of
// layer L; a pair past `cap` is counted and not written.
__global__ __launch_bounds__(256) void touched_kernel(const RemoveLayer* __restrict__ layers,
                                                      const uint32_t* __restrict__ levels,
                                                      const uint32_t* __restrict__ remap, uint64_t n0,
                                                      uint64_t* __restrict__ pairs, uint32_t cap,
                                                      uint32_t* __restrict__ counts) {
  const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63, layer = blockIdx.y;
  if (row >= n0 || remap[row] == kGone) return;
  if (levels && levels[row] < layer) return;  // no list on this layer
  const uint64_t* off = layers[layer].off;
  const uint32_t* adj = layers[layer].adj;
  const uint64_t s = off[row];
  const uint32_t dg = (uint32_t)(off[row + 1] - s);
  bool hit = false;
  for (uint32_t i = lane; i < dg; i += 64) hit |= remap[adj[s + i]] == kGone;
  if (ballot(hit) && lane == 0) {  // at most one pair per row and layer
    const uint32_t at = atomicAdd(counts, 1u);
    if (at < cap) pairs[at] = isl_plan::touched_pair(layer, (uint32_t)row);
    atomicAdd(counts + 1 + layer, 1u);
  }
}

// The repair of include/islands_amd.h for one touched (layer, node) pair per wave, over that layer's old CSR and
// M_L; a removed neighbour that lacks the layer has no list there.  C(p) is streamed from the old CSR into
// LDS: a surviving neighbour is one id on lane 0, a removed one its list in slices of 64; every slice is
// looked up in the ids taken so far (a list of the device CSR holds no id twice, so a slice needs no look at
// itself) and appended in lane order.  Nothing is written at or past kRemoveMaxCandidates, and the walk ends
// there.  |C| <= m0: the row is C.  Otherwise d(p, c) in slices of 64, the rank sort of
// select_neighbors_kernel (ordkey order: link_kernel's `<` order wherever no distance is a NaN, and a
// permutation whatever the values), then the first m0 or select().
template <int METRIC_API, bool DIVERSE, typename ROWT>
__global__ __launch_bounds__(64) void repair_kernel(RepairParams p) {
  constexpr int METRIC = METRIC_API == ISL_METRIC_COSINE ? METRIC_COSINE_PRE : METRIC_API;
  constexpr uint32_t CAP = isl_plan::kRemoveMaxCandidates;
  extern __shared__ __align__(16) unsigned char smem[];
  float* tile = reinterpret_cast<float*>(smem);
  float* qs = tile + (kBf16<ROWT> ? 0 : TILE_ROWS * TILE_LD);
  const SelState s = sel_state<ROWT>(qs, p.d, CAP);
  const uint32_t lane = threadIdx.x;
  const uint64_t below = (1ull << lane) - 1ull;
  const uint64_t pair = p.touched[blockIdx.x];
  const uint32_t node = isl_plan::pair_node(pair), layer = isl_plan::pair_layer(pair);
  const RemoveLayer ly = p.layers[layer];
  // the two lists the selection initialises itself hold the unsorted entries until then
  uint32_t* raw_id = s.lst;
  float* raw_d = reinterpret_cast<float*>(s.kept);
  uint32_t n = 0;
  auto take = [&](bool valid, uint32_t y) {
    bool fresh = valid;
    for (uint32_t j = 0; fresh && j < n; ++j) fresh = raw_id[j] != y;
    const uint64_t m = ballot(fresh);
    const uint32_t at = n + (uint32_t)__popcll(m & below);
    if (fresh && at < CAP) raw_id[at] = y;
    n += (uint32_t)__popcll(m);
    n = n < CAP ? n : CAP;
    __syncthreads();
  };
  const uint64_t ps = ly.off[node];
  const uint32_t pdeg = (uint32_t)(ly.off[node + 1] - ps);
  for (uint32_t t = 0; t < pdeg && n < CAP; ++t) {
    const uint32_t x = uni(ly.adj[ps + t]);
    if (p.remap[x] != kGone) {
      take(lane == 0, x);
    } else {
      const uint64_t xs = ly.off[x];
      const uint32_t xdeg = (p.levels && p.levels[x] < layer) ? 0u : (uint32_t)(ly.off[x + 1] - xs);
      for (uint32_t base = 0; base < xdeg && n < CAP; base += 64) {
        const bool in = base + lane < xdeg;
        const uint32_t y = in ? ly.adj[xs + base + lane] : 0u;
        take(in && y != node && p.remap[y] != kGone, y);
      }
    }
  }
  if (lane == 0) atomicAdd(p.total, (unsigned long long)n);
  uint32_t* row = ly.ell + (uint64_t)node * (ly.M + 1);
  if (n <= ly.M) {
    for (uint32_t i = lane; i < n; i += 64) row[i] = raw_id[i];
    if (lane == 0) ly.deg[node] = n;
    return;
  }
  const SelCtxT<ROWT> c{static_cast<const ROWT*>(p.emb), p.norm2, p.stride, p.d, p.alpha, p.keep_pruned};
  const float q_norm = load_row_query<METRIC>(c, node, qs);
  for (uint32_t base = 0; base < n; base += 64) {
    const uint32_t cnt = n - base < 64u ? n - base : 64u;
    const bool valid = lane < cnt;
    const uint32_t rid = valid ? raw_id[base + lane] : node;
    const float aux = (METRIC == METRIC_COSINE_PRE && valid) ? p.norm2[rid] : 0.0f;
    float ds;
    if constexpr (kBf16<ROWT>) ds = direct_distances<METRIC, uint16_t>(c.emb, c.stride, c.d, rid, cnt, qs, q_norm, aux);
    else ds = wave_distances<METRIC>(c.emb, c.stride, c.d, rid, cnt, qs, tile, q_norm, aux);
    if (valid) raw_d[base + lane] = ds;
  }
  __syncthreads();
  for (uint32_t i = lane; i < n; i += 64) {
    const uint32_t ki = ordkey(raw_d[i]);
    uint32_t r = 0;
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t kj = ordkey(raw_d[j]);
      r += (kj < ki) || (kj == ki && j < i);
    }
    s.cid[r] = raw_id[i];
    s.cd[r] = raw_d[i];
  }
  __syncthreads();
  uint32_t nk = ly.M;
  if constexpr (DIVERSE) {
    nk = diverse_select<METRIC>(c, n, ly.M, s, qs, tile);
    for (uint32_t i = lane; i < nk; i += 64) row[i] = s.out[i];
  } else {
    for (uint32_t i = lane; i < nk; i += 64) row[i] = s.cid[i];
  }
  if (lane == 0) ly.deg[node] = nk;
}

// Compaction of the lists: the table rows of the survivors, through the remap, into the new CSRs (one wave per old
// row and layer, blockIdx.y = layer).  A row of a node that lacks the layer is empty in the new CSR and is not
// read.  A removed id left in a survivor's row raises the flag and is not written as an id out of range.
__global__ __launch_bounds__(256) void table_to_csr_remap_kernel(const RemoveLayer* __restrict__ layers,
                                                                 const uint32_t* __restrict__ levels,
                                                                 const uint32_t* __restrict__ remap, uint64_t n0,
                                                                 uint32_t* __restrict__ flag) {
  const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63, layer = blockIdx.y;
  if (row >= n0) return;
  const uint32_t to = remap[row];
  if (to == kGone || (levels && levels[row] < layer)) return;
  const RemoveLayer ly = layers[layer];
  const uint32_t W = ly.M + 1;
  const uint32_t dg = ly.deg[row] < W ? ly.deg[row] : ly.M;
  const uint64_t at = ly.new_off[to];
  for (uint32_t i = lane; i < dg; i += 64) {
    uint32_t id = remap[ly.ell[row * W + i]];
    if (id == kGone) { atomicOr(flag, 1u); id = 0; }
    ly.new_adj[at + i] = id;
  }
}

// ... and of the rows: survivor `s` of the old table becomes row s of the new one, every element of the stride
// and the norm copied as bits
template <typename T>
__global__ __launch_bounds__(256) void gather_survivor_rows_kernel(const T* __restrict__ emb, uint64_t stride,
                                                                   const float* __restrict__ norm2,
                                                                   const uint32_t* __restrict__ survivors,
                                                                   T* __restrict__ out, float* __restrict__ out_norm2) {
  const uint64_t s = blockIdx.x;
  const uint64_t id = survivors[s];
  for (uint64_t j = threadIdx.x; j < stride; j += 256) out[s * stride + j] = emb[id * stride + j];
  if (threadIdx.x == 0) out_norm2[s] = norm2[id];
}

// ... and, for a reserved table that is compacted in place, one move of isl_plan::plan_row_moves: row dst_first + i
// of `dst` takes row src_ids[i] (src_ids NULL: row src_first + i) of `src`, every element of the stride and the norm
// copied as bits.  One wave per row at a time, 16-byte loads and stores along the row (rows are 16-byte aligned by
// the layout rule), 64-bit indexes.  `src` and `dst` may be the same block: the plan keeps the sources of a launch
// apart from its destinations, so neither is declared restrict.
template <typename T>
__global__ __launch_bounds__(256) void move_rows_kernel(const T* src, const float* src_norm2, const uint32_t* src_ids,
                                                        uint64_t src_first, T* dst, float* dst_norm2, uint64_t dst_first,
                                                        uint64_t count, uint64_t stride) {
  const uint64_t vecs = stride * sizeof(T) / 16;  // per row
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = (uint64_t)gridDim.x * 4;
  for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < count; i += waves) {
    const uint64_t from = src_ids ? (uint64_t)src_ids[i] : src_first + i, to = dst_first + i;
    const uint4* in = reinterpret_cast<const uint4*>(src + from * stride);
    uint4* out = reinterpret_cast<uint4*>(dst + to * stride);
    for (uint64_t v = lane; v < vecs; v += 64) out[v] = in[v];
    if (lane == 0) dst_norm2[to] = src_norm2[from];
  }
}

constexpr size_t kTileBytes = (size_t)TILE_ROWS * TILE_LD * 4;
// (bf16 rows: no tile)
size_t sel_lds(bool bf16, uint64_t d, uint32_t nmax, uint32_t M) {
  return bf16 ? isl_plan::select_lds_bf16((uint32_t)d, nmax, M) : isl_plan::select_lds(kTileBytes, (uint32_t)d, nmax, M);
}

// one wave per node of the step, the kernel instantiated for the index's metric and row type
template <bool DIVERSE, bool HNSW, typename ROWT = float>
void launch_link_as(uint32_t metric, uint32_t grid, size_t lds, const BuildParams& p) {
  isl::by_metric(metric, [&](auto mc) {
    hipLaunchKernelGGL((link_kernel<decltype(mc)::value, DIVERSE, HNSW, ROWT>), dim3(grid), dim3(64), lds, 0, p);
  });
}
void launch_link(uint32_t metric, bool diverse, bool hnsw, uint32_t grid, size_t lds, const BuildParams& p) {
  if (p.emb16) {  // bf16 rows, either builder
    if (!diverse && !hnsw) launch_link_as<false, false, uint16_t>(metric, grid, lds, p);
    else if (!hnsw) launch_link_as<true, false, uint16_t>(metric, grid, lds, p);
    else if (!diverse) launch_link_as<false, true, uint16_t>(metric, grid, lds, p);
    else launch_link_as<true, true, uint16_t>(metric, grid, lds, p);
  }
  else if (!diverse && !hnsw) launch_link_as<false, false>(metric, grid, lds, p);
  else if (!hnsw) launch_link_as<true, false>(metric, grid, lds, p);
  else if (!diverse) launch_link_as<false, true>(metric, grid, lds, p);
  else launch_link_as<true, true>(metric, grid, lds, p);
}
void launch_select_diverse(uint32_t metric, uint32_t grid, size_t lds, const BuildParams& p) {
  isl::by_metric(metric, [&](auto mc) {
    if (p.emb16)
      hipLaunchKernelGGL((select_diverse_kernel<decltype(mc)::value, uint16_t>), dim3(grid), dim3(64), lds, 0, p);
    else
      hipLaunchKernelGGL(select_diverse_kernel<decltype(mc)::value>, dim3(grid), dim3(64), lds, 0, p);
  });
}

// ---- the launches of a removal (shrink_finish below).  Each returns once the kernel is enqueued on the default
// stream.
// LDS of a repair launch whose widest layer keeps `widest` ids, for the rows' stored type
size_t repair_lds(const isl::RowTable& rows, uint32_t widest) {
  return rows.is_bf16() ? isl_plan::repair_lds_bf16((uint32_t)rows.d(), widest)
                        : isl_plan::repair_lds(kTileBytes, (uint32_t)rows.d(), widest);
}

// (layer, node) pairs of the survivors that lost a neighbour, all layers in one launch: d_counts [1 + layers],
// zeroed by the caller, receives the number of pairs and the pairs per layer; at most `cap` pairs are written.
isl_status list_touched(const RemoveLayer* d_layers, uint32_t layers, const uint32_t* d_levels, const uint32_t* d_remap,
                        uint64_t n0, uint64_t* d_pairs, uint32_t cap, uint32_t* d_counts) {
  hipLaunchKernelGGL(touched_kernel, dim3((uint32_t)((n0 + 3) / 4), layers), dim3(256), 0, 0, d_layers, d_levels, d_remap,
                     n0, d_pairs, cap, d_counts);
  if (hipGetLastError() != hipSuccess) return isl::fail(ISL_ERR_DEVICE, "listing the touched nodes failed");
  return ISL_OK;
}

// one wave per touched pair, the kernel instantiated for the graph's metric, the rule and the row type
isl_status launch_repair(uint32_t metric, bool diverse, const isl::RowTable& rows, uint32_t grid, size_t lds,
                         const RepairParams& p) {
  isl::by_metric(metric, [&](auto mc) {
    rows.with_row_type([&](auto row) {
      using T = decltype(row);
      if constexpr (!std::is_same<T, isl::fp8_e4m3>::value) {  // (the removals refuse fp8 rows)
        if (diverse) hipLaunchKernelGGL((repair_kernel<decltype(mc)::value, true, T>), dim3(grid), dim3(64), lds, 0, p);
        else hipLaunchKernelGGL((repair_kernel<decltype(mc)::value, false, T>), dim3(grid), dim3(64), lds, 0, p);
      }
    });
  });
  if (hipGetLastError() != hipSuccess) return isl::fail(ISL_ERR_DEVICE, "repair launch failed");
  return ISL_OK;
}

// the tables of layers 0 .. layers-1 -> their new CSRs through the remap, one launch; *d_flag (zeroed by the caller)
// is raised by a removed id left in a survivor's row
isl_status compact_lists(const RemoveLayer* d_layers, uint32_t layers, const uint32_t* d_levels, const uint32_t* d_remap,
                         uint64_t n0, uint32_t* d_flag) {
  hipLaunchKernelGGL(table_to_csr_remap_kernel, dim3((uint32_t)((n0 + 3) / 4), layers), dim3(256), 0, 0, d_layers,
                     d_levels, d_remap, n0, d_flag);
  if (hipGetLastError() != hipSuccess) return isl::fail(ISL_ERR_DEVICE, "CSR compaction failed");
  return ISL_OK;
}

// rows and norms of the n survivors d_surv[] (old ids, ascending), bit for bit, into `out`, a fresh table of the
// same stored type (row_table.hpp has the layout)
isl_status gather_survivors(const isl::RowTable& rows, const uint32_t* d_surv, uint64_t n, isl::RowTable& out) {
  if (out.allocate(rows.dtype(), n, rows.d()) != ISL_OK)
    return isl::fail(ISL_ERR_DEVICE, "hipMalloc failed for the rows of the shrunk graph");
  const uint64_t es = isl_rows::elem_size(rows.dtype());
  if (hipMemset(out.as<unsigned char>() + n * out.stride() * es, 0, (size_t)(isl_rows::slack(rows.dtype()) * es)) !=
      hipSuccess)
    return isl::fail(ISL_ERR_DEVICE, "hipMemset failed");
  rows.with_row_type([&](auto row) {
    using T = decltype(row);
    if constexpr (!std::is_same<T, isl::fp8_e4m3>::value)
      hipLaunchKernelGGL(gather_survivor_rows_kernel<T>, dim3((uint32_t)n), dim3(256), 0, 0, rows.as<const T>(),
                         rows.stride(), rows.norm2(), d_surv, out.as<T>(), out.norm2());
  });
  if (hipGetLastError() != hipSuccess) return isl::fail(ISL_ERR_DEVICE, "row compaction failed");
  return ISL_OK;
}

// ISL_DEBUG: where the time of one isl_index_insert / isl_index_remove goes.  mark(name) closes the phase that began
// at the previous mark (the device is drained first, so a phase owns its kernels); report() prints one stderr line,
// "[isl] <call> phases: name=ms ...", which tools/build_perf.py reads.  Without ISL_DEBUG nothing is timed or drained.
struct PhaseLog {
  bool on = false;
  std::chrono::steady_clock::time_point last;
  std::vector<std::pair<const char*, double>> phases;
  void start() {
    on = getenv("ISL_DEBUG") != nullptr;
    phases.clear();
    if (on) last = std::chrono::steady_clock::now();
  }
  void mark(const char* name) {
    if (!on) return;
    (void)hipDeviceSynchronize();
    const auto now = std::chrono::steady_clock::now();
    phases.emplace_back(name, std::chrono::duration<double, std::milli>(now - last).count());
    last = now;
  }
  void report(const char* call) {
    if (!on) return;
    std::string line;
    char buf[64];
    for (const auto& ph : phases) {
      snprintf(buf, sizeof(buf), " %s=%.3f", ph.first, ph.second);
      line += buf;
    }
    fprintf(stderr, "[isl] %s phases:%s\n", call, line.c_str());
    on = false;
  }
};
thread_local PhaseLog g_phases;

// What the in-place compaction of a reserved table needs, all of it allocated before the first move: the survivor
// list on the device, the plan and the staging buffer (rows at the table's stride, then their norms).
struct RowCompaction {
  std::vector<isl_plan::RowMove> moves;
  isl::DeviceBuffer<uint32_t> d_surv;       // [n] old ids, ascending
  isl::DeviceBuffer<unsigned char> stage;   // [stage_rows] rows, then [stage_rows] norms
  uint64_t stage_rows = 0, n = 0, n0 = 0;
};

isl_status prepare_row_compaction(const isl::RowTable& rows, const std::vector<uint32_t>& survivors, RowCompaction& c) {
  const uint64_t row_bytes = rows.stride() * isl_rows::elem_size(rows.dtype());
  c.n = survivors.size();
  c.n0 = rows.n();
  c.stage_rows = isl_plan::compact_stage_rows(row_bytes + 4, c.n, getenv("ISL_COMPACT_STAGE_ROWS"));
  isl_plan::plan_row_moves(survivors.data(), c.n, c.stage_rows, c.moves);
  bool staged = false;
  for (const isl_plan::RowMove& m : c.moves) staged = staged || m.staged;
  if (c.moves.empty()) return ISL_OK;
  ISL_TRY(c.d_surv.reserve(c.n));
  if (staged) ISL_TRY(c.stage.reserve(c.stage_rows * (row_bytes + 4)));
  if (hipMemcpy(c.d_surv, survivors.data(), c.n * 4, hipMemcpyHostToDevice) != hipSuccess)
    return isl::fail(ISL_ERR_DEVICE, "cannot upload the survivors");
  return ISL_OK;
}

// The moves, then the vacated tail [n, n0) zeroed; returns once the device is done.  Only a device failure
// interrupts it, and the table's rows are then undefined.
isl_status compact_rows_in_place(isl::RowTable& rows, const RowCompaction& c) {
  const uint64_t row_bytes = rows.stride() * isl_rows::elem_size(rows.dtype());
  rows.with_row_type([&](auto row) {
    using T = decltype(row);
    T* block = rows.as<T>();
    T* stage = reinterpret_cast<T*>(c.stage.get());
    float* stage_norm2 = stage ? reinterpret_cast<float*>(c.stage.get() + c.stage_rows * row_bytes) : nullptr;
    auto launch = [&](const T* src, const float* sn, const uint32_t* ids, T* dst, float* dn, uint64_t dst_first,
                      uint64_t count) {
      const uint32_t grid = (uint32_t)std::min<uint64_t>((count + 3) / 4, 1u << 20);
      hipLaunchKernelGGL(move_rows_kernel<T>, dim3(grid), dim3(256), 0, 0, src, sn, ids, (uint64_t)0, dst, dn, dst_first,
                         count, rows.stride());
    };
    for (const isl_plan::RowMove& m : c.moves) {
      const uint32_t* ids = c.d_surv.get() + m.first_new;
      if (!m.staged) {
        launch(block, rows.norm2(), ids, block, rows.norm2(), m.first_new, m.count);
      } else {
        launch(block, rows.norm2(), ids, stage, stage_norm2, 0, m.count);
        launch(stage, stage_norm2, nullptr, block, rows.norm2(), m.first_new, m.count);
      }
    }
  });
  if (hipGetLastError() != hipSuccess) return isl::fail(ISL_ERR_DEVICE, "row compaction launch failed");
  const uint64_t es = isl_rows::elem_size(rows.dtype());
  if (c.n0 > c.n &&
      (hipMemset(rows.as<unsigned char>() + c.n * rows.stride() * es, 0,
                 (size_t)(isl_rows::vacated_elems(rows.dtype(), rows.d(), c.n, c.n0) * es)) != hipSuccess ||
       hipMemset(rows.norm2() + c.n, 0, (size_t)(c.n0 - c.n) * 4) != hipSuccess))
    return isl::fail(ISL_ERR_DEVICE, "hipMemset failed");
  if (hipDeviceSynchronize() != hipSuccess) return isl::fail(ISL_ERR_DEVICE, "row compaction failed");
  return ISL_OK;
}
}  // namespace

namespace isl_build {

isl_status shrink_import(Scaffold& c, const std::vector<ShrinkLayer>& layers, uint64_t n0, ShrinkTables& t) {
  t.ly.resize(layers.size());
  ISL_TRY(c.alloc(&t.d_deg, layers.size() * n0, true));
  ISL_TRY(c.alloc(&t.d_flag, 3 + layers.size(), true));
  for (uint64_t L = 0; L < layers.size(); ++L) {
    const ShrinkLayer& in = layers[L];
    Table tab{nullptr, t.d_deg + L * n0, in.M};
    ISL_TRY(c.alloc(&tab.ell, n0 * (tab.M + 1)));
    t.ly[L] = RemoveLayer{in.off, in.adj, tab.ell, tab.deg, tab.M, 0u, nullptr, nullptr};
    ISL_TRY(c.csr_to_table(tab, in.off, in.adj, in.nnz, n0, t.d_flag));
  }
  return ISL_OK;
}

isl_status shrink_finish(Scaffold& c, ShrinkTables& t, const isl::RowTable& old_rows, uint32_t metric,
                         const isl_build_options& opts, const std::vector<uint32_t>& remap,
                         const std::vector<uint32_t>& survivors, const std::vector<uint64_t>& levels, bool has_entry,
                         uint64_t entry, uint64_t max_level, bool levels_name_layers, const char* call, Shrunk& out,
                         bool gather_rows) {
  using isl::fail;
  const uint64_t n0 = remap.size(), n = survivors.size(), layers = t.ly.size();
  std::vector<RemoveLayer>& ly = t.ly;
  out.entry = isl_plan::entry_after(levels, remap, survivors, has_entry, entry, max_level);
  // the layers above the new max_level cease to exist; layers that every node has all stay
  const uint64_t kept_layers = levels_name_layers ? isl_plan::layers_after(out.entry) : layers;
  // the rows that can hold a list bound the touched pairs
  const uint64_t pair_cap =
      levels_name_layers ? isl_plan::touched_capacity(isl_plan::layer_members(levels, survivors, layers)) : layers * n;
  if (pair_cap > 0xFFFFFFFFull) return fail(ISL_ERR_UNSUPPORTED, "%s: more than 2^32 lists", call);
  uint32_t widest = 0;
  for (const RemoveLayer& l : ly) widest = std::max(widest, l.M);

  uint32_t *d_counts = t.d_flag + 2, *d_remap = nullptr, *d_surv = nullptr, *d_lv = nullptr;
  uint64_t* d_pairs = nullptr;
  unsigned long long* d_total = nullptr;
  RemoveLayer* d_ly = nullptr;
  ISL_TRY(c.alloc(&d_total, 1, true));
  ISL_TRY(c.alloc(&d_remap, n0));
  ISL_TRY(c.alloc(&d_surv, n));
  ISL_TRY(c.alloc(&d_pairs, pair_cap));
  ISL_TRY(c.alloc(&d_ly, layers));
  std::vector<uint32_t> lv;  // what the kernels read "node has layer L" from; none: d_lv stays NULL
  if (levels_name_layers) {
    lv.assign(levels.begin(), levels.end());
    ISL_TRY(c.alloc(&d_lv, n0));
  }
  if (hipMemcpy(d_remap, remap.data(), n0 * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_surv, survivors.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess ||
      (d_lv && hipMemcpy(d_lv, lv.data(), n0 * 4, hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemcpy(d_ly, ly.data(), layers * sizeof(RemoveLayer), hipMemcpyHostToDevice) != hipSuccess)
    return fail(ISL_ERR_DEVICE, "cannot upload the remap");
  ISL_TRY(list_touched(d_ly, (uint32_t)layers, d_lv, d_remap, n0, d_pairs, (uint32_t)pair_cap, d_counts));
  out.counts.assign(layers + 1, 0);
  if (hipMemcpy(out.counts.data(), d_counts, (layers + 1) * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(ISL_ERR_DEVICE, "listing the touched lists failed");
  const uint32_t touched = out.counts[0];
  if (touched > pair_cap)
    return fail(ISL_ERR_DEVICE, "listing the touched lists failed: %u of %llu lists", touched, (unsigned long long)pair_cap);
  const bool debug = getenv("ISL_DEBUG") != nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (debug && touched && (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess)) ev0 = ev1 = nullptr;
  isl_status launched = ISL_OK;
  if (touched) {
    RepairParams p{};
    p.emb = old_rows.data(); p.norm2 = old_rows.norm2(); p.stride = old_rows.stride(); p.d = (uint32_t)old_rows.d();
    p.alpha = opts.alpha; p.keep_pruned = opts.keep_pruned ? 1u : 0u;
    p.layers = d_ly; p.levels = d_lv; p.remap = d_remap; p.touched = d_pairs; p.total = d_total;
    if (ev0) (void)hipEventRecord(ev0, 0);
    launched = launch_repair(metric, opts.select_rule == ISL_SELECT_DIVERSE, old_rows, touched,
                             repair_lds(old_rows, widest), p);
    if (ev1) (void)hipEventRecord(ev1, 0);
  }
  // the repaired degrees of every layer -> the offsets of the layers that are left (host scan, as table_to_csr)
  std::vector<uint32_t> hdeg(layers * n0);
  const bool read =
      launched == ISL_OK && hipMemcpy(hdeg.data(), t.d_deg, layers * n0 * 4, hipMemcpyDeviceToHost) == hipSuccess;
  if (debug && read) {
    (void)hipMemcpy(&out.candidates, d_total, 8, hipMemcpyDeviceToHost);
    if (ev0) (void)hipEventElapsedTime(&out.repair_ms, ev0, ev1);
  }
  if (ev0) { (void)hipEventDestroy(ev0); (void)hipEventDestroy(ev1); }
  ISL_TRY(launched);
  if (!read) return fail(ISL_ERR_DEVICE, "repair kernel failed");
  // layer 0: its own arrays (the core index copies them); the layers above: one block of offsets over ALL new
  // ids (a node below a layer has an empty row there, isl_hnsw_from_layers' shape) and one of ids, kept
  std::vector<uint64_t> hoff(kept_layers * (n + 1), 0);
  for (uint64_t L = 0; L < kept_layers; ++L) {
    uint64_t* o = hoff.data() + L * (n + 1);
    for (uint64_t i = 0; i < n; ++i) {
      const uint32_t s = survivors[i];
      o[i + 1] = o[i] + ((!d_lv || lv[s] >= L) ? std::min(hdeg[L * n0 + s], ly[L].M) : 0u);
    }
  }
  uint64_t upper_nnz = 0;
  for (uint64_t L = 1; L < kept_layers; ++L) upper_nnz += hoff[L * (n + 1) + n];
  uint64_t *d_off0 = nullptr, *d_off_up = nullptr;
  uint32_t *d_adj0 = nullptr, *d_adj_up = nullptr;
  ISL_TRY(c.alloc(&d_off0, n + 1));
  ISL_TRY(c.alloc(&d_adj0, hoff[n]));
  if (kept_layers > 1) {
    ISL_TRY(c.alloc(&d_off_up, (kept_layers - 1) * (n + 1), false, true));
    ISL_TRY(c.alloc(&d_adj_up, upper_nnz, false, true));
  }
  out.off.assign(kept_layers, nullptr);
  out.adj.assign(kept_layers, nullptr);
  out.off[0] = ly[0].new_off = d_off0;
  out.adj[0] = ly[0].new_adj = d_adj0;
  for (uint64_t L = 1, at = 0; L < kept_layers; ++L) {
    out.off[L] = ly[L].new_off = d_off_up + (L - 1) * (n + 1);
    out.adj[L] = ly[L].new_adj = d_adj_up + at;
    at += hoff[L * (n + 1) + n];
  }
  if (hipMemcpy(d_off0, hoff.data(), (n + 1) * 8, hipMemcpyHostToDevice) != hipSuccess ||
      (kept_layers > 1 && hipMemcpy(d_off_up, hoff.data() + (n + 1), (kept_layers - 1) * (n + 1) * 8,
                                    hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemcpy(d_ly, ly.data(), layers * sizeof(RemoveLayer), hipMemcpyHostToDevice) != hipSuccess)
    return fail(ISL_ERR_DEVICE, "cannot upload the CSR offsets");
  g_phases.mark("repair");
  ISL_TRY(compact_lists(d_ly, (uint32_t)kept_layers, d_lv, d_remap, n0, t.d_flag + 1));
  g_phases.mark("csr_export");
  if (gather_rows) ISL_TRY(gather_survivors(old_rows, d_surv, n, out.rows));
  g_phases.mark("rows");
  uint32_t flag = 0;
  if (hipMemcpy(&flag, t.d_flag + 1, 4, hipMemcpyDeviceToHost) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
    return fail(ISL_ERR_DEVICE, "compaction failed");
  if (flag) return fail(ISL_ERR_DEVICE, "%s: a repaired list kept a removed id", call);
  out.levels = isl_plan::levels_after(levels, survivors);
  return ISL_OK;
}

namespace {
// struct_size, rule and alpha of caller-supplied options
isl_status check_build_options(const isl_build_options* o, bool need_rule) {
  using isl::fail;
  if (o->struct_size < sizeof(isl_build_options))
    return fail(ISL_ERR_INVALID_ARGUMENT, "isl_build_options.struct_size %u is smaller than %zu", o->struct_size,
                sizeof(isl_build_options));
  if (need_rule && o->select_rule != ISL_SELECT_REFERENCE && o->select_rule != ISL_SELECT_DIVERSE)
    return fail(ISL_ERR_INVALID_ARGUMENT, "unknown selection rule %u", o->select_rule);
  if ((!need_rule || o->select_rule == ISL_SELECT_DIVERSE) && !(std::isfinite(o->alpha) && o->alpha >= 1.0f))
    return fail(ISL_ERR_INVALID_CONFIG, "Invalid configuration: alpha must be finite and >= 1");
  return ISL_OK;
}
}  // namespace

isl_status resolve_build_options(const isl_build_options* in, bool need_rule, isl_build_options& out) {
  isl_build_options_default(&out);
  if (in) {
    ISL_TRY(check_build_options(in, need_rule));
    out = *in;
  }
  return ISL_OK;
}

bool device_lists_differ(const isl_index* idx) {
  return idx->host_csr_valid && idx->node_offsets.size() == idx->num_nodes + 1 &&
         idx->node_offsets[idx->num_nodes] != idx->nnz;
}

void write_remap(const std::vector<uint32_t>* remap, uint64_t n0, uint64_t* out_remap) {
  if (!out_remap) return;
  for (uint64_t i = 0; i < n0; ++i)
    out_remap[i] = !remap ? i : (*remap)[i] == isl_plan::kGone ? ISL_REMOVED : (uint64_t)(*remap)[i];
}

size_t link_lds(uint64_t d) { return isl_plan::link_lds(kTileBytes, (uint32_t)d); }

isl_status check_row_dtype(int32_t dtype) {
  if (dtype != ISL_DTYPE_F32 && dtype != ISL_DTYPE_BF16) return isl::fail(ISL_ERR_INVALID_ARGUMENT, "unknown row dtype");
  return ISL_OK;
}

Scaffold::~Scaffold() {
  const isl::ErrorRecord first = isl::last_error();
  if (appended) (void)appended->zero_from(appended->n());  // a failed append: the rows behind the count are zero again
  keep.clear();
  isl_index_free(res);
  if (g) {  // the tables and per-query arrays it searched were borrowed from tmp, which goes after this body:
            // isl_index_free never sees them
    g->d_ell = nullptr; g->d_ell_deg = nullptr;
    g->build_q_entry = nullptr; g->build_q_evals = nullptr;
    isl_index_free(g);
  }
  isl::last_error() = first;
}

isl_status Scaffold::alloc_bytes(void** out, uint64_t bytes, bool zero, bool kept) {
  bytes = bytes ? bytes : 4;
  void* q = nullptr;
  if (!kept) q = tmp.alloc<unsigned char>(bytes);
  else if (keep.emplace_back().reserve(bytes) == ISL_OK) q = keep.back().get();
  if (!q) return isl::fail(ISL_ERR_DEVICE, "hipMalloc of %llu bytes failed for the builder", (unsigned long long)bytes);
  if (zero && hipMemset(q, 0, bytes) != hipSuccess) return isl::fail(ISL_ERR_DEVICE, "hipMemset failed");
  *out = q;
  return ISL_OK;
}

isl_status Scaffold::open(const isl_leann_config& cfg, const isl_build_options& opts, bool hnsw_, const void* vectors,
                          int32_t dtype, uint64_t n, uint64_t d, int32_t mem, int32_t device, uint64_t B, uint32_t m0,
                          uint32_t ef, const isl_index* old, isl::RowTable* into) {
  ISL_TRY(isl_index_new(&cfg, &g));
  g->cfg.prune_ratio = 0.0f;  // construction searches do not prune (leann.rs:692-749)
  g->host_csr_valid = false;
  g->num_nodes = n;
  g->device = device;
  g->has_dimension = true;
  g->dimension = d;
  g->max_degree = m0;  // the widest row a construction search can meet: a row is back at <= m0 ids before the next search
  if (into) {
    // a reserved table with room: the new rows and their norms go in behind the ones it holds, which are not written;
    // nothing else reads rows behind into->n() until the caller raises the count (after a failure the caller zeroes
    // them again).  The construction graph reads the table through a view of all n rows.
    const uint64_t n0 = into->n();
    ISL_TRY(isl::use_device(device));
    appended = into;
    ISL_TRY(into->fill(n0, n - n0, vectors, mem));
    g->rows = isl::RowTable::view_of(*into, n);
    g->nvec = n;
  }
  else if (old) ISL_TRY(isl::set_grown_embeddings(g, old, vectors, dtype, n - old->nvec, d, mem));
  else ISL_TRY(isl_set_embeddings(g, vectors, n, d, dtype, mem));
  // HnswGraph heap order: distance alone.  (Set once the rows are in: isl_set_embeddings refuses a caller who swaps
  // the rows of a facade's core index for another type; the builder's own graph takes the type it is given.)
  g->is_hnsw = hnsw_;
  hnsw = hnsw_;
  diverse = opts.select_rule == ISL_SELECT_DIVERSE;
  ISL_TRY(alloc(&p.lock, n, true));
  ISL_TRY(alloc(&qbuf, B * d));
  ISL_TRY(alloc(&cand_ids, B * ef));
  ISL_TRY(alloc(&cand_dist, B * ef));
  ISL_TRY(alloc(&cand_cnt, B));
  ISL_TRY(alloc(&p.sel, B * m0));
  ISL_TRY(alloc(&p.sel_cnt, B));
  p.emb = g->rows.f32(); p.emb16 = g->rows.bf16(); p.norm2 = g->rows.norm2(); p.stride = g->rows.stride();
  p.d = (uint32_t)d;
  p.ef = ef;
  p.cand_ids = cand_ids; p.cand_dist = cand_dist; p.cand_cnt = cand_cnt;
  if (!hnsw) { p.hub_percentile = cfg.hub_percentile; p.high_degree = cfg.high_degree_pruning; }
  p.alpha = opts.alpha; p.keep_pruned = opts.keep_pruned ? 1u : 0u;
  return ISL_OK;
}

isl_status Scaffold::insert(const Table& t, uint32_t cnt, bool locking, uint64_t id0, const uint32_t* node_ids,
                            uint32_t layer) {
  const uint64_t d = p.d;
  g->d_ell = t.ell;
  g->d_ell_deg = t.deg;
  g->ell_w = t.M + 1;
  ISL_TRY(isl::search_device_sync(g, qbuf, cnt, d, p.ef, p.ef, cand_ids, cand_dist, cand_cnt, nullptr));
  p.ell = t.ell; p.ell_deg = t.deg; p.W = t.M + 1; p.m0 = t.M;
  p.id0 = id0; p.node_ids = node_ids; p.layer = layer;
  p.B = cnt;
  p.locking = locking;
  const uint32_t metric = g->cfg.metric;
  const bool bf16 = p.emb16 != nullptr;
  if (diverse) {
    launch_select_diverse(metric, cnt, sel_lds(bf16, d, p.ef, t.M), p);
    launch_link(metric, true, hnsw, cnt, sel_lds(bf16, d, t.M + 1, t.M), p);
  } else {
    // the reference rule's selection does not measure: take(M), or the hub rule of LeannIndex::build
    hipLaunchKernelGGL(select_kernel, dim3(cnt), dim3(64), (size_t)p.ef * 12, 0, p);
    launch_link(metric, false, hnsw, cnt, bf16 ? isl_plan::link_lds_bf16((uint32_t)d) : link_lds(d), p);
  }
  if (hipGetLastError() != hipSuccess) return isl::fail(ISL_ERR_DEVICE, "builder launch failed");
  return ISL_OK;
}

void Scaffold::gather_bf16(uint64_t id0, uint32_t cnt, const uint32_t* node_ids, const uint32_t* cur_of,
                           const uint32_t* evals_of) {
  hipLaunchKernelGGL(gather_rows_bf16_kernel, dim3((uint32_t)(((uint64_t)cnt * p.d + 255) / 256)), dim3(256), 0, 0,
                     g->rows.bf16(), g->rows.stride(), p.d, id0, node_ids, cnt, cur_of, evals_of, qbuf, g->build_q_entry,
                     g->build_q_evals);
}

isl_status Scaffold::csr_to_table(const Table& t, const uint64_t* off, const uint32_t* adj, uint64_t nnz, uint64_t n0,
                                  uint32_t* d_flag) {
  if (!n0) return ISL_OK;
  hipLaunchKernelGGL(csr_to_table_kernel, dim3((uint32_t)((n0 + 3) / 4)), dim3(256), 0, 0, off, adj, nnz, n0, t.M + 1,
                     t.ell, t.deg, d_flag);
  if (hipGetLastError() != hipSuccess) return isl::fail(ISL_ERR_DEVICE, "table import launch failed");
  return ISL_OK;
}

isl_status Scaffold::table_to_csr(const Table& t, uint64_t n, bool kept, uint64_t** off, uint32_t** adj) {
  std::vector<uint32_t> hdeg(n);
  if (hipMemcpy(hdeg.data(), t.deg, n * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return isl::fail(ISL_ERR_DEVICE, "cannot read the degrees back");
  std::vector<uint64_t> hoff(n + 1, 0);
  for (uint64_t i = 0; i < n; ++i) hoff[i + 1] = hoff[i] + hdeg[i];
  ISL_TRY(alloc(off, n + 1, false, kept));
  ISL_TRY(alloc(adj, hoff[n], false, kept));
  if (hipMemcpy(*off, hoff.data(), (n + 1) * 8, hipMemcpyHostToDevice) != hipSuccess)
    return isl::fail(ISL_ERR_DEVICE, "cannot upload the CSR offsets");
  hipLaunchKernelGGL(ell_to_csr_kernel, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, 0, t.ell, t.deg, t.M + 1, *off, n,
                     *adj);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)
    return isl::fail(ISL_ERR_DEVICE, "CSR compaction failed");
  return ISL_OK;
}

isl_index* Scaffold::release() {
  isl_index* r = res;
  r->rows = std::move(g->rows);  // (a view, where the rows were appended in place)
  r->nvec = g->nvec;
  if (!r->rows.borrowed()) ++r->row_allocations;
  appended = nullptr;
  for (auto& b : keep) r->hnsw_owned.push_back(std::move(b));
  keep.clear();
  res = nullptr;
  return r;
}

}  // namespace isl_build

using isl_build::Scaffold;
using isl_build::Table;

extern "C" void isl_build_options_default(isl_build_options* o) {
  if (!o) return;
  o->struct_size = (uint32_t)sizeof(isl_build_options);
  o->select_rule = ISL_SELECT_REFERENCE;
  o->alpha = 1.0f;
  o->keep_pruned = 1;
  o->batch = 1;
}

extern "C" isl_status isl_index_build(const isl_leann_config* cfg, const float* vectors, uint64_t n, uint64_t d,
                                      const uint64_t* levels, uint64_t batch, int32_t mem, int32_t device,
                                      isl_index** out) {
  isl_build_options o;
  isl_build_options_default(&o);
  o.batch = batch;
  return isl_index_build_ex(cfg, &o, vectors, n, d, levels, mem, device, out);
}

extern "C" isl_status isl_index_build_ex(const isl_leann_config* cfg, const isl_build_options* opts,
                                         const float* vectors, uint64_t n, uint64_t d, const uint64_t* levels,
                                         int32_t mem, int32_t device, isl_index** out) {
  return isl_index_build_rows(cfg, opts, vectors, ISL_DTYPE_F32, n, d, levels, mem, device, out);
}

namespace {

// What `call` (isl_index_insert, isl_index_remove) refuses once the lists of `old` have returned to a table:
// *d_flag holds Scaffold::csr_to_table's bits, read here once.  Past this the CSR is in range.
isl_status check_import(const char* call, const uint32_t* d_flag, const isl_index* old) {
  using isl::fail;
  uint32_t flag = 0;
  if (hipMemcpy(&flag, d_flag, 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(ISL_ERR_DEVICE, "importing the index's lists failed");
  if (flag & 1u)
    return fail(ISL_ERR_UNSUPPORTED, "%s: the index has a list longer than m0 = %u", call, (uint32_t)old->cfg.m0);
  if (isl_build::device_lists_differ(old))
    return fail(ISL_ERR_UNSUPPORTED, "%s: the device copy of the graph is not the lists verbatim (ids repeated inside a "
                "list were removed at upload)", call);
  if (flag & 4u) return fail(ISL_ERR_UNSUPPORTED, "%s: a list names an id that is not below len = %llu", call,
                             (unsigned long long)old->num_nodes);
  if (flag) return fail(ISL_ERR_UNSUPPORTED, "%s: the index's offsets do not fit its lists", call);
  return ISL_OK;
}

// LeannIndex::build (leann.rs:578-615) for nodes n0 .. n-1 of a graph that holds n0 (`old`: a finished index
// with resident rows of `dtype`, whose CSR returns to the builder's table in its stored order and whose
// entry_point / max_level the loop continues from; NULL: nothing, node 0 starts the graph).  One loop over the
// plan's steps, then compaction.  `old` is only read; the graph of all n nodes leaves in `out`, built beside
// it, with the rows of all n nodes.  `into`: the reserved table of the handle that grows, with room for all n rows
// (NULL: a new table of exactly n rows); the new rows are appended to it and `out` leaves with a view of it.
// `levels`: of all n nodes, or empty (all 0).
isl_status grow_flat(const isl_leann_config& cfg, const isl_build_options& opts, const isl_index* old,
                     const void* vectors, int32_t dtype, uint64_t n_new, uint64_t d, const std::vector<uint64_t>& levels,
                     int32_t mem, int32_t device, isl::RowTable* into, isl_index** out) {
  using isl::fail;
  const uint64_t n0 = old ? old->num_nodes : 0, n = n0 + n_new;
  ISL_TRY(isl::use_device(device));
  // `levels` only name the entry point here (they are an input because random_level draws from thread_rng):
  // the steps are the planner's for all-zero levels, nodes in id order
  std::vector<isl_plan::Step> steps;
  {
    std::vector<uint32_t> order;
    isl_plan::plan_steps_from(std::vector<uint32_t>(n, 0u), n0 ? n0 : 1, 0u, opts.batch ? opts.batch : 1, steps, order);
  }
  const uint32_t m0 = (uint32_t)cfg.m0, ef = (uint32_t)cfg.ef_construction;

  Scaffold c;
  ISL_TRY(c.open(cfg, opts, false, vectors, dtype, n, d, mem, device, isl_plan::largest_step(steps), m0, ef, old, into));
  g_phases.mark("rows");
  Table t{nullptr, nullptr, m0};
  ISL_TRY(c.alloc(&t.ell, n * (m0 + 1)));
  ISL_TRY(c.alloc(&t.deg, n, true));
  isl_index* g = c.g;

  bool has_entry = old && old->has_entry;
  uint64_t entry = has_entry ? old->entry_point : 0, max_level = old ? old->max_level : 0;
  if (old) {
    // the finished lists return to the table; rows n0 .. n-1 keep degree 0
    uint32_t* d_flag = nullptr;
    ISL_TRY(c.alloc(&d_flag, 1, true));
    ISL_TRY(c.csr_to_table(t, old->d_off, old->d_adj, old->nnz, n0, d_flag));
    ISL_TRY(check_import("isl_index_insert", d_flag, old));
  }
  g_phases.mark("list_import");
  auto note_level = [&](uint64_t id) {  // :610-613
    const uint64_t lv = levels.empty() ? 0 : levels[id];
    if (!has_entry || lv > max_level) { has_entry = true; entry = id; max_level = lv; }
  };
  // node 0 of an empty graph: no neighbours (adjacency is empty, :585), becomes the entry point
  if (!n0) note_level(0);
  for (const isl_plan::Step& s : steps) {
    g->has_entry = true;
    g->entry_point = entry;  // :669: entry_point.unwrap_or(0) as of the start of the step
    const dim3 ggrid((uint32_t)((s.count * d + 255) / 256));
    if (g->rows.is_bf16())  // the step's queries are the widened rows
      c.gather_bf16(s.first, s.count);
    else
      hipLaunchKernelGGL(gather_rows_kernel, ggrid, dim3(256), 0, 0, g->rows.f32(), g->rows.stride(), (uint32_t)d,
                         s.first, s.count, c.qbuf);
    if (hipGetLastError() != hipSuccess) return fail(ISL_ERR_DEVICE, "gather launch failed");
    ISL_TRY(c.insert(t, s.count, s.count > 1, s.first));
    if (hipDeviceSynchronize() != hipSuccess) return fail(ISL_ERR_DEVICE, "builder kernels failed");
    for (uint64_t i = 0; i < s.count; ++i) note_level(s.first + i);
  }

  // flatten, :617-627
  uint64_t* d_off = nullptr;
  uint32_t* d_adj = nullptr;
  g_phases.mark("construction");
  ISL_TRY(c.table_to_csr(t, n, false, &d_off, &d_adj));
  g_phases.mark("csr_export");
  ISL_TRY(isl_index_from_device_csr(&cfg, device, n, d_off, d_adj, 1, entry, 1, d, &c.res));
  g_phases.mark("padded_adjacency");
  c.res->max_level = max_level;
  c.res->levels = levels;
  *out = c.release();
  return ISL_OK;
}

// What isl_index_insert does to the handle once the grown graph stands beside it (under idx->mu, no lane busy):
// every member that follows the node count takes the grown graph's value or goes.  Nothing here can fail.
// isl_index_remove moves its shrunk graph in the same way (`grown` is then the smaller one) and deals with the
// entry seeds itself.  `rows_in_place`: the rows of grown->nvec nodes already stand in the handle's reserved table
// (appended, or compacted), which stays where it is.
void adopt_grown(isl_index* idx, isl_index* grown, bool rows_in_place = false) {
  // host CSR (read back from the device on demand), levels, entry
  idx->host_csr_valid = grown->host_csr_valid;
  idx->node_offsets.swap(grown->node_offsets);
  idx->neighbors.swap(grown->neighbors);
  idx->levels.swap(grown->levels);
  idx->degree_counts.swap(grown->degree_counts);
  idx->num_nodes = grown->num_nodes;
  idx->has_entry = grown->has_entry;
  idx->entry_point = grown->entry_point;
  idx->max_level = grown->max_level;
  idx->has_dimension = grown->has_dimension;
  idx->dimension = grown->dimension;
  // device CSR and rows
  idx->device = grown->device;
  idx->d_off = std::move(grown->d_off);
  idx->d_adj = std::move(grown->d_adj);
  idx->nnz = grown->nnz;
  idx->max_degree = grown->max_degree;
  if (rows_in_place) {  // the handle's own reserved table: only its count follows
    idx->rows.set_n(grown->nvec);
  } else {
    idx->rows = std::move(grown->rows);
    if (idx->rows.resident()) ++idx->row_allocations;
  }
  idx->nvec = grown->nvec;
  idx->refine.reset();  // one row per node of the old graph
  // the padded adjacency of the old graph goes.  In its place comes the grown graph's, which
  // isl_index_from_device_csr has just made: the copy the next search would otherwise make again (absent when
  // there was no memory for it; the searches then pad on demand or stay on the CSR)
  idx->ell_copy = std::move(grown->ell_copy);
  idx->ell_deg_copy = std::move(grown->ell_deg_copy);
  idx->d_ell = idx->ell_copy; idx->d_ell_deg = idx->ell_deg_copy; idx->ell_w = grown->ell_w;
  grown->d_ell = nullptr; grown->d_ell_deg = nullptr;
  // vis_words / cand_cap follow the node count: the pool is made again on demand
  isl::free_exact_pool(idx->pool);
  // PQ codes no longer cover every node
  idx->pq = nullptr; idx->d_codes.reset(); idx->ncodes = 0;
  // kept: cfg, evals_hint, the entry seeds (ids and row copies of nodes the graph still has), the lanes (their
  // buffers follow nq, k, ef, d and the wave count of a call, never the node count)
}

}  // namespace

extern "C" isl_status isl_index_remove(isl_index* idx, const isl_build_options* opts_in, const uint64_t* ids,
                                       uint64_t n_ids, uint64_t* out_remap, uint64_t* out_len) {
  using isl::fail;
  if (!idx || (!ids && n_ids)) return fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  isl_build_options opts;
  ISL_TRY(isl_build::resolve_build_options(opts_in, true, opts));
  const uint64_t n0 = idx->num_nodes;
  if (n_ids == 0) {
    isl_build::write_remap(nullptr, n0, out_remap);
    if (out_len) *out_len = n0;
    return ISL_OK;
  }
  if (idx->is_hnsw)
    return fail(ISL_ERR_UNSUPPORTED, "isl_index_remove: this is the core index of an HnswGraph, which does not shrink");
  if (idx->recompute)
    return fail(ISL_ERR_UNSUPPORTED, "isl_index_remove: an index on the recompute provider does not give rows up");
  if (idx->rows.is_fp8())
    return fail(ISL_ERR_UNSUPPORTED, "isl_index_remove: the index holds fp8 rows, which the repair does not read");
  uint64_t bad = 0;
  if (isl_plan::first_unknown_id(ids, n_ids, n0, &bad)) return isl::fail_node(bad);
  const isl::RowTable& old_rows = idx->rows;
  if (idx->device < 0 || !idx->d_off || !old_rows.resident() || !old_rows.norm2() || old_rows.n() != n0 || idx->nvec != n0)
    return fail(ISL_ERR_UNSUPPORTED, "isl_index_remove needs the index's rows resident on the device "
                "(isl_index_upload, isl_set_embeddings)");
  if (idx->cfg.m0 > isl_plan::kMaxM0) return fail(ISL_ERR_UNSUPPORTED, "%s", isl_plan::shape_limit(idx->cfg.m0, 0, 0));
  {  // the &mut self of the reference: not beside a search on the same handle
    std::lock_guard<std::mutex> lock(idx->mu);
    if (isl::any_lane_busy(idx))
      return fail(ISL_ERR_SEARCH, "Search error: the index cannot shrink while searches are in flight");
  }
  std::vector<uint32_t> remap, survivors;
  const uint64_t n = isl_plan::build_remap(n0, ids, n_ids, remap, survivors);
  // a reserved table is compacted in place once the shrunk graph stands (below); one nobody reserved is left alone
  // and the survivors' rows are gathered into a new table beside it
  const bool in_place = old_rows.reserved();
  RowCompaction compaction;
  isl_index* shrunk = nullptr;
  // every node gone: what isl_index_build_rows gives for n == 0 under the handle's config
  if (n == 0) {
    ISL_TRY(isl_index_new(&idx->cfg, &shrunk));
  } else {
    // one layer that every node has: the levels only name the entry point.  `idx` is only read; the shrunk graph is
    // built beside it, with the survivors' rows.
    const uint32_t m0 = (uint32_t)idx->cfg.m0;
    ISL_TRY(isl::use_device(idx->device));
    Scaffold c;  // the staging buffers alone: no construction graph
    isl_build::ShrinkTables t;
    g_phases.start();
    ISL_TRY(isl_build::shrink_import(c, {{idx->d_off.get(), idx->d_adj.get(), idx->nnz, m0}}, n0, t));
    ISL_TRY(check_import("isl_index_remove", t.d_flag, idx));
    g_phases.mark("list_import");
    isl_build::Shrunk r;
    ISL_TRY(isl_build::shrink_finish(c, t, old_rows, idx->cfg.metric, opts, remap, survivors,
                                     idx->levels.size() == n0 ? idx->levels : std::vector<uint64_t>(), idx->has_entry,
                                     idx->entry_point, idx->max_level, false, "isl_index_remove", r, !in_place));
    if (getenv("ISL_DEBUG"))
      fprintf(stderr, "[isl] isl_index_remove: %llu of %llu nodes removed, touched %u, candidates %llu, repair kernel "
              "%.3f ms\n", (unsigned long long)(n0 - n), (unsigned long long)n0, r.counts[0], r.candidates, r.repair_ms);
    ISL_TRY(isl_index_from_device_csr(&idx->cfg, idx->device, n, r.off[0], r.adj[0], r.entry.has ? 1 : 0, r.entry.id,
                                      idx->has_dimension ? 1 : 0, idx->dimension, &c.res));
    g_phases.mark("padded_adjacency");
    c.res->max_level = r.entry.max_level;
    c.res->levels = std::move(r.levels);
    c.res->rows = std::move(r.rows);
    c.res->nvec = n;
    shrunk = c.res;
    c.res = nullptr;
  }
  if (in_place) {  // every allocation of the compaction, before the first move
    const isl_status st = n ? prepare_row_compaction(old_rows, survivors, compaction) : isl::use_device(idx->device);
    if (st != ISL_OK) {
      const isl::ErrorRecord keep = isl::last_error();
      isl_index_free(shrunk);
      isl::last_error() = keep;
      return st;
    }
  }
  // the entry seeds that survive, under their new ids
  std::vector<uint64_t> seeds;
  for (uint64_t s : idx->seeds.ids)
    if (s < n0 && remap[s] != isl_plan::kGone) seeds.push_back(remap[s]);
  // the move: the shrunk graph was built beside the old one, which nothing has touched so far
  {
    std::lock_guard<std::mutex> lock(idx->mu);
    if (isl::any_lane_busy(idx)) {
      isl_index_free(shrunk);
      return fail(ISL_ERR_SEARCH, "Search error: the index cannot shrink while searches are in flight");
    }
    if (in_place) {
      // the last step that can fail: the survivors' rows and norms move down inside the block, bit for bit, and the
      // vacated tail is zeroed.  Nothing has been moved before this; a device failure in it leaves the rows undefined.
      g_phases.mark("scaffold_free");
      const isl_status st = n ? compact_rows_in_place(idx->rows, compaction) : idx->rows.zero_from(0);
      g_phases.mark("rows_in_place");
      if (st != ISL_OK) {
        const isl::ErrorRecord keep = isl::last_error();
        isl_index_free(shrunk);
        isl::last_error() = keep;
        return st;
      }
    }
    const int32_t device = idx->device;
    adopt_grown(idx, shrunk, in_place);
    if (in_place) idx->device = device;  // (every node gone: the table stays where it is)
    idx->seeds = {};  // ids and row copies of the old numbering
  }
  isl_index_free(shrunk);  // what is left of it: the old graph's host vectors
  g_phases.mark("adopt");
  g_phases.report("isl_index_remove");
  // their rows are gathered again from the shrunk table; a table that cannot be made stays dropped, and a plain
  // search then starts at the entry point: the graph, the rows and the remap stand either way
  if (!seeds.empty() && isl_index_set_entry_seeds(idx, seeds.data(), seeds.size()) != ISL_OK) isl::last_error() = {};
  isl_build::write_remap(&remap, n0, out_remap);
  if (out_len) *out_len = n;
  return ISL_OK;
}

extern "C" isl_status isl_index_build_rows(const isl_leann_config* cfg_in, const isl_build_options* opts_in,
                                           const void* vectors, int32_t dtype, uint64_t n, uint64_t d,
                                           const uint64_t* levels, int32_t mem, int32_t device, isl_index** out) {
  using isl::fail;
  if (!out || (!vectors && n)) return fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  isl_build_options opts;
  ISL_TRY(isl_build::resolve_build_options(opts_in, true, opts));
  ISL_TRY(isl_build::check_row_dtype(dtype));
  isl_leann_config cfg;
  if (cfg_in) cfg = *cfg_in;
  else isl_leann_config_paper_default(&cfg);
  ISL_TRY(isl_leann_config_validate(&cfg));
  if (n == 0) return isl_index_new(&cfg, out);  // build(&[]) -> Ok(()), leann.rs:565-567
  if (d == 0) return fail(ISL_ERR_EMPTY_COLLECTION, "Empty vector collection");
  if (const char* why = isl_plan::shape_limit(cfg.m0, cfg.ef_construction, n)) return fail(ISL_ERR_UNSUPPORTED, "%s", why);
  std::vector<uint64_t> lv;
  if (levels) lv.assign(levels, levels + n);
  isl_index* built = nullptr;
  ISL_TRY(grow_flat(cfg, opts, nullptr, vectors, dtype, n, d, lv, mem, device, nullptr, &built));  // insert into nothing
  // ISL_ENTRY_SEEDS=N: the finished index leaves with N entry seeds selected (as isl_index_select_entry_seeds)
  const isl_status seeded = isl::env_entry_seeds(built);
  if (seeded != ISL_OK) {
    const isl::ErrorRecord keep = isl::last_error();
    isl_index_free(built);
    isl::last_error() = keep;
    return seeded;
  }
  *out = built;
  return ISL_OK;
}

extern "C" isl_status isl_index_insert(isl_index* idx, const isl_build_options* opts_in, const void* rows, int32_t dtype,
                                       uint64_t n_new, uint64_t d, const uint64_t* levels, int32_t mem,
                                       uint64_t* first_id) {
  using isl::fail;
  if (!idx || (!rows && n_new)) return fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  isl_build_options opts;
  ISL_TRY(isl_build::resolve_build_options(opts_in, true, opts));
  ISL_TRY(isl_build::check_row_dtype(dtype));
  const uint64_t n0 = idx->num_nodes;
  if (n_new == 0) {
    if (first_id) *first_id = n0;
    return ISL_OK;
  }
  if (idx->is_hnsw)
    return fail(ISL_ERR_UNSUPPORTED, "isl_index_insert: this is the core index of an HnswGraph, which grows through "
                "isl_hnsw_insert");
  if (idx->recompute)
    return fail(ISL_ERR_UNSUPPORTED, "isl_index_insert: an index on the recompute provider does not take rows");
  if (idx->rows.is_fp8())
    return fail(ISL_ERR_UNSUPPORTED, "isl_index_insert: the index holds fp8 rows, which the builder does not read");
  const isl::RowTable& old_rows = idx->rows;
  if (n0) {
    const bool known = idx->has_dimension || old_rows.resident();
    const uint64_t have = idx->has_dimension ? idx->dimension : old_rows.d();
    if (known && d != have) return isl::fail_dim(have, d);
  }
  if (d == 0) return fail(ISL_ERR_EMPTY_COLLECTION, "Empty vector collection");
  if (n0) {
    if (idx->device < 0 || !idx->d_off || !old_rows.resident() || !old_rows.norm2() || old_rows.n() != n0 ||
        idx->nvec != n0 || old_rows.d() != d)
      return fail(ISL_ERR_UNSUPPORTED, "isl_index_insert needs the index's rows resident on the device "
                  "(isl_index_upload, isl_set_embeddings)");
    if (old_rows.dtype() != dtype)
      return fail(ISL_ERR_UNSUPPORTED, "isl_index_insert: the index stores %s rows and takes no other type",
                  old_rows.is_bf16() ? "bf16" : "float32");
  }
  else if (old_rows.reserved() && old_rows.n() == 0) {  // an empty handle whose rows to come isl_index_reserve fixed
    if (old_rows.d() != d) return isl::fail_dim(old_rows.d(), d);
    if (old_rows.dtype() != dtype)
      return fail(ISL_ERR_UNSUPPORTED, "isl_index_insert: the index reserved %s rows and takes no other type",
                  old_rows.is_bf16() ? "bf16" : "float32");
  }
  const isl_leann_config cfg = idx->cfg;
  if (const char* why = isl_plan::shape_limit(cfg.m0, cfg.ef_construction, n0 + n_new))
    return fail(ISL_ERR_UNSUPPORTED, "%s", why);
  {  // the &mut self of the reference: not beside a search on the same handle
    std::lock_guard<std::mutex> lock(idx->mu);
    if (isl::any_lane_busy(idx))
      return fail(ISL_ERR_SEARCH, "Search error: the index cannot grow while searches are in flight");
  }
  // a reserved table with room takes the new rows in place; one without it is used up: a new table of exactly
  // n0 + n_new rows, as for an index nobody reserved
  const bool in_place = old_rows.reserved() && old_rows.resident() && old_rows.n() == n0 && old_rows.d() == d &&
                        old_rows.dtype() == dtype && n0 + n_new <= old_rows.capacity();
  // levels of all nodes: the index's (all 0 where it keeps none), then the new nodes'
  std::vector<uint64_t> lv(n0 + n_new, 0);
  if (idx->levels.size() == n0) std::copy(idx->levels.begin(), idx->levels.end(), lv.begin());
  if (levels) std::copy(levels, levels + n_new, lv.begin() + n0);
  isl_index* grown = nullptr;
  g_phases.start();
  ISL_TRY(grow_flat(cfg, opts, n0 ? idx : nullptr, rows, dtype, n_new, d, lv, mem,
                    idx->device >= 0 ? idx->device : 0, in_place ? &idx->rows : nullptr, &grown));
  // the move: the grown graph was built beside the old one, which nothing has touched so far
  {
    std::lock_guard<std::mutex> lock(idx->mu);
    if (isl::any_lane_busy(idx)) {
      if (in_place) (void)idx->rows.zero_from(n0);  // the appended rows, which no search reads
      isl_index_free(grown);
      return fail(ISL_ERR_SEARCH, "Search error: the index cannot grow while searches are in flight");
    }
    adopt_grown(idx, grown, in_place);
  }
  isl_index_free(grown);  // what is left of it: the old graph's host vectors
  g_phases.mark("adopt");
  g_phases.report("isl_index_insert");
  if (first_id) *first_id = n0;
  return ISL_OK;
}

extern "C" isl_status isl_select_neighbors(const isl_index* idx, const isl_build_options* opts_in,
                                           const uint64_t* base_ids, uint64_t nb, const uint64_t* cand_ids,
                                           uint64_t pitch, const uint32_t* cand_cnt, uint64_t cap,
                                           uint64_t* out_ids, uint32_t* out_cnt) {
  using isl::fail;
  if (!idx || (nb && (!base_ids || !cand_cnt || !out_ids || !out_cnt || (!cand_ids && pitch))))
    return fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  isl_build_options opts;
  ISL_TRY(isl_build::resolve_build_options(opts_in, false, opts));
  if (cap == 0 || cap > isl_plan::kMaxM0) return fail(ISL_ERR_UNSUPPORTED, "isl_select_neighbors: 1 <= cap <= 128");
  if (nb == 0) return ISL_OK;
  if (nb > 0x7FFFFFFFull) return fail(ISL_ERR_UNSUPPORTED, "isl_select_neighbors: too many base nodes");
  if (idx->recompute || !idx->rows.f32() || idx->device < 0)
    return fail(ISL_ERR_UNSUPPORTED, "isl_select_neighbors needs float32 rows resident on the device");
  uint32_t nmax = 1;
  for (uint64_t i = 0; i < nb; ++i) {
    if (cand_cnt[i] > isl_plan::kMaxEfConstruction || cand_cnt[i] > pitch)
      return fail(ISL_ERR_UNSUPPORTED, "isl_select_neighbors: cand_cnt <= min(pitch, 512)");
    nmax = std::max(nmax, cand_cnt[i]);
  }
  // ids leave the host as the 32-bit ids of the device tables
  std::vector<uint32_t> hbase(nb), hcand((size_t)nb * nmax, 0u);
  for (uint64_t i = 0; i < nb; ++i) {
    if (base_ids[i] >= idx->nvec) return isl::fail_node(base_ids[i]);
    hbase[i] = (uint32_t)base_ids[i];
    for (uint32_t j = 0; j < cand_cnt[i]; ++j) {
      const uint64_t c = cand_ids[i * pitch + j];
      if (c >= idx->nvec) return isl::fail_node(c);
      hcand[(size_t)i * nmax + j] = (uint32_t)c;
    }
  }
  ISL_TRY(isl::use_device(idx->device));
  Scaffold c;  // the staging buffers alone: no construction graph
  SelectNeighborsParams p{};
  uint32_t *d_base = nullptr, *d_cand = nullptr, *d_cnt = nullptr;
  ISL_TRY(c.alloc(&d_base, nb));
  ISL_TRY(c.alloc(&d_cand, nb * nmax));
  ISL_TRY(c.alloc(&d_cnt, nb));
  ISL_TRY(c.alloc(&p.out, nb * cap, true));
  ISL_TRY(c.alloc(&p.out_cnt, nb));
  if (hipMemcpy(d_base, hbase.data(), nb * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_cand, hcand.data(), (size_t)nb * nmax * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_cnt, cand_cnt, nb * 4, hipMemcpyHostToDevice) != hipSuccess)
    return fail(ISL_ERR_DEVICE, "cannot stage the candidates");
  const isl::RowTable& rows = idx->rows;
  p.c = SelCtx{rows.f32(), rows.norm2(), rows.stride(), (uint32_t)rows.d(), opts.alpha, opts.keep_pruned ? 1u : 0u};
  p.base_ids = d_base; p.cand = d_cand; p.cand_cnt = d_cnt;
  p.pitch = nmax; p.cap = (uint32_t)cap; p.nmax = nmax;
  isl::by_metric(idx->cfg.metric, [&](auto mc) {
    hipLaunchKernelGGL(select_neighbors_kernel<decltype(mc)::value>, dim3((uint32_t)nb), dim3(64),
                       sel_lds(false, rows.d(), nmax, (uint32_t)cap), 0, p);
  });
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)
    return fail(ISL_ERR_DEVICE, "select_neighbors kernel failed");
  std::vector<uint32_t> hout((size_t)nb * cap);
  if (hipMemcpy(hout.data(), p.out, (size_t)nb * cap * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(out_cnt, p.out_cnt, nb * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(ISL_ERR_DEVICE, "cannot read the selection back");
  for (size_t i = 0; i < hout.size(); ++i) out_ids[i] = hout[i];
  return ISL_OK;
}
