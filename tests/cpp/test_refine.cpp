// C++ checks of LeannIndex::set_refine_rows / refine_storage / search_refined_batch / rescore
// (include/islands_amd.hpp over isl_index_set_refine_rows, isl_index_refine_storage, isl_search_refined_batch and
// isl_rescore).  `test_refine cpu`: what is answered without a device; `test_refine gpu`: a 300-row index built on
// the device, narrowed to fp8, refined against its f32 rows kept in pinned host memory.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "islands_amd.hpp"

using namespace islands::core;

static int failures = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)

template <class F>
static bool throws(isl_status st, F f) {
  try { f(); } catch (const CoreError& e) { return e.status == st; }
  return false;
}

static CsrGraph ring(uint64_t n) {
  CsrGraph g;
  g.num_nodes = n;
  g.node_offsets.assign(1, 0);
  for (uint64_t i = 0; i < n; ++i) {
    g.neighbors.push_back((i + 1) % n);
    g.node_offsets.push_back(g.neighbors.size());
  }
  g.levels.assign(n, 0);
  g.degree_counts.assign(n, 1);
  g.entry_point = 0;
  return g;
}

// euclidean_distance of the reference: one sequential f32 sum, then the square root
static float euclid(const float* a, const float* b, uint64_t d) {
  volatile float sum = 0.0f;
  for (uint64_t j = 0; j < d; ++j) {
    volatile float diff = a[j] - b[j];
    volatile float sq = diff * diff;
    sum = sum + sq;
  }
  return std::sqrt((float)sum);
}

static uint32_t bits(float v) {
  uint32_t u;
  std::memcpy(&u, &v, 4);
  return u;
}

int main(int argc, char** argv) {
  const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
  LeannConfig cfg;
  cfg.m = 8; cfg.m0 = 16; cfg.ef_construction = 40; cfg.metric = ISL_METRIC_EUCLIDEAN;
  {
    LeannIndex host = LeannIndex::from_csr(ring(5), cfg, 4);  // never uploaded
    const std::vector<float> rows(5 * 4, 1.0f), q(2 * 4, 0.5f);
    EXPECT(isl_index_set_refine_rows(nullptr, rows.data(), 5, 4, ISL_DTYPE_F32, ISL_MEM_HOST, ISL_REFINE_HOST) ==
           ISL_ERR_INVALID_ARGUMENT);
    EXPECT(isl_index_set_refine_rows(host.handle(), rows.data(), 5, 4, 7, ISL_MEM_HOST, ISL_REFINE_HOST) == ISL_ERR_INVALID_ARGUMENT);
    EXPECT(isl_index_set_refine_rows(host.handle(), rows.data(), 5, 4, ISL_DTYPE_FP8_E4M3, ISL_MEM_HOST, ISL_REFINE_HOST) ==
           ISL_ERR_UNSUPPORTED);
    EXPECT(throws(ISL_ERR_UNSUPPORTED, [&] { host.set_refine_rows(rows, 5, ISL_REFINE_HOST); }));  // not on a device
    const RefineStorage none = host.refine_storage();
    EXPECT(none.rows == 0 && none.block_bytes == 0 && none.dtype == ISL_DTYPE_F32 && none.placement == ISL_REFINE_DEVICE);
    EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { host.search_refined_batch(q, 2, 1, 8); }));  // no table
    EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { host.rescore(q, 2, {0, 1, 2, 3}, {2, 2}, 1); }));
    static_assert(ISL_REFINE_MAX_CANDIDATES == 512u, "the cap of the header");
  }
  if (gpu) {
    const uint64_t n = 300, d = 24, nq = 32, k = 10, ef = 64, cand = 32;
    std::mt19937 rng(17);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    std::vector<float> x(n * d), q(nq * d);
    for (float& v : x) v = u(rng);
    for (float& v : q) v = u(rng);
    LeannIndex idx = LeannIndex::build(x, n, d, cfg);
    EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { idx.set_refine_rows(std::vector<float>(x.begin(), x.end() - d), n - 1); }));
    idx.set_refine_rows(x, n, ISL_REFINE_HOST);
    idx.convert_rows(ISL_DTYPE_FP8_E4M3);  // build, set, narrow: the table stays
    RefineStorage st = idx.refine_storage();
    EXPECT(st.rows == n && st.placement == ISL_REFINE_HOST && st.dtype == ISL_DTYPE_F32 && st.block_bytes == (n * d + 256) * 4);
    EXPECT(idx.row_storage().dtype == ISL_DTYPE_FP8_E4M3);
    // the refined answer is the rescoring of the plain search's candidates, with distances to the ORIGINAL rows
    std::vector<uint64_t> cids(nq * cand);
    std::vector<float> cdist(nq * cand);
    std::vector<uint32_t> ccnt(nq);
    EXPECT(isl_search_batch(idx.handle(), q.data(), nq, d, cand, ef, cids.data(), cdist.data(), ccnt.data()) == ISL_OK);
    const BatchAnswer a = idx.search_refined_batch(q, nq, k, ef, cand);
    const BatchAnswer b = idx.rescore(q, nq, cids, ccnt, k);
    uint64_t hits_plain = 0, hits_refined = 0;
    for (uint64_t i = 0; i < nq; ++i) {
      EXPECT(a.count[i] == k && b.count[i] == k);
      // the exact top-k of query i, by hand
      std::vector<std::pair<float, uint64_t>> all(n);
      for (uint64_t r = 0; r < n; ++r) all[r] = {euclid(&q[i * d], &x[r * d], d), r};
      std::sort(all.begin(), all.end());
      for (uint64_t j = 0; j < k; ++j) {
        EXPECT(a.ids[i * k + j] == b.ids[i * k + j] && bits(a.dist[i * k + j]) == bits(b.dist[i * k + j]));
        const uint64_t id = a.ids[i * k + j];
        EXPECT(id < n && bits(a.dist[i * k + j]) == bits(euclid(&q[i * d], &x[id * d], d)));
        if (j) EXPECT(a.dist[i * k + j - 1] <= a.dist[i * k + j]);
        for (uint64_t t = 0; t < k; ++t) {
          hits_refined += all[t].second == id;
          hits_plain += all[t].second == cids[i * cand + j];
        }
      }
    }
    std::printf("recall@10 plain fp8 %.4f refined %.4f\n", hits_plain / double(nq * k), hits_refined / double(nq * k));
    EXPECT(hits_refined >= hits_plain);
    // an id that names no row is skipped, equal rows go to the earlier position
    const BatchAnswer c = idx.rescore(std::vector<float>(q.begin(), q.begin() + d), 1, {n + 5, 7, 7, 3}, {4}, 4);
    EXPECT(c.count[0] == 3 && c.ids[0] + c.ids[1] + c.ids[2] == 17 && c.dist[0] <= c.dist[1] && c.dist[1] <= c.dist[2]);
    EXPECT(throws(ISL_ERR_UNSUPPORTED, [&] { idx.search_refined_batch(q, nq, k, 600, 513); }));
    EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { idx.search_refined_batch(q, nq, k, 16, 17); }));
    // a bf16 table on the device replaces it; rows that change the node count drop it
    std::vector<uint16_t> xb(n * d);
    for (uint64_t i = 0; i < n * d; ++i) xb[i] = (uint16_t)(bits(x[i]) >> 16);  // (truncated: any bf16 pattern is a row)
    idx.set_refine_rows_bf16(xb, n);
    st = idx.refine_storage();
    EXPECT(st.rows == n && st.placement == ISL_REFINE_DEVICE && st.dtype == ISL_DTYPE_BF16);
    EXPECT(idx.search_refined_batch(q, nq, k, ef).count[0] == k);  // candidates default to min(ef, 512)
    idx.convert_rows(ISL_DTYPE_F32);
    idx.insert(std::vector<float>(x.begin(), x.begin() + 4 * d), 4, d);
    EXPECT(idx.refine_storage().rows == 0);
    EXPECT(throws(ISL_ERR_INVALID_ARGUMENT, [&] { idx.search_refined_batch(q, nq, k, ef, cand); }));
    idx.set_refine_rows(std::vector<float>((n + 4) * d, 0.25f), n + 4);
    idx.set_refine_rows({}, 0);  // n == 0 drops it
    EXPECT(idx.refine_storage().rows == 0);
  }
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("test_refine %s ok\n", gpu ? "gpu" : "cpu");
  return 0;
}
