// islands_amd.hpp -- C++ host-side mirror of `islands::core` over the C ABI (islands_amd.h).
//
// The reference is compiled code (Rust) and its toolchain is absent from the build image, so
// the host side above the C ABI is mirrored in C++: same type and method names, argument
// meaning and error behaviour as src/core/{leann,distance,error}.rs.  Header-only; link with
// -lislands_amd.  CoreError variants become the `kind` of one exception type.
#pragma once

#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "islands_amd.h"

namespace islands::core {

// CoreError, src/core/error.rs:9-62
struct CoreError : std::runtime_error {
  isl_status status;
  uint64_t expected, actual, node;
  CoreError(isl_status s, const std::string& msg, uint64_t e = 0, uint64_t a = 0, uint64_t n = 0)
      : std::runtime_error(msg), status(s), expected(e), actual(a), node(n) {}
  std::string kind() const { return isl_status_name(status); }
};

inline void check(isl_status s) {
  if (s != ISL_OK)
    throw CoreError(s, isl_last_error_message(), isl_last_error_expected(),
                    isl_last_error_actual(), isl_last_error_node());
}

// DistanceMetric, src/core/distance.rs:9-19
enum class DistanceMetric : int32_t { Cosine = 0, Euclidean = 1, DotProduct = 2, Manhattan = 3 };
// PruningStrategy, src/core/leann.rs:168-178
enum class PruningStrategy : uint32_t { Global = 0, Local = 1, Proportional = 2 };

// Distance trait, src/core/distance.rs:22-35
inline float calculate(DistanceMetric m, const std::vector<float>& a, const std::vector<float>& b) {
  float out = 0;
  check(isl_distance((int32_t)m, a.data(), a.size(), b.data(), b.size(), &out));
  return out;
}
inline float calculate_squared(DistanceMetric m, const std::vector<float>& a,
                               const std::vector<float>& b) {
  float out = 0;
  check(isl_distance_squared((int32_t)m, a.data(), a.size(), b.data(), b.size(), &out));
  return out;
}
// rows: n contiguous rows of row_len floats
inline std::vector<float> batch_calculate(DistanceMetric m, const std::vector<float>& query,
                                          const std::vector<float>& rows, uint64_t row_len,
                                          int32_t device = 0) {
  uint64_t n = row_len ? rows.size() / row_len : 0;
  std::vector<float> out(n);
  check(isl_distance_batch((int32_t)m, query.data(), query.size(), rows.data(), n, row_len,
                           out.data(), ISL_MEM_HOST, device, nullptr));
  return out;
}

// LeannConfig, src/core/leann.rs:322-461
struct LeannConfig : isl_leann_config {
  LeannConfig() { isl_leann_config_paper_default(this); }
  static LeannConfig paper_default() { return LeannConfig(); }
  static LeannConfig fast() { LeannConfig c; isl_leann_config_fast(&c); return c; }
  static LeannConfig accurate() { LeannConfig c; isl_leann_config_accurate(&c); return c; }
  void validate() const { check(isl_leann_config_validate(this)); }
};

// CsrGraph, src/core/leann.rs:193-302 (public fields)
struct CsrGraph {
  std::vector<uint64_t> node_offsets{0};
  std::vector<uint64_t> neighbors;
  std::vector<uint64_t> levels;
  std::optional<uint64_t> entry_point;
  uint64_t max_level = 0;
  uint64_t num_nodes = 0;
  std::vector<uint64_t> degree_counts;

  uint64_t add_node(const std::vector<uint64_t>& nb, uint64_t level) {  // leann.rs:236-253
    uint64_t id = num_nodes++;
    levels.push_back(level);
    degree_counts.push_back(nb.size());
    neighbors.insert(neighbors.end(), nb.begin(), nb.end());
    node_offsets.push_back(neighbors.size());
    if (!entry_point || level > max_level) {
      entry_point = id;
      max_level = level;
    }
    return id;
  }
  std::optional<std::pair<const uint64_t*, size_t>> get_neighbors(uint64_t id) const {  // :225-233
    if (id >= num_nodes) return std::nullopt;
    return std::make_pair(neighbors.data() + node_offsets[id],
                          (size_t)(node_offsets[id + 1] - node_offsets[id]));
  }
  uint64_t storage_bytes() const {  // leann.rs:296-301
    return 8 * (node_offsets.size() + neighbors.size() + levels.size() + degree_counts.size());
  }
};

// InMemoryEmbeddingProvider, src/core/leann.rs:104-159 (row-major matrix)
struct InMemoryEmbeddingProvider {
  std::vector<float> embeddings;
  uint64_t dim = 0;
  InMemoryEmbeddingProvider(std::vector<float> rows, uint64_t dimension)
      : embeddings(std::move(rows)), dim(dimension) {
    if (embeddings.empty() || dim == 0) throw CoreError(ISL_ERR_EMPTY_COLLECTION, "Empty vector collection");
  }
  uint64_t dimension() const { return dim; }
  uint64_t len() const { return embeddings.size() / dim; }
};

// The reachability report of a graph on the device (isl_index_reachability / isl_hnsw_reachability): the counters, and
// the per-node arrays that were asked for ([len], ISL_DEPTH_UNREACHED / ISL_DEPTH_ABSENT as the header defines them).
struct Reachability {
  isl_reach_report report{};
  std::vector<uint32_t> depth, in_degree;
};
struct CoveredSeeds {
  std::vector<uint64_t> ids;  // the table after the call
  uint64_t unreached = 0;     // rows it still does not reach (non-zero only where max_seeds ended the loop)
};

// What the refine table costs (isl_index_refine_storage; rows == 0: no table), and the answer of a batch call:
// row q of ids / dist ([nq][k]) holds count[q] valid entries, ascending distance.
struct RefineStorage {
  int32_t dtype = ISL_DTYPE_F32, placement = ISL_REFINE_DEVICE;
  uint64_t rows = 0, block_bytes = 0;
};
struct BatchAnswer {
  uint64_t k = 0;
  std::vector<uint64_t> ids;
  std::vector<float> dist;
  std::vector<uint32_t> count;
  BatchAnswer(uint64_t nq, uint64_t k_) : k(k_), ids(nq * k_ + 1), dist(nq * k_ + 1), count(nq + 1) {}
};

// LeannIndex, src/core/leann.rs:492-1067
class LeannIndex {
 public:
  explicit LeannIndex(const LeannConfig& cfg = LeannConfig()) { check(isl_index_new(&cfg, &h_)); }
  static LeannIndex with_defaults() { return LeannIndex(); }
  static LeannIndex from_csr(const CsrGraph& g, const LeannConfig& cfg,
                             std::optional<uint64_t> dimension) {
    LeannIndex idx(nullptr);
    check(isl_index_from_csr(&cfg, g.num_nodes, g.node_offsets.data(), g.neighbors.data(),
                             g.levels.size() == g.num_nodes && g.num_nodes ? g.levels.data() : nullptr,
                             g.degree_counts.size() == g.num_nodes && g.num_nodes ? g.degree_counts.data() : nullptr,
                             g.entry_point ? 1 : 0, g.entry_point.value_or(0), g.max_level,
                             dimension ? 1 : 0, dimension.value_or(0), &idx.h_));
    return idx;
  }
  static LeannIndex from_bytes(const std::vector<uint8_t>& bytes) {  // leann.rs:1064
    LeannIndex idx(nullptr);
    check(isl_index_from_bytes(bytes.data(), bytes.size(), &idx.h_));
    return idx;
  }
  // LeannIndex::build (leann.rs:560-630) on the device with build options: `vectors` is n rows of
  // d floats; opts.select_rule = ISL_SELECT_DIVERSE takes the occlusion rule (islands_amd.h).
  static isl_build_options build_options() {
    isl_build_options o;
    isl_build_options_default(&o);
    return o;
  }
  static LeannIndex build(const std::vector<float>& vectors, uint64_t n, uint64_t d, const LeannConfig& cfg,
                          const isl_build_options& opts = build_options(), const uint64_t* levels = nullptr,
                          int32_t device = 0) {
    LeannIndex idx(nullptr);
    check(isl_index_build_ex(&cfg, &opts, vectors.data(), n, d, levels, ISL_MEM_HOST, device, &idx.h_));
    return idx;
  }
  // The same from bf16 rows (isl_index_build_rows): `rows_bits` is n rows of d bf16 bit patterns; the graph is
  // the one build() makes from their exact f32 images, and the index keeps the rows as bf16.
  static LeannIndex build_bf16(const std::vector<uint16_t>& rows_bits, uint64_t n, uint64_t d, const LeannConfig& cfg,
                               const isl_build_options& opts = build_options(), const uint64_t* levels = nullptr,
                               int32_t device = 0) {
    LeannIndex idx(nullptr);
    check(isl_index_build_rows(&cfg, &opts, rows_bits.data(), ISL_DTYPE_BF16, n, d, levels, ISL_MEM_HOST, device,
                               &idx.h_));
    return idx;
  }
  // More rows into the index, in place (isl_index_insert): `vectors` is n rows of d floats, which become nodes
  // len .. len + n - 1 under the index's config; returns the first new id.  opts: the rule and batch of this
  // call; levels: one per row, or NULL.  With batch 1 the index afterwards is the one build() makes of all rows.
  // On an error the index is unchanged.  Not beside searches on the same index.
  uint64_t insert(const std::vector<float>& vectors, uint64_t n, uint64_t d,
                  const isl_build_options& opts = build_options(), const uint64_t* levels = nullptr) {
    uint64_t first = 0;
    check(isl_index_insert(h_, &opts, n ? vectors.data() : nullptr, ISL_DTYPE_F32, n, d, levels, ISL_MEM_HOST, &first));
    return first;
  }
  // ... of an index that stores bf16 rows: n rows of d bf16 bit patterns
  uint64_t insert_bf16(const std::vector<uint16_t>& rows_bits, uint64_t n, uint64_t d,
                       const isl_build_options& opts = build_options(), const uint64_t* levels = nullptr) {
    uint64_t first = 0;
    check(isl_index_insert(h_, &opts, n ? rows_bits.data() : nullptr, ISL_DTYPE_BF16, n, d, levels, ISL_MEM_HOST,
                           &first));
    return first;
  }
  // Rows out of the index, in place (isl_index_remove): the lists that named a removed id are repaired under
  // opts' rule, the survivors keep their order and take new ids; returns remap[old] = new id or ISL_REMOVED.
  // Entry seeds are reduced to the survivors, PQ codes are detached.  On an error the index is unchanged.  Not
  // beside searches on the same index.
  std::vector<uint64_t> remove(const std::vector<uint64_t>& ids, const isl_build_options& opts = build_options()) {
    std::vector<uint64_t> remap(len());
    check(isl_index_remove(h_, &opts, ids.empty() ? nullptr : ids.data(), ids.size(), remap.data(), nullptr));
    return remap;
  }
  // select() of the diverse rule for one base node over candidates in any order (isl_select_neighbors)
  std::vector<uint64_t> select_neighbors(uint64_t base, const std::vector<uint64_t>& candidates, uint64_t cap,
                                         const isl_build_options& opts = build_options()) const {
    std::vector<uint64_t> out(cap ? cap : 1);
    uint32_t cnt = (uint32_t)candidates.size(), n = 0;
    check(isl_select_neighbors(h_, &opts, &base, 1, candidates.data(), candidates.size(), &cnt, cap, out.data(), &n));
    out.resize(n);
    return out;
  }
  std::vector<uint8_t> to_bytes() const {  // leann.rs:1059
    uint8_t* p = nullptr;
    size_t n = 0;
    check(isl_index_to_bytes(h_, &p, &n));
    std::vector<uint8_t> out(p, p + n);
    isl_free_bytes(p);
    return out;
  }
  LeannIndex(LeannIndex&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  LeannIndex& operator=(LeannIndex&& o) noexcept {
    if (this != &o) { isl_index_free(h_); h_ = o.h_; o.h_ = nullptr; }
    return *this;
  }
  LeannIndex(const LeannIndex&) = delete;
  LeannIndex& operator=(const LeannIndex&) = delete;
  ~LeannIndex() { isl_index_free(h_); }

  uint64_t len() const { return isl_index_len(h_); }
  bool is_empty() const { return isl_index_is_empty(h_) != 0; }
  std::optional<uint64_t> dimension() const {
    uint64_t d = 0;
    return isl_index_dimension(h_, &d) ? std::optional<uint64_t>(d) : std::nullopt;
  }
  uint64_t storage_bytes() const { return isl_index_storage_bytes(h_); }
  bool is_recompute() const { return isl_index_is_recompute(h_) != 0; }
  bool is_compact() const { return isl_index_is_compact(h_) != 0; }
  LeannConfig config() const { LeannConfig c; check(isl_index_config(h_, &c)); return c; }

  void upload(int32_t device = 0) { check(isl_index_upload(h_, device)); }
  void attach(const InMemoryEmbeddingProvider& p) {
    check(isl_set_embeddings(h_, p.embeddings.data(), p.len(), p.dim, ISL_DTYPE_F32, ISL_MEM_HOST));
  }
  // fp8 rows: n x d OCP e4m3fn codes under one power-of-two scale (host memory, or the index's device with
  // mem = ISL_MEM_DEVICE); the provider's vectors are the exact f32 images e4m3(c) * 2^scale_exp
  void set_embeddings_fp8(const uint8_t* codes, uint64_t n, uint64_t d, int32_t scale_exp = 0,
                          int32_t mem = ISL_MEM_HOST) {
    check(isl_set_embeddings_fp8(h_, codes, n, d, scale_exp, mem));
  }
  // what the in-memory rows cost: stored type (ISL_DTYPE_*), scale exponent (fp8), bytes of the row block in HBM
  struct RowStorage { int32_t dtype; int32_t scale_exp; uint64_t block_bytes; };
  RowStorage row_storage() const {
    RowStorage s{};
    check(isl_index_row_storage(h_, &s.dtype, &s.scale_exp, &s.block_bytes));
    return s;
  }
  // Room for `capacity` rows (isl_index_reserve): insert() then appends and remove() compacts in place, without a
  // second row block.  A non-empty index reserves its stored d and dtype (this is the one copy a reservation costs);
  // an empty handle fixes those of the rows to come.
  void reserve(uint64_t capacity, uint64_t d, int32_t dtype = ISL_DTYPE_F32) {
    check(isl_index_reserve(h_, capacity, d, dtype));
  }
  // rows the block is allocated for, and how often a row block has been allocated for this handle
  struct Capacity { uint64_t rows; uint64_t row_allocations; };
  Capacity capacity() const {
    Capacity c{};
    check(isl_index_capacity(h_, &c.rows, &c.row_allocations));
    return c;
  }
  // The resident rows become rows of `dtype` (ISL_DTYPE_*) on the device, each element narrowed from its exact
  // f32 image (isl_index_convert_rows); scale_exp is read for fp8 only (the default: taken from the images).
  void convert_rows(int32_t dtype, int32_t scale_exp = ISL_FP8_SCALE_AUTO) {
    check(isl_index_convert_rows(h_, dtype, scale_exp));
  }
  // Rows [first, first + count) in their stored type as bytes, dense: count x d elements of 4 (f32), 2 (bf16 bit
  // patterns) or 1 byte (e4m3 codes) -- row_storage().dtype says which (isl_index_read_rows)
  std::vector<uint8_t> read_rows(uint64_t first, uint64_t count) const {
    const int32_t dtype = row_storage().dtype;
    const uint64_t es = dtype == ISL_DTYPE_FP8_E4M3 ? 1 : dtype == ISL_DTYPE_BF16 ? 2 : 4;
    std::vector<uint8_t> out(count * dimension().value_or(0) * es);
    check(isl_index_read_rows(h_, first, count, out.data(), ISL_MEM_HOST));
    return out;
  }
  // recompute mode: EmbeddingProvider backed by the encoder (leann.rs:82-99); the embedder is
  // borrowed and must outlive the index
  void attach_recompute(isl_encoder* enc, const std::vector<uint16_t>& tokens, uint64_t n, uint64_t L,
                        bool normalize = true, bool keep_rows = false) {
    check(isl_set_recompute_provider(h_, enc, tokens.data(), nullptr, n, L, normalize ? 1 : 0,
                                     keep_rows ? 1 : 0, ISL_MEM_HOST));
  }
  // entry seeds (no reference counterpart): plain searches start at the seed nearest to the query
  std::vector<uint64_t> select_entry_seeds(uint64_t count) {
    std::vector<uint64_t> ids(count < len() ? count : len());
    uint64_t n = 0;
    check(isl_index_select_entry_seeds(h_, count, ids.data(), &n));
    ids.resize(n);
    return ids;
  }
  void set_entry_seeds(const std::vector<uint64_t>& ids) { check(isl_index_set_entry_seeds(h_, ids.data(), ids.size())); }
  std::vector<uint64_t> entry_seeds() const {
    uint64_t n = 0;
    check(isl_index_entry_seeds(h_, nullptr, 0, &n));
    std::vector<uint64_t> ids(n);
    check(isl_index_entry_seeds(h_, ids.data(), n, &n));
    return ids;
  }
  // Breadth-first report of the graph on the device from `sources` (empty: the entry-seed table if there is one,
  // else the entry point); no rows need be attached
  Reachability reachability(const std::vector<uint64_t>& sources = {}, bool depth = false, bool in_degree = false) const {
    Reachability r;
    if (depth) r.depth.resize(len());
    if (in_degree) r.in_degree.resize(len());
    check(isl_index_reachability(h_, sources.empty() ? nullptr : sources.data(), sources.size(),
                                 depth ? r.depth.data() : nullptr, in_degree ? r.in_degree.data() : nullptr, ISL_MEM_HOST,
                                 &r.report));
    return r;
  }
  // Extends the table (or [entry_point]) by the smallest unreached id until every row is reachable from SOME seed or
  // the table holds max_seeds (isl_index_cover_entry_seeds)
  CoveredSeeds cover_entry_seeds(uint64_t max_seeds = ISL_MAX_ENTRY_SEEDS) {
    CoveredSeeds c;
    c.ids.resize(max_seeds);
    uint64_t n = 0;
    check(isl_index_cover_entry_seeds(h_, max_seeds, c.ids.data(), &n, &c.unreached));
    c.ids.resize(n < max_seeds ? n : max_seeds);
    return c;
  }
  // queries: nq rows of dimension() floats, row-major
  std::vector<uint64_t> pick_entries(const std::vector<float>& queries, uint64_t nq) const {
    std::vector<uint64_t> ids(nq);
    check(isl_index_pick_entries(h_, queries.data(), nq, nq ? queries.size() / nq : 0, ids.data(), ISL_MEM_HOST, nullptr));
    return ids;
  }
  // no reference counterpart: sets up every search lane ahead of time (isl_index_prepare)
  void prepare(uint64_t max_nq, uint64_t max_ef, uint64_t max_k = 10, int32_t lanes = 8) {
    check(isl_index_prepare(h_, max_nq, max_ef, max_k, lanes));
  }
  // search / search_with_params, leann.rs:858-896
  std::vector<std::pair<uint64_t, float>> search(const std::vector<float>& query, uint64_t k) const {
    return search_with_params(query, k, config().ef_search);
  }
  std::vector<std::pair<uint64_t, float>> search_with_params(const std::vector<float>& query,
                                                             uint64_t k, uint64_t ef) const {
    std::vector<uint64_t> ids(k ? k : 1);
    std::vector<float> dist(k ? k : 1);
    uint32_t cnt = 0;
    check(isl_search_batch(h_, query.data(), 1, query.size(), k, ef, ids.data(), dist.data(), &cnt));
    std::vector<std::pair<uint64_t, float>> out;
    for (uint32_t i = 0; i < cnt; i++) out.emplace_back(ids[i], dist[i]);
    return out;
  }
  // extension: the two-level search leann.rs:855-857 asks for (docs/leann-specification.md:223-275);
  // codes = ProductQuantizer::encode of every node, [n][m]; the quantizer is borrowed
  void attach_pq_codes(const isl_pq* pq, const std::vector<uint16_t>& codes, uint64_t n) {
    check(isl_index_set_pq_codes(h_, pq, codes.data(), n, ISL_MEM_HOST));
  }
  std::vector<std::pair<uint64_t, float>> search_two_level(const std::vector<float>& query, uint64_t k,
                                                           uint64_t ef, float rerank_ratio) const {
    std::vector<uint64_t> ids(k ? k : 1);
    std::vector<float> dist(k ? k : 1);
    uint32_t cnt = 0;
    check(isl_search_two_level_batch(h_, query.data(), 1, query.size(), k, ef, rerank_ratio, ids.data(),
                                     dist.data(), &cnt));
    std::vector<std::pair<uint64_t, float>> out;
    for (uint32_t i = 0; i < cnt; i++) out.emplace_back(ids[i], dist[i]);
    return out;
  }
  // extension: refined search.  The table a refined search re-scores its candidates against: n = len() rows of d
  // floats (or bf16 bit patterns), kept on the device or in pinned host memory (ISL_REFINE_*); no rows drops it
  void set_refine_rows(const std::vector<float>& rows, uint64_t n, int32_t placement = ISL_REFINE_DEVICE) {
    check(isl_index_set_refine_rows(h_, rows.data(), n, n ? rows.size() / n : 0, ISL_DTYPE_F32, ISL_MEM_HOST, placement));
  }
  void set_refine_rows_bf16(const std::vector<uint16_t>& bits, uint64_t n, int32_t placement = ISL_REFINE_DEVICE) {
    check(isl_index_set_refine_rows(h_, bits.data(), n, n ? bits.size() / n : 0, ISL_DTYPE_BF16, ISL_MEM_HOST, placement));
  }
  RefineStorage refine_storage() const {
    RefineStorage s;
    check(isl_index_refine_storage(h_, &s.dtype, &s.placement, &s.rows, &s.block_bytes));
    return s;
  }
  // search_batch(queries, candidates, ef) over the stored rows, then the best k of those by their distances to the
  // refine rows (isl_search_refined_batch); queries: nq rows of dimension() floats
  BatchAnswer search_refined_batch(const std::vector<float>& queries, uint64_t nq, uint64_t k, uint64_t ef,
                                   uint64_t candidates = 0) const {
    if (!candidates) candidates = ef < ISL_REFINE_MAX_CANDIDATES ? ef : ISL_REFINE_MAX_CANDIDATES;
    BatchAnswer a(nq, k);
    check(isl_search_refined_batch(h_, queries.data(), nq, nq ? queries.size() / nq : 0, k, candidates, ef, a.ids.data(),
                                   a.dist.data(), a.count.data()));
    return a;
  }
  // the rescoring alone (isl_rescore): cand_ids [nq][pitch], the first cand_count[q] of row q valid
  BatchAnswer rescore(const std::vector<float>& queries, uint64_t nq, const std::vector<uint64_t>& cand_ids,
                      const std::vector<uint32_t>& cand_count, uint64_t k) const {
    BatchAnswer a(nq, k);
    check(isl_rescore(h_, queries.data(), nq, nq ? queries.size() / nq : 0, cand_ids.data(), cand_count.data(),
                      nq ? cand_ids.size() / nq : 0, k, a.ids.data(), a.dist.data(), a.count.data()));
    return a;
  }
  isl_index* handle() const { return h_; }

 private:
  explicit LeannIndex(std::nullptr_t) {}
  isl_index* h_ = nullptr;
};

// ---- hnsw.rs / search.rs facade ------------------------------------------------------------
// SearchResult, src/core/search.rs:54-103
struct SearchResult {
  uint64_t id = 0;
  float score = 0.f;
  std::optional<std::vector<float>> vector;
  std::optional<std::string> text;
  float to_similarity() const { return 1.0f / (1.0f + score); }  // search.rs:100-102
};

// SearchConfig, src/core/search.rs:8-52
struct SearchConfig {
  uint64_t top_k = 10, ef = 100;
  bool include_vectors = false, include_metadata = true;
  std::optional<float> min_similarity;
  static SearchConfig fast(uint64_t k) { SearchConfig c; c.top_k = k; c.ef = k * 2; return c; }
  static SearchConfig accurate(uint64_t k) { SearchConfig c; c.top_k = k; c.ef = k * 10; return c; }
};

// HnswGraph, src/core/hnsw.rs:149-515, on the device.  build() constructs one from its vectors
// (HnswGraph::insert, hnsw.rs:214-329, as isl_hnsw_build); the constructor takes a graph made elsewhere
// layer by layer (layers[L][node] = neighbour ids); from_bytes / to_bytes carry the bincode image.
class HnswGraph {
 public:
  HnswGraph(const std::vector<float>& vectors, uint64_t dim,
            const std::vector<std::vector<std::vector<uint64_t>>>& layers,
            const std::vector<uint64_t>& levels, std::optional<uint64_t> entry_point, uint64_t max_level,
            uint64_t m = 16, uint64_t m0 = 32, uint64_t ef_construction = 200,
            DistanceMetric metric = DistanceMetric::Cosine, int32_t device = 0)
      : vectors_(vectors), dim_(dim) {
    const uint64_t n = levels.size();
    std::vector<std::vector<uint64_t>> offs(layers.size()), adjs(layers.size());
    std::vector<const uint64_t*> po, pa;
    for (size_t L = 0; L < layers.size(); L++) {
      offs[L].assign(1, 0);
      for (uint64_t i = 0; i < n; i++) {
        adjs[L].insert(adjs[L].end(), layers[L][i].begin(), layers[L][i].end());
        offs[L].push_back(adjs[L].size());
      }
      if (adjs[L].empty()) adjs[L].push_back(0);
      po.push_back(offs[L].data());
      pa.push_back(adjs[L].data());
    }
    check(isl_hnsw_from_layers(m, m0, ef_construction, (int32_t)metric, n, dim, layers.size(), po.data(),
                               pa.data(), n ? levels.data() : nullptr, entry_point ? 1 : 0,
                               entry_point.value_or(0), max_level, n ? vectors.data() : nullptr, device, &h_));
  }
  // HnswGraph::from_bytes, hnsw.rs:511-514 (bincode image; entries in any HashMap order)
  static HnswGraph from_bytes(const std::vector<uint8_t>& bytes, int32_t device = 0) {
    HnswGraph g;
    check(isl_hnsw_from_bytes(bytes.data(), bytes.size(), device, &g.h_));
    return g;
  }
  // HnswGraph::insert for rows 0 .. n-1 on the device (isl_hnsw_build): `levels` empty = drawn from
  // level_seed; opts NULL = the reference rule, one node per step
  static HnswGraph build(const std::vector<float>& vectors, uint64_t dim, const isl_hnsw_config* cfg = nullptr,
                         const std::vector<uint64_t>& levels = {}, uint64_t level_seed = 0,
                         const isl_build_options* opts = nullptr, int32_t device = 0) {
    HnswGraph g;
    const uint64_t n = dim ? vectors.size() / dim : 0;
    check(isl_hnsw_build(cfg, opts, n ? vectors.data() : nullptr, n, dim, levels.empty() ? nullptr : levels.data(),
                         level_seed, ISL_MEM_HOST, device, &g.h_));
    return g;
  }
  // build() from bf16 rows (isl_hnsw_build_rows): rows_bits = n x dim bf16 bit patterns.  The graph is the one
  // build() makes of their exact float32 images; the rows stay bf16 on the device (row_storage()).
  static HnswGraph build_bf16(const std::vector<uint16_t>& rows_bits, uint64_t dim, const isl_hnsw_config* cfg = nullptr,
                              const std::vector<uint64_t>& levels = {}, uint64_t level_seed = 0,
                              const isl_build_options* opts = nullptr, int32_t device = 0) {
    HnswGraph g;
    const uint64_t n = dim ? rows_bits.size() / dim : 0;
    check(isl_hnsw_build_rows(cfg, opts, n ? rows_bits.data() : nullptr, ISL_DTYPE_BF16, n, dim,
                              levels.empty() ? nullptr : levels.data(), level_seed, ISL_MEM_HOST, device, &g.h_));
    return g;
  }
  // insert() for a graph that stores bf16 rows (isl_hnsw_insert_rows); an empty graph becomes a bf16 graph.  Rows
  // of the other type than the graph stores are refused (Unsupported) and leave the graph unchanged.
  uint64_t insert_bf16(const std::vector<uint16_t>& rows_bits, uint64_t dim, const std::vector<uint64_t>& levels = {},
                       uint64_t level_seed = 0, const isl_build_options* opts = nullptr) {
    const uint64_t n = dim ? rows_bits.size() / dim : 0;
    uint64_t first = 0;
    check(isl_hnsw_insert_rows(h_, opts, n ? rows_bits.data() : nullptr, ISL_DTYPE_BF16, n, dim,
                               levels.empty() ? nullptr : levels.data(), level_seed, ISL_MEM_HOST, &first));
    if (n) vectors_.clear();
    return first;
  }
  // What the rows cost on the device (isl_hnsw_row_storage): the stored type (ISL_DTYPE_F32 / ISL_DTYPE_BF16) and
  // the bytes of the row table; an empty graph: ISL_DTYPE_F32 and 0.
  struct RowStorage {
    int32_t dtype;
    uint64_t block_bytes;
  };
  RowStorage row_storage() const {
    RowStorage s{ISL_DTYPE_F32, 0};
    check(isl_hnsw_row_storage(h_, &s.dtype, &s.block_bytes));
    return s;
  }
  // HnswGraph::insert (hnsw.rs:214-251) for more rows, in place (isl_hnsw_insert): nodes len .. len + n - 1 under
  // the config the graph carries; returns the first new id.  `levels` empty = the level_seed stream continued at
  // position len; opts NULL = the reference rule, one node per step.  On an error the graph is unchanged.
  uint64_t insert(const std::vector<float>& vectors, uint64_t dim, const std::vector<uint64_t>& levels = {},
                  uint64_t level_seed = 0, const isl_build_options* opts = nullptr) {
    const uint64_t n = dim ? vectors.size() / dim : 0;
    uint64_t first = 0;
    check(isl_hnsw_insert(h_, opts, n ? vectors.data() : nullptr, n, dim, levels.empty() ? nullptr : levels.data(),
                          level_seed, ISL_MEM_HOST, &first));
    if (n) vectors_.clear();  // the host copy of the smaller graph's rows: get_vector asks the device now
    return first;
  }
  // Rows out of the graph, in place (isl_hnsw_remove): on every layer the lists that named a removed id are
  // repaired under opts' rule, the survivors keep their order and levels and take new ids; returns
  // remap[old] = new id or ISL_REMOVED.  On an error the graph is unchanged.  Not beside searches on the same
  // graph.
  std::vector<uint64_t> remove(const std::vector<uint64_t>& ids,
                               const isl_build_options& opts = LeannIndex::build_options()) {
    std::vector<uint64_t> remap(len());
    check(isl_hnsw_remove(h_, &opts, ids.empty() ? nullptr : ids.data(), ids.size(), remap.data(), nullptr));
    if (!ids.empty()) vectors_.clear();  // the host copy of the larger graph's rows: get_vector asks the device now
    return remap;
  }
  // Breadth-first report of one layer from `sources` (empty: the entry point); depth holds ISL_DEPTH_ABSENT for the
  // nodes below the layer (isl_hnsw_reachability)
  Reachability reachability(uint64_t layer = 0, const std::vector<uint64_t>& sources = {}, bool depth = false,
                            bool in_degree = false) const {
    Reachability r;
    if (depth) r.depth.resize(len());
    if (in_degree) r.in_degree.resize(len());
    check(isl_hnsw_reachability(h_, layer, sources.empty() ? nullptr : sources.data(), sources.size(),
                                depth ? r.depth.data() : nullptr, in_degree ? r.in_degree.data() : nullptr, ISL_MEM_HOST,
                                &r.report));
    return r;
  }
  // HnswGraph::to_bytes, hnsw.rs:507-509 (nodes in ascending id)
  std::vector<uint8_t> to_bytes() const {
    uint8_t* p = nullptr;
    size_t n = 0;
    check(isl_hnsw_to_bytes(h_, &p, &n));
    std::vector<uint8_t> out(p, p + n);
    isl_free_bytes(p);
    return out;
  }
  std::vector<uint64_t> neighbors(uint64_t node, uint64_t layer) const {  // neighbors_at(layer); empty above the level
    uint64_t cnt = 0;
    check(isl_hnsw_get_neighbors(h_, node, layer, nullptr, 0, &cnt, nullptr));
    std::vector<uint64_t> out(cnt);
    if (cnt) check(isl_hnsw_get_neighbors(h_, node, layer, out.data(), cnt, &cnt, nullptr));
    return out;
  }
  HnswGraph(HnswGraph&& o) noexcept : h_(o.h_), vectors_(std::move(o.vectors_)), dim_(o.dim_) { o.h_ = nullptr; }
  HnswGraph(const HnswGraph&) = delete;
  HnswGraph& operator=(const HnswGraph&) = delete;
  ~HnswGraph() { isl_hnsw_free(h_); }
  uint64_t len() const { return isl_hnsw_len(h_); }
  bool is_empty() const { return len() == 0; }
  // HnswGraph::search, hnsw.rs:458-504
  std::vector<std::pair<uint64_t, float>> search(const std::vector<float>& query, uint64_t k, uint64_t ef) const {
    return search_batch(query, 1, k, ef)[0];
  }
  std::vector<std::vector<std::pair<uint64_t, float>>> search_batch(const std::vector<float>& queries,
                                                                    uint64_t nq, uint64_t k, uint64_t ef) const {
    std::vector<uint64_t> ids(nq * (k ? k : 1));
    std::vector<float> dist(nq * (k ? k : 1));
    std::vector<uint32_t> cnt(nq);
    check(isl_hnsw_search_batch(h_, queries.data(), nq, nq ? queries.size() / nq : 0, k, ef, ids.data(),
                                dist.data(), cnt.data()));
    std::vector<std::vector<std::pair<uint64_t, float>>> out(nq);
    for (uint64_t q = 0; q < nq; q++)
      for (uint32_t i = 0; i < cnt[q]; i++) out[q].emplace_back(ids[q * k + i], dist[q * k + i]);
    return out;
  }
  std::optional<std::vector<float>> get_vector(uint64_t id) const {  // get_node(id).vector, hnsw.rs:507-510
    if (id >= len()) return std::nullopt;
    if (!vectors_.empty()) return std::vector<float>(vectors_.begin() + id * dim_, vectors_.begin() + (id + 1) * dim_);
    uint64_t dim = 0;  // built on the device or read by from_bytes: no host copy, the row comes back from the device
    check(isl_hnsw_info(h_, nullptr, nullptr, nullptr, &dim));
    std::vector<float> out(dim);
    check(isl_hnsw_get_vector(h_, id, out.data()));
    return out;
  }

 private:
  HnswGraph() = default;
  isl_hnsw* h_ = nullptr;
  std::vector<float> vectors_;
  uint64_t dim_ = 0;
};

// Searcher, src/core/search.rs:105-182; search_batch is one device launch instead of the
// reference's sequential map (:179-181).
class Searcher {
 public:
  explicit Searcher(const HnswGraph& g, SearchConfig c = SearchConfig()) : graph_(g), config_(c) {}
  Searcher& top_k(uint64_t k) { config_.top_k = k; return *this; }
  Searcher& ef(uint64_t e) { config_.ef = e; return *this; }
  Searcher& include_vectors() { config_.include_vectors = true; return *this; }
  Searcher& min_similarity(float t) { config_.min_similarity = t; return *this; }
  std::vector<SearchResult> search(const std::vector<float>& query) const { return search_batch(query, 1)[0]; }
  std::vector<std::vector<SearchResult>> search_batch(const std::vector<float>& queries, uint64_t nq) const {
    auto raw = graph_.search_batch(queries, nq, config_.top_k, config_.ef);
    std::vector<std::vector<SearchResult>> out(nq);
    for (uint64_t q = 0; q < nq; q++)
      for (auto& [id, d] : raw[q]) {
        SearchResult r;
        r.id = id;
        r.score = d;
        if (config_.include_vectors) r.vector = graph_.get_vector(id);
        if (!config_.min_similarity || r.to_similarity() >= *config_.min_similarity) out[q].push_back(std::move(r));
      }
    return out;
  }

 private:
  const HnswGraph& graph_;
  SearchConfig config_;
};

// ---- MultiIndexSearcher over id-range shards, one rank per GPU (search.rs:211-237) ------------
// ShardGroup = the ranks' communicator: RCCL from a unique id rank 0 made (unique_id(), carried to the
// other ranks by the host's own means), or a blocking host all-gather callback.
class ShardGroup {
 public:
  static std::vector<uint8_t> unique_id() {
    std::vector<uint8_t> id(ISL_SHARD_UNIQUE_ID_BYTES);
    check(isl_shard_unique_id(id.data()));
    return id;
  }
  ShardGroup(int32_t device, int32_t world, int32_t rank, const std::vector<uint8_t>& id) {
    check(isl_shard_group_create(device, world, rank, id.data(), &h_));
  }
  ShardGroup(int32_t device, int32_t world, int32_t rank, isl_shard_allgather_fn fn, void* user) {
    check(isl_shard_group_create_host(device, world, rank, fn, user, &h_));
  }
  ShardGroup(const ShardGroup&) = delete;
  ShardGroup& operator=(const ShardGroup&) = delete;
  ~ShardGroup() { isl_shard_group_free(h_); }
  int32_t comm_ranks() const { int32_t n = 0; check(isl_shard_group_info(h_, nullptr, nullptr, &n, nullptr)); return n; }
  isl_shard_group* handle() const { return h_; }

 private:
  isl_shard_group* h_ = nullptr;
};

struct ShardedResult { uint64_t id; float score; uint32_t shard; };

class ShardedSearcher {
 public:
  // `shard`: this rank's index over its id range (local ids); group = nullptr: a single shard
  ShardedSearcher(const LeannIndex& shard, ShardGroup* group, uint64_t n_total, int32_t depth = 8) {
    check(isl_sharded_searcher_new(shard.handle(), group ? group->handle() : nullptr, n_total, nullptr, depth, &h_));
  }
  ShardedSearcher(const ShardedSearcher&) = delete;
  ShardedSearcher& operator=(const ShardedSearcher&) = delete;
  ~ShardedSearcher() { isl_sharded_searcher_free(h_); }
  void prepare(uint64_t nq, uint64_t k, uint64_t ef) { check(isl_sharded_prepare(h_, nq, k, ef)); }
  // the same batch on every rank; every rank gets the merged answer (global ids, ascending, ties -> lower shard)
  std::vector<std::vector<ShardedResult>> search_batch(const std::vector<float>& queries, uint64_t nq, uint64_t k,
                                                       uint64_t ef) {
    std::vector<uint64_t> ids(nq * k);
    std::vector<float> dist(nq * k);
    std::vector<uint32_t> src(nq * k), cnt(nq);
    check(isl_sharded_search_batch(h_, queries.data(), nq, nq ? queries.size() / nq : 0, k, ef, ids.data(), dist.data(),
                                   src.data(), cnt.data()));
    std::vector<std::vector<ShardedResult>> out(nq);
    for (uint64_t q = 0; q < nq; q++)
      for (uint32_t j = 0; j < cnt[q]; j++) out[q].push_back({ids[q * k + j], dist[q * k + j], src[q * k + j]});
    return out;
  }
  isl_sharded_searcher* handle() const { return h_; }

 private:
  isl_sharded_searcher* h_ = nullptr;
};

// ---- embedding/candle_provider.rs ---------------------------------------------------------
// CandleEmbedder after tokenisation (candle_provider.rs:226-507): weights by checkpoint tensor
// name, embed = embed_texts_raw on padded token ids.
class CandleEmbedder {
 public:
  CandleEmbedder(const isl_bert_config& cfg, bool normalize = true, int32_t device = 0)
      : cfg_(cfg), normalize_(normalize) { check(isl_encoder_new(&cfg, device, &h_)); }
  CandleEmbedder(const CandleEmbedder&) = delete;
  CandleEmbedder& operator=(const CandleEmbedder&) = delete;
  ~CandleEmbedder() { isl_encoder_free(h_); }
  void set_weight(const std::string& name, const std::vector<float>& v) {
    check(isl_encoder_set_weight(h_, name.c_str(), v.data(), v.size(), ISL_MEM_HOST));
  }
  uint64_t dimension() const { return cfg_.hidden; }
  // ids / mask: B rows of L entries (padding: id 0, mask 0, candle_provider.rs:385-402)
  std::vector<float> embed(const std::vector<int64_t>& ids, const std::vector<float>& mask, uint64_t B,
                           uint64_t L) const {
    std::vector<float> out(B * cfg_.hidden);
    check(isl_encoder_embed(h_, ids.data(), nullptr, mask.empty() ? nullptr : mask.data(), B, L,
                            normalize_ ? 1 : 0, out.data(), ISL_MEM_HOST, nullptr));
    return out;
  }
  isl_encoder* handle() const { return h_; }

 private:
  isl_encoder* h_ = nullptr;
  isl_bert_config cfg_;
  bool normalize_;
};

}  // namespace islands::core
