/*
 * islands_amd.h -- C ABI of the MI355X-native LEANN search path.
 *
 * This is the drop-in boundary for the `islands::core` search hot path of
 * panbanda/islands v1.5.0.  The reference has no FFI of its own (it is a
 * single Rust crate); each entry point below replaces one inherent method /
 * trait method of `src/core`, cited as file:line, and is what a Rust
 * `unsafe extern "C"` block would bind (see INTEGRATION.md for that stub).
 *
 * Conventions
 *   - every function returns isl_status (0 = Ok, otherwise the CoreError
 *     variant of src/core/error.rs:9-62, same order); nothing aborts or throws
 *     across the ABI.  Details of the last error on the calling thread are read
 *     with the isl_last_error_* getters.
 *   - inputs are borrowed for the duration of the call; outputs are written
 *     into caller-allocated buffers, except *_to_bytes (freed with
 *     isl_free_bytes).  An index handle owns its host and device copies.
 *   - plain pointers and sizes only; no C++/torch types.  `stream` arguments
 *     are a hipStream_t passed as void* (NULL = the library's own stream).
 *   - the compute path is HIP on gfx950.  There is NO CPU fallback: without a
 *     usable device every compute entry point returns ISL_ERR_DEVICE.
 */
#ifndef ISLANDS_AMD_H
#define ISLANDS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISL_ABI_VERSION 3

typedef int32_t isl_status;

/* CoreError, src/core/error.rs:9-62 (declaration order), plus ABI-level codes >= 100. */
enum {
  ISL_OK = 0,
  ISL_ERR_DIMENSION_MISMATCH = 1, /* payload: expected, actual */
  ISL_ERR_EMPTY_COLLECTION = 2,
  ISL_ERR_INVALID_CONFIG = 3,
  ISL_ERR_INDEX_NOT_BUILT = 4,
  ISL_ERR_NODE_NOT_FOUND = 5, /* payload: node id */
  ISL_ERR_SERIALIZATION = 6,
  ISL_ERR_DESERIALIZATION = 7,
  ISL_ERR_IO = 8,
  ISL_ERR_HNSW = 9,
  ISL_ERR_PQ = 10,
  ISL_ERR_SEARCH = 11,
  ISL_ERR_EMBEDDING = 12,
  ISL_ERR_DEVICE = 100,           /* no gfx950 device / HIP runtime error */
  ISL_ERR_INVALID_ARGUMENT = 101, /* NULL pointer, bad enum value */
  ISL_ERR_UNSUPPORTED = 102
};

/* DistanceMetric, src/core/distance.rs:9-19 (bincode variant index). */
enum { ISL_METRIC_COSINE = 0, ISL_METRIC_EUCLIDEAN = 1, ISL_METRIC_DOT = 2, ISL_METRIC_MANHATTAN = 3 };
/* PruningStrategy, src/core/leann.rs:168-178. */
enum { ISL_PRUNE_GLOBAL = 0, ISL_PRUNE_LOCAL = 1, ISL_PRUNE_PROPORTIONAL = 2 };
/* Row element types accepted by isl_set_embeddings.  ISL_DTYPE_FP8_E4M3: one byte per element, OCP e4m3fn
 * (isl_set_embeddings_fp8); the builders, isl_index_insert and the encoder take F32 and BF16 only. */
enum { ISL_DTYPE_F32 = 0, ISL_DTYPE_BF16 = 1, ISL_DTYPE_FP8_E4M3 = 2 };
/* Where a caller's buffer lives. */
enum { ISL_MEM_HOST = 0, ISL_MEM_DEVICE = 1 };

/* ---- error details (thread-local) ---- */
const char* isl_last_error_message(void);
uint64_t isl_last_error_expected(void); /* DimensionMismatch.expected */
uint64_t isl_last_error_actual(void);   /* DimensionMismatch.actual   */
uint64_t isl_last_error_node(void);     /* NodeNotFound(id)           */
const char* isl_status_name(isl_status s);
uint32_t isl_abi_version(void);
/* Number of usable gfx950 devices (0 when none; never an error). */
int32_t isl_device_count(void);

/* ---- LeannConfig, src/core/leann.rs:322-371 (same fields, same order) ---- */
typedef struct isl_leann_config {
  uint64_t m;
  uint64_t m0;
  uint64_t ef_construction;
  double ml;
  uint64_t max_layers;
  uint32_t metric; /* ISL_METRIC_* */
  uint64_t ef_search;
  uint64_t beam_width;
  float prune_ratio;
  uint32_t pruning_strategy; /* ISL_PRUNE_* */
  uint8_t high_degree_pruning;
  float hub_percentile;
  uint8_t is_compact;
  uint8_t is_recompute;
} isl_leann_config;

void isl_leann_config_paper_default(isl_leann_config* c); /* leann.rs:386-403 */
void isl_leann_config_fast(isl_leann_config* c);          /* leann.rs:406-416 */
void isl_leann_config_accurate(isl_leann_config* c);      /* leann.rs:419-429 */
isl_status isl_leann_config_validate(const isl_leann_config* c); /* leann.rs:432-460 */

/* ---- LeannIndex, src/core/leann.rs:492-546 ---- */
typedef struct isl_index isl_index;

/* LeannIndex::new, leann.rs:504-511 (validates the config). */
isl_status isl_index_new(const isl_leann_config* cfg, isl_index** out);
/* Build an index handle from CsrGraph's public fields (leann.rs:193-208).
 * levels/degree_counts may be NULL (zeros / row lengths).  dimension:
 * has_dimension = 0 encodes None. */
isl_status isl_index_from_csr(const isl_leann_config* cfg, uint64_t num_nodes,
                              const uint64_t* node_offsets, const uint64_t* neighbors,
                              const uint64_t* levels, const uint64_t* degree_counts,
                              int32_t has_entry, uint64_t entry_point, uint64_t max_level,
                              int32_t has_dimension, uint64_t dimension, isl_index** out);
/* Same, from arrays already resident on `device` (u64 offsets, u32 neighbour
 * ids); the handle takes a private device copy, the host CSR is materialised
 * lazily (to_bytes / get_neighbors). */
isl_status isl_index_from_device_csr(const isl_leann_config* cfg, int32_t device,
                                     uint64_t num_nodes, const uint64_t* d_node_offsets,
                                     const uint32_t* d_neighbors, int32_t has_entry,
                                     uint64_t entry_point, int32_t has_dimension,
                                     uint64_t dimension, isl_index** out);
/* LeannIndex::build, leann.rs:560-630, on the device: insertion in id order, construction
 * search with ef_construction (:692-749), high-degree-preserving selection (:761-833) or
 * truncation (:685), bidirectional links with a distance re-sort past m0 (:592-607, :634-658).
 * `levels` replaces random_level (thread_rng, :549-554; NULL = all 0).  `batch` = nodes inserted
 * per step: 1 reproduces the reference's sequential construction (CsrGraph identical field by
 * field), larger values trade that for throughput.  The vectors become the index's in-memory
 * provider.  Limits: m0 <= 128 (LeannConfig::accurate() has 96), ef_construction <= 512. */
isl_status isl_index_build(const isl_leann_config* cfg, const float* vectors, uint64_t n, uint64_t d,
                           const uint64_t* levels, uint64_t batch, int32_t mem, int32_t device,
                           isl_index** out);

/* ---- extension: a second neighbour-selection rule for the builder ----
 * ISL_SELECT_REFERENCE is the rule above.  ISL_SELECT_DIVERSE is the occlusion rule (HNSW "select
 * neighbours by heuristic", Vamana robust prune).  select(b, C, M): walk the candidates C in
 * ascending d(b, c), ties in their given order; c is occluded iff some s kept before it has
 * alpha * d(s, c) <= d(b, c) (f32 multiply, then compare; a NaN occludes nothing; d(s, c) =
 * Distance::calculate(vec[s], vec[c]) in the index's metric); an occluded c goes to `dropped`, any
 * other to `kept`; stop at M kept.  With keep_pruned, `dropped` then fills the row up to M in its
 * order.  The row is `kept` followed by the fillers.  The build is otherwise the one above: the new
 * node i gets select(i, search result, m0) with the search's distances; every selected s that does
 * not hold i yet gets it appended, and a row that reaches m0 + 1 ids is replaced by select(s, the
 * row stable-sorted by d(s, .), m0).  high_degree_pruning / hub_percentile are ignored under this
 * rule.  The rule is not recorded in the index: isl_leann_config and its bytes stay the
 * reference's, and the result is an ordinary flat CsrGraph. */
enum { ISL_SELECT_REFERENCE = 0, ISL_SELECT_DIVERSE = 1 };
typedef struct isl_build_options {
  uint32_t struct_size; /* sizeof(isl_build_options), for later growth */
  uint32_t select_rule; /* ISL_SELECT_* */
  float alpha;          /* finite and >= 1, DIVERSE only */
  uint32_t keep_pruned; /* 0 / 1, DIVERSE only */
  uint64_t batch;       /* as isl_index_build's */
} isl_build_options;
void isl_build_options_default(isl_build_options* o); /* REFERENCE, 1.0, 1, batch 1 */
/* isl_index_build with options (NULL = the defaults; isl_index_build is this call with the
 * default options and its `batch`).  Checked before any device call: struct_size too small or an
 * unknown rule -> ISL_ERR_INVALID_ARGUMENT; DIVERSE with alpha not finite or < 1 ->
 * ISL_ERR_INVALID_CONFIG. */
isl_status isl_index_build_ex(const isl_leann_config* cfg, const isl_build_options* opts,
                              const float* vectors, uint64_t n, uint64_t d, const uint64_t* levels,
                              int32_t mem, int32_t device, isl_index** out);
/* isl_index_build_ex over rows of either stored type.  dtype ISL_DTYPE_F32: rows = n x d float, the call IS
 * isl_index_build_ex.  dtype ISL_DTYPE_BF16: rows = n x d bf16 bit patterns (u16); the provider's vectors are
 * their exact f32 images, the construction is LeannIndex::build over those images (either selection rule,
 * any batch), and the finished index keeps the rows as bf16 -- as if isl_set_embeddings(..., ISL_DTYPE_BF16)
 * had been called on it.  Host or device rows (mem).  Checked in this order before any device call: NULL
 * out, or NULL rows with n > 0 -> ISL_ERR_INVALID_ARGUMENT; opts as in isl_index_build_ex; an unknown dtype ->
 * ISL_ERR_INVALID_ARGUMENT; isl_leann_config_validate; n == 0 -> an empty index; d == 0 ->
 * ISL_ERR_EMPTY_COLLECTION; m0 > 128, ef_construction > 512 or too many nodes -> ISL_ERR_UNSUPPORTED. */
isl_status isl_index_build_rows(const isl_leann_config* cfg, const isl_build_options* opts, const void* rows,
                                int32_t dtype, uint64_t n, uint64_t d, const uint64_t* levels, int32_t mem,
                                int32_t device, isl_index** out);
/* More rows into a built index, in place: nodes len .. len + n_new - 1 enter `idx` in id order under the config
 * the handle carries.  rows = n_new x d elements of `dtype`, host or device (mem); opts = the rule and batch of
 * this call as for isl_index_build_rows (NULL: the defaults); levels[i] stands for random_level() of node
 * len + i (NULL: 0), taken as isl_index_build_rows takes them; *first_id (may be NULL) receives the old len,
 * written only on ISL_OK.
 * Definition: the graph afterwards is the state of LeannIndex::build's loop (leann.rs:578-615) continued at
 * iteration id = len from adjacency = the index's lists in their stored order and entry_point / max_level =
 * the index's.  With opts->batch == 1, on an index built here with batch 1, the result is therefore the
 * isl_index_to_bytes image of isl_index_build_rows over all len + n_new rows with the concatenated levels, under
 * either rule.  batch > 1 is the builder's throughput mode entered at node len: same rules, no parity claim.
 * Rows: the index must hold resident in-memory rows (isl_set_embeddings or a build), and dtype must be their
 * stored type -- nothing is converted.  bf16: the construction runs over the widened rows and the grown index
 * keeps bf16 rows.  An index from isl_index_from_csr / _load / _from_bytes + isl_index_upload + isl_set_embeddings
 * grows like a built one.  An empty handle takes the rows as isl_index_build_rows would with the handle's config,
 * on the device it was uploaded to, else on device 0 (ISL_ENTRY_SEEDS is read by builds only).
 * Strong guarantee: the grown graph is built beside the old one and moved into the handle at the end; on any
 * failure idx is unchanged (bytes, rows, search answers) and the old rows are never modified.  Peak device
 * memory: the old index whole, plus what isl_index_build_rows over len + n_new rows holds at its peak (the rows
 * of all nodes, the (m0 + 1)-wide construction table, the CSR twice at compaction, the padded adjacency).
 * Reserved index (isl_index_reserve) with len + n_new <= its capacity: the new rows are written in place behind
 * the old ones and their norms computed there; no row block is allocated and no old row is copied or written, so
 * the peak above loses "the rows of all nodes".  The steps, the kernels, the lists built beside the old graph, the
 * refusals and what the handle keeps are the same, and so is the guarantee: rows behind len are invisible until the
 * grown graph is moved in, and on failure they are zeroed again.  Searches on other lanes read rows below len only.
 * len + n_new > capacity: the reservation is used up -- a new table of exactly len + n_new rows as for an index
 * nobody reserved, and afterwards capacity == len.  Nothing grows a reservation on its own.
 * What the handle keeps: its config, the visited-table hint, its prepared lanes (none of their buffers follows
 * the node count) and its entry seeds AS THEY ARE -- ids and row copies of nodes the graph still has, so a
 * plain search is still the reference search entered at the nearest seed; they are not re-selected.  What goes:
 * the heap-exact kernel's pool (made again on demand) and the PQ codes, which no longer cover every node -- a
 * two-level search afterwards answers as for an index that never had codes until isl_index_set_pq_codes is
 * called again.
 * The call is the reference's &mut self: not beside searches on the same handle (a busy lane ->
 * ISL_ERR_SEARCH).  Checked in this order before any device call: NULL idx, or NULL rows with n_new > 0 ->
 * ISL_ERR_INVALID_ARGUMENT; opts as in isl_index_build_ex; an unknown dtype -> ISL_ERR_INVALID_ARGUMENT;
 * n_new == 0 -> ISL_OK, nothing changed; the core index of an HnswGraph (use isl_hnsw_insert) or an index on the
 * recompute provider -> ISL_ERR_UNSUPPORTED; a non-empty index and d != its dimension ->
 * ISL_ERR_DIMENSION_MISMATCH (expected, actual); d == 0 -> ISL_ERR_EMPTY_COLLECTION; a non-empty index without
 * resident rows -> ISL_ERR_UNSUPPORTED; dtype != the stored type -> ISL_ERR_UNSUPPORTED; m0 > 128,
 * ef_construction > 512 or too many nodes -> ISL_ERR_UNSUPPORTED.  Refused once the import kernel has looked,
 * each with ISL_ERR_UNSUPPORTED and a message that says which: a list longer than m0; a device copy that is not
 * the lists verbatim (ids repeated inside a list were removed at upload); an id not below len. */
isl_status isl_index_insert(isl_index* idx, const isl_build_options* opts, const void* rows, int32_t dtype,
                            uint64_t n_new, uint64_t d, const uint64_t* levels, int32_t mem, uint64_t* first_id);
/* Rows out of a built index, in place (extension: the reference has no removal on LeannIndex).  ids = n_ids node
 * ids in host memory, repeated ids counting once: the set D.  opts = the selection rule of this call (select_rule,
 * alpha, keep_pruned; NULL: the defaults; batch is not used).  out_remap [old len] (may be NULL) receives the new
 * id of every old node or ISL_REMOVED, *out_len (may be NULL) the new len; both are written only on ISL_OK.
 * Definition, over a flat index with len nodes, lists L[p] in their stored order and resident rows:
 * 1. Repair over the old ids.  Every list is computed from the OLD lists only, so the result does not depend on
 *    the order in which nodes are processed.  For each survivor p: if no id of L[p] is in D, L'[p] = L[p].
 *    Otherwise the candidate list C(p): walk L[p] in stored order; a survivor x emits x; a removed x emits every y
 *    of L[x], in stored order, with y not in D and y != p; the first occurrence of every id is kept; the walk
 *    stops after ISL_REMOVE_MAX_CANDIDATES distinct ids (the builder's bound on a candidate list).  If |C(p)| <= m0,
 *    L'[p] = C(p) in that order.  If |C(p)| > m0: d(p, c) = Distance::calculate(vec[p], vec[c]) through the
 *    library's exact-order chain, C(p) stable-sorted ascending by it (NaN last, -0 == +0), then
 *    ISL_SELECT_REFERENCE keeps the first m0 (prune_neighbors_temp, leann.rs:634-658, the builder's re-sort) and
 *    ISL_SELECT_DIVERSE keeps select(p, sorted C(p), m0) as defined above.  high_degree_pruning / hub_percentile
 *    play no part, as in the builder's re-sort.  A survivor whose candidates are all gone ends with an EMPTY
 *    list: nothing is invented for it, and nothing may lead to it any more.
 * 2. Compaction, order kept.  A survivor's new id is its old id minus the number of removed ids below it; lists,
 *    levels, degree_counts, node_offsets and num_nodes follow.  Rows and norms of the survivors are copied bit
 *    for bit on the device, f32 or bf16: nothing is converted, no norm is computed again.  Entry point: one that
 *    survives is kept (remapped) and max_level stays; otherwise the new entry point is the lowest new id among the
 *    survivors of the highest level and max_level is that level, which is what LeannIndex::build leaves for those
 *    nodes (an index without entry point keeps none).  Removing every node leaves what isl_index_build_rows gives
 *    for n == 0 under the handle's config.
 * Strong guarantee: the shrunk graph is built beside the old one and moved into the handle at the end; on any
 * failure idx is unchanged (bytes, rows, search answers).  Peak device memory: the old index whole, plus the
 * (m0 + 1)-wide table over the old nodes, the shrunk CSR twice, its padded adjacency and the survivors' rows.
 * Reserved index (isl_index_reserve): repair, remap, the new CSR and the padded adjacency are built beside the old
 * graph as above, but no second row block is made.  Once they stand, under the handle's lock with no lane busy and
 * as the last step that can fail, the survivors' rows and norms move down inside the block bit for bit (new row j
 * takes old row s[j], s the ascending survivors; rows below the first removed id do not move; a destination is
 * written only once the row that lived there has been read, through a staging buffer of 64 MiB -- at least one row --
 * where sources and destinations of a move overlap; ISL_COMPACT_STAGE_ROWS overrides the rows per staged move) and
 * the vacated tail is zeroed.  The capacity is kept.  Every refusal and every allocation comes before the first
 * move, and a busy lane answers ISL_ERR_SEARCH with nothing moved; once moves have started only a device failure
 * can interrupt them, AND THE HANDLE'S ROWS ARE THEN UNDEFINED.  The peak above loses "the survivors' rows".
 * What the handle keeps: its config, the visited-table hint and its prepared lanes (none of their buffers
 * follows the node count), and its entry seeds REDUCED to the surviving seeds, under their new ids, their row
 * copies gathered again from the shrunk table as isl_index_set_entry_seeds gathers them (no seed left, or no
 * memory for the copies: no table, a plain search then starts at the entry point).  What goes: the heap-exact
 * kernel's pool (made again on demand) and the PQ codes, detached exactly as isl_index_insert detaches them.
 * The call is the reference's &mut self: not beside searches on the same handle.  Checked in this order before
 * any device call: NULL idx, or NULL ids with n_ids > 0 -> ISL_ERR_INVALID_ARGUMENT; opts as in
 * isl_index_build_ex; n_ids == 0 -> ISL_OK, nothing changed, out_remap the identity; the core index of an
 * HnswGraph or an index on the recompute provider -> ISL_ERR_UNSUPPORTED; an id >= len ->
 * ISL_ERR_NODE_NOT_FOUND (node); a non-empty index without resident rows -> ISL_ERR_UNSUPPORTED; m0 > 128 ->
 * ISL_ERR_UNSUPPORTED; a busy lane -> ISL_ERR_SEARCH.  Refused once the import kernel has looked, as
 * isl_index_insert refuses them, each with ISL_ERR_UNSUPPORTED and a message that says which: a list longer than
 * m0; a device copy that is not the lists verbatim; an id not below len. */
#define ISL_REMOVED UINT64_MAX
#define ISL_REMOVE_MAX_CANDIDATES 512u
isl_status isl_index_remove(isl_index* idx, const isl_build_options* opts, const uint64_t* ids, uint64_t n_ids,
                            uint64_t* out_remap /* [old len], may be NULL */, uint64_t* out_len /* may be NULL */);
/* select() of ISL_SELECT_DIVERSE for nb base nodes of an index whose f32 rows are on the device
 * (bf16 rows or a recompute provider -> ISL_ERR_UNSUPPORTED): cand_ids is [nb][pitch] in any order
 * (the call computes d(base, c) and stable-sorts), cand_cnt[i] <= min(pitch, 512), cap <= 128;
 * out_ids [nb][cap], out_cnt [nb].  Host buffers.  The device routine is the builder's.  The call
 * does not look for the base id or for repeated ids among the candidates: a repeated id is a
 * second entry at distance 0 from the first.  An id >= the number of rows ->
 * ISL_ERR_NODE_NOT_FOUND.  opts->select_rule and opts->batch are not used. */
isl_status isl_select_neighbors(const isl_index* idx, const isl_build_options* opts,
                                const uint64_t* base_ids, uint64_t nb, const uint64_t* cand_ids,
                                uint64_t pitch, const uint32_t* cand_cnt, uint64_t cap,
                                uint64_t* out_ids, uint32_t* out_cnt);

/* LeannIndex::from_bytes / to_bytes, leann.rs:1059-1066 (bincode 1.x default layout). */
isl_status isl_index_from_bytes(const uint8_t* bytes, size_t len, isl_index** out);
isl_status isl_index_to_bytes(const isl_index* idx, uint8_t** out, size_t* len);
void isl_free_bytes(uint8_t* p);
void isl_index_free(isl_index* idx);

/* ---- storage.rs: IndexMetadata (:16-47) and the chunk framing of IndexWriter / IndexReader ----
 * A chunk is tag[4] || u64 LE length || payload (:127-135, :159-173); the META chunk carries
 * serde_json::to_vec(&IndexMetadata) (:119-124).  `now` replaces chrono::Utc::now() (:37). */
typedef struct isl_index_metadata {
  uint32_t version;        /* IndexMetadata::CURRENT_VERSION = 1 */
  uint64_t num_vectors;
  uint64_t dimension;
  int64_t created_at;
  int64_t updated_at;
  int32_t has_description; /* Option<String> */
  char description[256];   /* NUL-terminated UTF-8 */
} isl_index_metadata;
void isl_index_metadata_new(uint64_t num_vectors, uint64_t dimension, int64_t now, isl_index_metadata* out);
/* IndexWriter::write_metadata on a buffer: the META chunk (free with isl_free_bytes). */
isl_status isl_storage_write_metadata(const isl_index_metadata* meta, uint8_t** out, size_t* len);
/* IndexReader::read_metadata on a buffer; *consumed = bytes of the chunk.  A different tag is
 * Deserialization("expected META chunk") (:151-153), a short buffer is Io. */
isl_status isl_storage_read_metadata(const uint8_t* bytes, size_t len, isl_index_metadata* meta,
                                     size_t* consumed);
/* One-file persistence: parents created like FileSystemStorage::save (:68-74), chunk META then
 * chunk "LIDX" = LeannIndex::to_bytes().  meta NULL = IndexMetadata::new(len, dimension) now. */
isl_status isl_index_save(const isl_index* idx, const char* path, const isl_index_metadata* meta);
isl_status isl_index_load(const char* path, isl_index** out, isl_index_metadata* meta);

uint64_t isl_index_len(const isl_index* idx);                 /* leann.rs:519-521 */
int32_t isl_index_is_empty(const isl_index* idx);             /* leann.rs:524-526 */
int32_t isl_index_dimension(const isl_index* idx, uint64_t* dim); /* 1 = Some, leann.rs:529 */
uint64_t isl_index_storage_bytes(const isl_index* idx);       /* leann.rs:534, 296-301 */
int32_t isl_index_is_recompute(const isl_index* idx);         /* leann.rs:539 */
int32_t isl_index_is_compact(const isl_index* idx);           /* leann.rs:544 */
isl_status isl_index_config(const isl_index* idx, isl_leann_config* out);
int32_t isl_index_entry_point(const isl_index* idx, uint64_t* entry); /* 1 = Some */
uint64_t isl_index_max_level(const isl_index* idx);
/* CsrGraph::get_neighbors, leann.rs:225-233: returns 1 (Some) / 0 (None).  The
 * slice stays valid until the index is freed. */
int32_t isl_index_get_neighbors(const isl_index* idx, uint64_t node, const uint64_t** ptr,
                                size_t* len);

/* Copy the CSR graph into HBM of `device` (u64 offsets, u32 neighbour ids). */
isl_status isl_index_upload(isl_index* idx, int32_t device);

/* InMemoryEmbeddingProvider::new, leann.rs:111-120: attach n rows of d
 * elements as the provider for this index.  `rows` is row-major, on the host
 * or already on the index's device (mem = ISL_MEM_*).  The handle keeps its
 * own HBM copy (rows padded to 16-byte multiples).  n == 0 -> EmptyCollection.
 * dtype ISL_DTYPE_BF16: `rows` holds bf16 bit patterns (u16) and is stored as such -- half the
 * HBM bytes per visited node; the provider's vectors are their exact f32 images and the
 * arithmetic stays the reference's f32 chain, so results equal the reference's on those f32
 * rows.  (The LeannIndex builder takes either type through isl_index_build_rows, the HnswGraph facade and its
 * builder through isl_hnsw_build_rows / isl_hnsw_insert_rows / isl_hnsw_from_layers_rows -- on the core index of a
 * facade this call itself keeps refusing anything but f32; isl_select_neighbors and the distance / PQ entry points
 * take f32.) */
isl_status isl_set_embeddings(isl_index* idx, const void* rows, uint64_t n, uint64_t d,
                              int32_t dtype, int32_t mem);

/* The same provider over fp8 rows: `codes` holds n x d bytes, each an OCP e4m3fn code (1 sign bit, 4 exponent
 * bits with bias 7, 3 mantissa bits; subnormals m * 2^-9, largest value 448, 0x7F and 0xFF are NaN, no
 * infinities -- not the fnuz encoding), and the table carries one power-of-two scale: the provider's vector
 * element of code c is e4m3(c) * 2^scale_exp, an exact float32.  A quarter of the HBM bytes of float32 rows per
 * visited node.  The arithmetic stays the reference's f32 chain over those images (queries stay float32), so
 * results equal the reference's on them: ids, distance bits, counters.  A NaN code is a NaN element; the upload
 * does not look for them.  Checks are those of isl_set_embeddings in the same order; scale_exp outside
 * [-32, 32] -> ISL_ERR_INVALID_ARGUMENT before any device call; the HnswGraph facade -> ISL_ERR_UNSUPPORTED.
 * isl_set_embeddings(..., ISL_DTYPE_FP8_E4M3, ...) is this call with scale_exp = 0.
 * Every plain search form runs over fp8 rows.  An index that holds them refuses, with ISL_ERR_UNSUPPORTED and
 * before any launch: isl_index_insert, isl_index_remove, isl_index_select_entry_seeds,
 * isl_index_set_entry_seeds (count > 0), isl_index_pick_entries and the two-level searches.  Attaching the
 * rows drops the entry seeds, as every provider swap does. */
isl_status isl_set_embeddings_fp8(isl_index* idx, const void* codes, uint64_t n, uint64_t d, int32_t scale_exp,
                                  int32_t mem);

/* What the index's in-memory rows cost: their stored type (ISL_DTYPE_*), the scale exponent (0 unless fp8) and
 * the bytes of the allocated row block in HBM (rows at their 16-byte-aligned pitch plus 1 KiB of slack; a reserved
 * index: the rows of its capacity, also while it holds no row -- type and scale are then reported as for a handle
 * without rows).  Any out pointer may be NULL.  No resident rows (none attached, or the recompute provider) -> ISL_DTYPE_F32, 0, 0. */
isl_status isl_index_row_storage(const isl_index* idx, int32_t* dtype, int32_t* scale_exp, uint64_t* block_bytes);

/* Room for rows that come and go (extension).  The row block and the norms of `idx` are allocated for `capacity`
 * rows; isl_index_insert then appends in place while len + n_new <= capacity and isl_index_remove compacts in
 * place, neither allocating a second row block (see there).  Every element of the block behind row len is zero, so
 * a reserved index answers every search bit for bit as one nobody reserved.
 * Non-empty index with resident rows (any stored type, fp8 included): d and dtype must be the stored ones.  The call
 * allocates one block of `capacity` rows, copies rows and norms bit for bit, zeroes the rest and moves the block in.
 * THIS IS THE ONE COPY A RESERVATION COSTS: for its length the old table and the new one both stand.  Strong
 * guarantee: on any failure the handle is unchanged.  capacity <= the current capacity -> ISL_OK with nothing
 * touched (a reservation never shrinks); a capacity below len is treated as len.  isl_index_convert_rows keeps the
 * capacity (the new table is allocated for the same number of rows: widen, insert, narrow keeps its reservation);
 * isl_set_embeddings* replaces the table and the reservation goes with it; an insert past the capacity uses it up.
 * Empty handle: the call fixes d and dtype (f32 or bf16) of the rows to come and allocates the table on the device
 * the handle was uploaded to, else on device 0 (isl_index_insert's rule; the handle then lives there).  new ->
 * reserve -> insert(all rows) is a one-call build without a second table, byte for byte isl_index_build_rows'
 * result at batch == 1; an insert of another d -> ISL_ERR_DIMENSION_MISMATCH, of another dtype ->
 * ISL_ERR_UNSUPPORTED.
 * Refused in this order, before any device call: NULL idx, an unknown dtype -> ISL_ERR_INVALID_ARGUMENT; the core
 * index of an HnswGraph, a recompute provider, a non-empty index without resident rows -> ISL_ERR_UNSUPPORTED;
 * d == 0 on an empty handle -> ISL_ERR_EMPTY_COLLECTION; capacity above the device id range -> ISL_ERR_UNSUPPORTED;
 * d != the stored dimension -> ISL_ERR_DIMENSION_MISMATCH (expected, actual); dtype != the stored type (an empty
 * handle: fp8) -> ISL_ERR_UNSUPPORTED; a busy lane, because the block's address changes -> ISL_ERR_SEARCH. */
isl_status isl_index_reserve(isl_index* idx, uint64_t capacity, uint64_t d, int32_t dtype);
/* *capacity_rows: rows the block is allocated for (len for an index nobody reserved, 0 without resident rows);
 * *row_allocations: how often a row block has been allocated for this handle -- a call that appends into or
 * compacts a reserved table leaves it unchanged.  A fresh handle: 0, 0.  Either pointer may be NULL. */
isl_status isl_index_capacity(const isl_index* idx, uint64_t* capacity_rows, uint64_t* row_allocations);

/* ---- row conversions on the device (extension) ----
 * image(x) is the exact float32 value of a stored element: the float itself, the bf16 bits shifted left by 16, or
 * e4m3(code) * 2^scale_exp.  Every conversion below is new = narrow_T(image(old)), element by element, defined bit
 * for bit (islands_amd/csrc/row_convert_plan.hpp is the definition in C++, islands_amd.f32_to_bf16_bits and
 * islands_amd.quantize_fp8_e4m3 in Python):
 *   narrow_f32      the identity.
 *   narrow_bf16     on the bit pattern b: not a NaN -> (b + 0x7FFF + ((b >> 16) & 1)) >> 16 (round to nearest, ties
 *                   to even; past the largest finite bf16 -> infinity); a NaN -> (b >> 16) | 0x0040 (sign kept, quiet).
 *   narrow_fp8(e)   y = min(|x| * 2^-e, 448) rounded to the nearest e4m3 value, ties to the even code, subnormal
 *                   spacing 2^-9; the sign bit of x is kept (-0.0 and negative values that round to zero give 0x80);
 *                   infinities saturate to +-448; a NaN is an error, not a code.
 * The automatic exponent (ISL_FP8_SCALE_AUTO) is the smallest e in [-32, 32] with max|x| <= 448 * 2^e: all zeros
 * give -32, anything above 448 * 2^32, infinity included, gives 32 and saturates. */
#define ISL_FP8_SCALE_AUTO INT32_MIN

/* n x d float32 -> n x d e4m3 codes (dense, no padding), host or device buffers alike (mem).
 * scale_exp: an exponent in [-32, 32] or ISL_FP8_SCALE_AUTO.
 * *out_scale_exp (may be NULL) receives the exponent used.
 * Checked before any device call: NULL buffers with n * d > 0, an unknown mem, a scale_exp that is neither ->
 * ISL_ERR_INVALID_ARGUMENT; n * d == 0 -> ISL_OK (*out_scale_exp = -32 under AUTO).  A NaN among the rows ->
 * ISL_ERR_INVALID_ARGUMENT with a message that says so; *out_scale_exp is then not written and the codes are
 * undefined.  Runs on `stream` and is synchronised before returning. */
isl_status isl_quantize_fp8_e4m3(const float* rows, uint64_t n, uint64_t d, int32_t scale_exp,
                                 uint8_t* codes, int32_t* out_scale_exp,
                                 int32_t mem, int32_t device, void* stream);

/* n x d float32 -> bf16 bit patterns by narrow_bf16.  Checks and synchronisation as above. */
isl_status isl_round_bf16(const float* rows, uint64_t n, uint64_t d, uint16_t* bits,
                          int32_t mem, int32_t device, void* stream);

/* The index's resident rows become rows of `dtype`: narrow_dtype(image(old)), on the device.
 * scale_exp is read only for ISL_DTYPE_FP8_E4M3 (AUTO: taken from the images).
 * Narrowing lets an index be built in f32 and served in a quarter of the bytes; widening is lossless and gives an
 * fp8 index its lifecycle back: widen, isl_index_insert / isl_index_remove, narrow again under the same scale.
 * Checks and refusals in this order: NULL idx, an unknown dtype, or target fp8 with scale_exp neither AUTO nor in
 * [-32, 32] -> ISL_ERR_INVALID_ARGUMENT; the core index of an HnswGraph -> ISL_ERR_UNSUPPORTED; a recompute
 * provider or no resident rows -> ISL_ERR_UNSUPPORTED; a busy lane -> ISL_ERR_SEARCH; the stored type itself ->
 * ISL_OK with nothing touched (fp8: under AUTO or the stored exponent; another exponent -> ISL_ERR_UNSUPPORTED);
 * a NaN image with target fp8 -> ISL_ERR_INVALID_ARGUMENT.
 * Strong guarantee: the new table is allocated and filled beside the old one and moved in at the end; on any
 * failure the handle is unchanged (bytes, rows, seeds, search answers).  Peak extra device memory: the new block,
 * its norms and the norm chunk buffer.  The norms of the new table are computed from its images by the routine
 * isl_set_embeddings uses: bit for bit what isl_set_embeddings[_fp8] of the same elements gives.
 * What the handle keeps: config, graph, host CSR, visited-table hint, prepared lanes, the heap-exact pool and PQ
 * codes.  Target f32 or bf16: the entry seeds keep their ids and their row copies are gathered again from the
 * converted table (as isl_index_remove does for survivors).  Target fp8: the entry seeds go. */
isl_status isl_index_convert_rows(isl_index* idx, int32_t dtype, int32_t scale_exp);

/* Rows [first, first + count) in their stored type, dense (count x d elements, no padding),
 * to host or device memory.  The residency checks are those of the conversion (the core index of an HnswGraph
 * may be read); first + count > the number of rows -> ISL_ERR_NODE_NOT_FOUND naming the first id that has no row.
 * The call only reads: it needs no idle lanes. */
isl_status isl_index_read_rows(const isl_index* idx, uint64_t first, uint64_t count,
                               void* out, int32_t mem);

/* ---- search ---- */
/* Work counters of one search call (summed over the batch): the inputs of the roofline formula
 * (SURVEY.md section 8d). */
typedef struct isl_search_stats {
  uint64_t queries;
  uint64_t expansions;     /* H: candidates expanded */
  uint64_t edges;          /* E: neighbour ids read */
  uint64_t evals;          /* V: embeddings fetched / distances evaluated (an index with entry seeds: the
                              pick's evaluations against its L2-resident seed table are not counted) */
  uint64_t pushes;         /* heap insertions */
  uint64_t exact_path;     /* queries answered by the heap-exact kernel */
  uint64_t replayed;       /* queries whose tied prefix was re-ordered by the replay kernel */
  double kernel_ms;        /* HIP-event time of the search kernels of that call */
  uint64_t encoded_nodes;    /* recompute provider: embeddings computed by the encoder */
  uint64_t recompute_rounds; /* recompute provider: search rounds of that call (0 otherwise) */
  uint64_t allocations;    /* device / pinned-host allocations and stream / event creations the
                              call had to make (0 for every call that fits isl_index_prepare) */
} isl_search_stats;

/* Sets up everything a search needs so that no later call allocates, creates a stream or
 * synchronises for set-up: `lanes` (1..32) search lanes sized for batches of up to max_nq queries
 * with ef <= max_ef and k <= max_k (streams, events, per-query arrays, overflow tables, push
 * logs, pinned staging buffers for the host-pointer entry points), the padded adjacency, the
 * shared scratch pool of the heap-exact kernel, and one empty launch of the search kernels on
 * every lane's stream (code objects loaded, hardware queues created).  Call it after
 * isl_index_upload + a provider setter.  Lanes run on a per-device pool of at most 16 HIP streams
 * (ISL_MAX_STREAMS; a card serves about that many hardware queues side by side and the rate
 * collapses beyond): lanes past the pool's size share streams, their calls queue in stream order.
 * The reference has no such step (its search allocates
 * per call, leann.rs:903-908); without it the first calls on each lane do this work lazily and
 * report it in isl_search_stats::allocations. */
isl_status isl_index_prepare(isl_index* idx, uint64_t max_nq, uint64_t max_ef, uint64_t max_k,
                             int32_t lanes);

/* LeannIndex::search_with_params over a batch of queries (leann.rs:868-896;
 * batch = Searcher::search_batch semantics, search.rs:179-181: each query is
 * answered independently, results in query order).
 *   queries: nq rows of d floats; out_ids/out_dist: nq*k slots, row i holds
 *   out_count[i] <= k valid entries, ascending distance.
 * Errors that the reference raises per query (NodeNotFound) fail the whole
 * call with the first failing query's error, as the sequential map would.
 * Host buffers in, host buffers out (the caller contract of search.rs:150-181,
 * indexer/service.rs:781-785); re-entrant: concurrent calls run on different lanes. */
isl_status isl_search_batch(const isl_index* idx, const float* queries, uint64_t nq, uint64_t d,
                            uint64_t k, uint64_t ef, uint64_t* out_ids, float* out_dist,
                            uint32_t* out_count);
/* Pipelined form of isl_search_batch: copies `queries` into the lane's pinned staging buffer
 * (they may be reused as soon as the call returns), enqueues H2D copy, search and D2H copies on
 * the lane's stream and returns.  out_ids / out_dist / out_count must stay valid until
 * isl_search_wait[_stats](*token) has returned; they are written there.  Up to 32 calls may be
 * in flight.  token 0 = answered immediately (empty index, nq == 0). */
isl_status isl_search_batch_async(const isl_index* idx, const float* queries, uint64_t nq, uint64_t d,
                                  uint64_t k, uint64_t ef, uint64_t* out_ids, float* out_dist,
                                  uint32_t* out_count, uint64_t* token);
/* Same with every buffer already on the index's device; enqueued on `stream`
 * (NULL = the legacy default stream, i.e. ordered after the caller's earlier
 * default-stream work) and synchronised before returning (status needs the result). */
isl_status isl_search_batch_device(const isl_index* idx, const float* d_queries, uint64_t nq,
                                   uint64_t d, uint64_t k, uint64_t ef, uint64_t* d_out_ids,
                                   float* d_out_dist, uint32_t* d_out_count, void* stream);
/* Asynchronous form: enqueues the search on one of the index's private streams (ordered after
 * the work already enqueued on `stream`) and returns at once; up to 32 searches may be in
 * flight, so consecutive batches overlap and the slowest queries of one batch no longer idle
 * the chip.  Outputs are valid and the per-query status is reported once isl_search_wait
 * returns for *token (token 0 = the call was answered immediately).  An index with the recompute
 * provider is accepted too (this form and isl_search_batch_async): the provider works through the
 * batch in rounds -- search, encode what was missed, resume -- on a host thread of the library's,
 * one set of rounds at a time per index; isl_search_stream_wait then waits on the host.  Calls of
 * this form (and of isl_search_batch_async and isl_search_two_level_batch_device_async) that are waiting for their turn are
 * answered TOGETHER by the call that gets it, when they agree in d, k, ef and search kind: one set of
 * rounds over the union of their queries, so a node several of them need is encoded once and the
 * encoder gets fuller passes (Searcher::search_batch, search.rs:179-181, hands batches over one by one;
 * how they are batched on the device is the library's business).  Each call's answers, status and
 * counters are its own (recompute_rounds / encoded_nodes of its statistics are the shared rounds'); if
 * the union fails, every member is run by itself and gets its own error.
 *
 * In-memory provider: a call of this form that finds the chip full -- at least as many queries of the
 * index in flight as the call's launch has resident waves -- is HELD, not enqueued: a process has only a
 * few hardware queues (GPU_MAX_HW_QUEUES, 4 unless set before HIP starts), in one queue the next call's
 * kernel starts only when the previous call's slowest query has finished, so the call would wait on the
 * device anyway.  Held calls that agree in d, k and ef go out TOGETHER as one launch over the union of
 * their queries: when they reach ISL_GROUP_CAP queries (default 4096), at the next entry into the library
 * that finds room (another call of this form, isl_search_wait[_stats], isl_search_stream_wait), or when
 * one of them is waited for.  Each call keeps its token, its output buffers, its status and its counters;
 * kernel_ms of its statistics is then the shared launch's.  Calls are held only in a process that had
 * GPU_MAX_HW_QUEUES below 8 in its environment when the library was loaded (or none: HIP's default is 4);
 * with more queues every call is enqueued at once, as ISL_NO_GROUP=1 makes it everywhere (ISL_NO_GROUP=0:
 * held whatever the queues).  A caller that wants a call started at once leaves room or sets
 * ISL_NO_GROUP=1 (read, like ISL_GROUP_CAP and ISL_GROUP_ROOM, when the index handle is created).
 * Recompute provider, two-level search, HnswGraph, host-buffer calls and runs with
 * ISL_TIMELINE / ISL_DEBUG keep one launch per call. */
isl_status isl_search_batch_device_async(const isl_index* idx, const float* d_queries, uint64_t nq,
                                         uint64_t d, uint64_t k, uint64_t ef, uint64_t* d_out_ids,
                                         float* d_out_dist, uint32_t* d_out_count, void* stream,
                                         uint64_t* token);
/* Completes the call `token` names: waits for its stream, copies host-pointer results out, turns
 * per-query failures into the CoreError of the first failing query.  `stats` (may be NULL)
 * receives the counters of exactly that call. */
isl_status isl_search_wait_stats(const isl_index* idx, uint64_t token, isl_search_stats* stats);
isl_status isl_search_wait(const isl_index* idx, uint64_t token);
/* Makes `stream` wait (on the device, no host synchronisation) for the search kernels of the call
 * `token` names: what a consumer of the device-resident answers enqueues on its own stream -- the
 * shard exchange of a multi-GPU search issues its all-gather behind this -- while the host keeps
 * submitting.  The call still has to be completed with isl_search_wait[_stats]. */
isl_status isl_search_stream_wait(const isl_index* idx, uint64_t token, void* stream);
/* How the asynchronous device-pointer calls of this index went out so far: launches submitted by the
 * group path, those of them that served several calls, and the calls those served.  Zeros for an index
 * no such call has reached.  Any of the pointers may be NULL. */
isl_status isl_index_group_counters(const isl_index* idx, uint64_t* launches, uint64_t* shared_launches,
                                    uint64_t* shared_calls);
/* The calls the group path took so far, and those of them that found work pending on their caller's stream
 * and put a marker (an event record) on it, for their launch to wait for.  A call whose caller's stream has
 * nothing pending puts none: in a process of few hardware queues the caller's stream shares a queue with the
 * library's launches, and a marker in it is reached only after the kernel in front of it has ended.
 * ISL_GROUP_MARK=1 marks every call.  Either pointer may be NULL. */
isl_status isl_index_group_markers(const isl_index* idx, uint64_t* calls, uint64_t* marked_calls);
/* LeannIndex::search, leann.rs:858-865: one query, ef = config.ef_search. */
isl_status isl_search(const isl_index* idx, const float* query, uint64_t d, uint64_t k,
                      uint64_t* out_ids, float* out_dist, uint32_t* out_count);

/* Counters of the most recent search call THIS THREAD completed on this index (synchronous entry
 * points and isl_search_wait alike); zeros when there is none.  Calls made by other threads never
 * show up here -- use isl_search_wait_stats for a per-call record. */
isl_status isl_search_last_stats(const isl_index* idx, isl_search_stats* out);

/* ---- entry seeds (extension; the reference enters every search at entry_point, leann.rs:911) ----
 * A LeannIndex may carry an entry-seed table: E node ids plus a contiguous device copy of their rows.
 * While the table is non-empty every plain search of the index -- isl_search, isl_search_batch, _async,
 * _device, _device_async and each shard of a sharded submit -- starts query q at
 *   pick(q) = the seed at the smallest position p minimising Distance::calculate(metric, q, x[seeds[p]])
 * in the search's total order of distances (-0 == +0, NaN last), and is otherwise the reference's search:
 * ids, distances, count and the H / E / V / push counters are those of the reference search of the same
 * graph with entry_point = pick(q).  The pick's own E evaluations are NOT in V: the table stays resident
 * in L2 and adds no HBM row traffic, which is what V stands for in the roofline formula; V counts the
 * entry node once, as always.  Two-level searches and searches over the recompute provider IGNORE the
 * table and keep entry_point.  With no table (the default) nothing changes: no launch, buffer or counter.
 * The table is dropped by whatever replaces the rows it copied (isl_set_embeddings,
 * isl_set_recompute_provider, a fresh isl_index_upload) and is not part of isl_index_to_bytes /
 * isl_index_save, which are the reference's format: keep the ids from isl_index_entry_seeds and set them
 * again after a load.  Setting or selecting while searches are in flight -> ISL_ERR_SEARCH, as
 * isl_index_prepare.  An isl_index_prepare made after the seeds are set covers the pick's buffers
 * (isl_search_stats::allocations stays 0).  ISL_ENTRY_SEEDS=N in the environment makes isl_index_build,
 * isl_index_build_ex and isl_index_build_rows select N seeds for the index they return (unset or 0: none;
 * not a decimal count -> ISL_ERR_INVALID_ARGUMENT; above the cap -> ISL_ERR_UNSUPPORTED).
 * Common errors: a NULL index -> ISL_ERR_INVALID_ARGUMENT; count > ISL_MAX_ENTRY_SEEDS -> ISL_ERR_UNSUPPORTED;
 * the index of an HnswGraph -> ISL_ERR_UNSUPPORTED; an empty index -> ISL_ERR_EMPTY_COLLECTION; no rows
 * resident on the device (none attached, or the recompute provider) -> ISL_ERR_UNSUPPORTED. */
#define ISL_MAX_ENTRY_SEEDS 65536ull
/* Greedy k-centre selection of min(count, len) seeds, installed as the index's table (count == 0 clears it):
 *   seeds[0] = entry_point;  mind[r] = D(x[seeds[0]], x[r]) for every row r;
 *   repeat: j = the row not yet chosen with the largest mind[j] (ties: the smaller id); seeds += j;
 *           mind[r] = min(mind[r], D(x[j], x[r]))
 * with D(a, b) = Distance::calculate(metric, a, b) (the seed is a), bf16 rows as their f32 images, min / largest
 * in the total order above.  One pass over the rows per seed, no host round trip between passes.
 * out_ids (may be NULL) receives the ids in selection order, *out_count (may be NULL) their number. */
isl_status isl_index_select_entry_seeds(isl_index* idx, uint64_t count, uint64_t* out_ids, uint64_t* out_count);
/* Installs the caller's seeds (count == 0 clears the table).  Repeated ids are accepted (the pick's tie rule
 * makes them harmless); an id >= len (or without a row) -> ISL_ERR_NODE_NOT_FOUND with the id. */
isl_status isl_index_set_entry_seeds(isl_index* idx, const uint64_t* ids, uint64_t count);
/* *count = seeds in the table; the first min(cap, *count) ids go to `out` (NULL with cap == 0). */
isl_status isl_index_entry_seeds(const isl_index* idx, uint64_t* out, uint64_t cap, uint64_t* count);
/* out_ids[q] = seeds[pick(q)] for nq queries of d floats (d != the rows' -> ISL_ERR_DIMENSION_MISMATCH; no table
 * -> ISL_ERR_INVALID_ARGUMENT).  mem applies to queries and out_ids alike; runs on `stream` and is synchronised
 * before returning.  Must not run concurrently with the two setters above. */
isl_status isl_index_pick_entries(const isl_index* idx, const float* queries, uint64_t nq, uint64_t d,
                                  uint64_t* out_ids, int32_t mem, void* stream);

/* ---- graph reachability (extension; the reference has no such report) ----
 * A breadth-first walk over the graph as the device holds it, and entry seeds chosen with it.
 * The graph of a LeannIndex: nodes 0 .. len-1, list(u) = the distinct ids of isl_index_get_neighbors(u) (the device
 * copy keeps the first occurrence of an id within a row).  The graph of layer l of an HnswGraph: the population is
 * the nodes with level >= l, list(u) = isl_hnsw_get_neighbors(u, l) as the device holds it (the builders never
 * repeat an id within a list; a graph handed over with a repeated id in an upper-layer list counts every occurrence).
 * An id in list(u) that names no node of the population (>= len, or below the layer) is a DANGLING edge: counted,
 * never followed -- the search kernels skip such ids too.  A self-loop is an ordinary edge.
 * Given a set of sources, depth[v] = the least number of edges from any source to v (sources: 0),
 * ISL_DEPTH_UNREACHED for a node of the population no source reaches, ISL_DEPTH_ABSENT for a node that is not on
 * the layer (HnswGraph only).  in_degree[v] = the number of nodes u of the population, u == v included, whose list
 * names v; 0 for absent nodes.  Every output is independent of the order in which the device runs.
 * The walk expands every reached node once.  isl_reach_report is eight uint64_t, 64 bytes:
 *   nodes           the population
 *   sources         distinct sources
 *   reached         nodes with depth != UNREACHED, sources included
 *   levels          max depth + 1
 *   edges           edges followed: the ids in the lists of reached nodes that name a node of the population
 *   dangling_edges  the ids in the lists of reached nodes that do not
 *   no_inbound      nodes of the population with in_degree 0 (wherever they are, reached or not)
 *   max_in_degree
 * sources is a host array, repeats accepted; NULL with n_sources == 0 selects the starts a plain search uses: for
 * a LeannIndex the entry-seed table if it is non-empty, else entry_point; for an HnswGraph its entry point.
 * out_depth / out_in_degree: [len] uint32_t in `mem` (host or the graph's device), either may be NULL, as may report.
 * Only the graph has to be on the device: no rows need be attached, and f32, bf16, fp8 rows or the recompute
 * provider make no difference.  Errors, in this order: a NULL handle, an unknown mem, sources NULL with n_sources > 0
 * -> ISL_ERR_INVALID_ARGUMENT; layer > max_level -> ISL_ERR_INVALID_ARGUMENT; an empty graph ->
 * ISL_ERR_EMPTY_COLLECTION; no sources given and no entry point -> ISL_ERR_INDEX_NOT_BUILT; a source >= len or not on
 * the layer -> ISL_ERR_NODE_NOT_FOUND with the id; a graph that is not on a device -> ISL_ERR_UNSUPPORTED.
 * The calls only read the graph, allocate their own scratch (about 16 bytes per node) and run on a stream of their
 * own, synchronised before they return: they may run beside searches, and must not run beside a call that changes
 * the graph (insert, remove, upload) -- the rule of isl_index_pick_entries. */
#define ISL_DEPTH_UNREACHED 0xFFFFFFFFu
#define ISL_DEPTH_ABSENT 0xFFFFFFFEu
typedef struct isl_reach_report {
  uint64_t nodes, sources, reached, levels, edges, dangling_edges, no_inbound, max_in_degree;
} isl_reach_report;
isl_status isl_index_reachability(const isl_index* idx, const uint64_t* sources, uint64_t n_sources,
                                  uint32_t* out_depth, uint32_t* out_in_degree, int32_t mem, isl_reach_report* report);
/* (isl_hnsw_reachability: with the HnswGraph calls below) */
/* Entry seeds with a guarantee, by this loop over the walk above:
 *   S = the current seed table if it is non-empty, else [entry_point];  R = the nodes reachable from S
 *   while R != all nodes and |S| < max_seeds:
 *     j = the smallest id not in R;  S += [j];  R |= the nodes reachable from j
 * If the loop added an id, S becomes the index's table exactly as isl_index_set_entry_seeds(S) would make it (the
 * earlier table stays as its prefix); if it added none the table is left as it was, and an index without a table
 * stays without one.  *out_count = the table's size after the call, out_ids (may be NULL, room for max_seeds) its
 * ids, *out_unreached = the rows the table still does not reach: non-zero only where max_seeds ended the loop.
 * THE GUARANTEE: with *out_unreached == 0 every row is reachable from SOME seed of the table.  It does not say that
 * the greedy search that starts at the seed PICKED for a query (the nearest one) finds a given row: a search of
 * bounded ef may stop short of it, and the row may be reachable only from another seed.
 * Preconditions, refusals and the "no search in flight" rule are those of isl_index_select_entry_seeds, each checked
 * before anything is touched: max_seeds > ISL_MAX_ENTRY_SEEDS, the index of an HnswGraph, no rows resident on the
 * device (none attached, or the recompute provider), fp8 rows -> ISL_ERR_UNSUPPORTED; an empty index ->
 * ISL_ERR_EMPTY_COLLECTION; searches in flight -> ISL_ERR_SEARCH. */
isl_status isl_index_cover_entry_seeds(isl_index* idx, uint64_t max_seeds, uint64_t* out_ids, uint64_t* out_count,
                                       uint64_t* out_unreached);

/* ---- refined search (extension; the reference scores every candidate against the rows it traverses) ----
 * An index may carry a REFINE TABLE: a second table y of len x d elements, f32 or bf16 (bf16 rows count as their
 * exact f32 images, as everywhere), independent of the provider's rows.  A refined search traverses the provider's
 * rows -- narrow ones, fp8 or bf16, are the point -- and re-scores the `candidates` best of them against y:
 *   isl_search_refined_batch[_device](q, k, candidates, ef)  IS  isl_search_batch_device(q, candidates, ef)
 *   followed by the rescoring of its output rows (below); the inner search is the existing one with its entry
 *   seeds, stored row type, per-query errors and counters, and isl_search_last_stats reports ITS counters (the
 *   rescoring's evaluations are not in V).
 * Rescoring one query q with candidate ids cand[0 .. c) and k:
 *   s_i = Distance::calculate(metric, q, y[cand[i]]) in the reference's order of operations (cosine: norm_b is the
 *   precomputed sum of squares of the row); the answer is the first min(k, c') candidates in ascending order of
 *   (key(s_i), i), key = the search's total order of distances (-0 == +0, NaN last): among equal scores the EARLIER
 *   position wins.  The distances written are the s_i.  c' counts the candidates with cand[i] < len: an id that
 *   names no row is skipped, neither scored nor counted.  A repeated id is scored where it stands and may appear
 *   twice.  Limits: c <= ISL_REFINE_MAX_CANDIDATES, k <= pitch.
 * Placement: ISL_REFINE_DEVICE keeps y in a row table like the provider's (same pitch and slack rules);
 * ISL_REFINE_HOST keeps it in ONE block of pinned, device-mapped host memory at the same pitch, allocated by the
 * library, which the kernel reads across the bus through its device pointer (no XNACK, no managed memory): one
 * query touches `candidates` rows, so the wide rows of an index need no HBM.  In both placements the sums of squares
 * live on the device and come from the routine isl_set_embeddings uses: bit for bit the provider's norms for the
 * same elements.
 * The table is dropped by isl_index_insert and isl_index_remove (they change the node count) and by n == 0; it is
 * kept by isl_set_embeddings*, isl_index_convert_rows, isl_index_reserve and the entry-seed setters -- the intended
 * flow is build(rows), isl_index_set_refine_rows(rows, ISL_REFINE_HOST), isl_index_convert_rows(fp8).  It is not part
 * of isl_index_to_bytes / isl_index_save, which are the reference's format. */
enum { ISL_REFINE_DEVICE = 0, ISL_REFINE_HOST = 1 };
#define ISL_REFINE_MAX_CANDIDATES 512u
/* rows: n x d elements of `dtype` (ISL_DTYPE_F32 or ISL_DTYPE_BF16 bit patterns), dense, in host memory or on the
 * index's device (mem = ISL_MEM_*).  Checks and refusals in this order, before any device call: NULL idx, or NULL
 * rows with n > 0 -> ISL_ERR_INVALID_ARGUMENT; an unknown dtype, mem or placement -> ISL_ERR_INVALID_ARGUMENT; fp8 ->
 * ISL_ERR_UNSUPPORTED; the core index of an HnswGraph -> ISL_ERR_UNSUPPORTED; an index that is not on a device ->
 * ISL_ERR_UNSUPPORTED; n == 0 -> the table is dropped, ISL_OK; n != isl_index_len -> ISL_ERR_INVALID_ARGUMENT naming
 * both; d == 0 -> ISL_ERR_EMPTY_COLLECTION; the index has a dimension and d differs -> ISL_ERR_DIMENSION_MISMATCH; a
 * busy lane -> ISL_ERR_SEARCH.  Strong guarantee: the new table is made beside the old one and moved in at the end. */
isl_status isl_index_set_refine_rows(isl_index* idx, const void* rows, uint64_t n, uint64_t d,
                                     int32_t dtype, int32_t mem, int32_t placement);
/* The refine table's stored type, placement, row count (0: no table) and the bytes of its row block (device memory
 * for ISL_REFINE_DEVICE, pinned host memory for ISL_REFINE_HOST).  Any out pointer may be NULL. */
isl_status isl_index_refine_storage(const isl_index* idx, int32_t* dtype, int32_t* placement,
                                    uint64_t* rows, uint64_t* block_bytes);
/* The rescoring alone, every buffer on the index's device.  Enqueue only: no synchronisation, no allocation; it
 * composes behind any search via stream order or isl_search_stream_wait.  d_cand_ids: [nq][pitch] u64 of which
 * d_cand_count[q] <= pitch are valid in row q (what lies behind them is not read); d_out_ids / d_out_dist: [nq][k],
 * d_out_count: [nq].  Refusals as for the refined search below (pitch in the place of candidates). */
isl_status isl_rescore_device(const isl_index* idx, const float* d_queries, uint64_t nq, uint64_t d,
                              const uint64_t* d_cand_ids, const uint32_t* d_cand_count, uint64_t pitch,
                              uint64_t k, uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count,
                              void* stream);
/* ... with host buffers in and out (what the C++ and Python mirrors' rescore() call): staged through the handle's
 * scratch on the legacy default stream, synchronised before returning; slots behind out_count[q] are zero. */
isl_status isl_rescore(const isl_index* idx, const float* queries, uint64_t nq, uint64_t d, const uint64_t* cand_ids,
                       const uint32_t* cand_count, uint64_t pitch, uint64_t k, uint64_t* out_ids, float* out_dist,
                       uint32_t* out_count);
/* The plain search with k = candidates, then the rescoring, on one stream with no host round trip in between;
 * synchronised before returning, like isl_search_batch_device.  The scratch for the inner answers (nq x candidates
 * ids and distances, nq counts) is the handle's and is reused; concurrent calls are safe, one set per call in
 * flight.  A call that had to grow it adds to isl_search_stats::allocations; the next call of the same shape adds
 * nothing.  Refusals, in this order: NULL pointers with nq > 0 -> ISL_ERR_INVALID_ARGUMENT; no refine table ->
 * ISL_ERR_INVALID_ARGUMENT; k == 0, k > candidates or candidates > ef -> ISL_ERR_INVALID_ARGUMENT; candidates above
 * ISL_REFINE_MAX_CANDIDATES -> ISL_ERR_UNSUPPORTED; d != the table's -> ISL_ERR_DIMENSION_MISMATCH; the recompute
 * provider or the core index of an HnswGraph -> ISL_ERR_UNSUPPORTED.  nq == 0 -> ISL_OK. */
isl_status isl_search_refined_batch_device(const isl_index* idx, const float* d_queries, uint64_t nq,
                                           uint64_t d, uint64_t k, uint64_t candidates, uint64_t ef,
                                           uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count,
                                           void* stream);
/* ... with host buffers in and out. */
isl_status isl_search_refined_batch(const isl_index* idx, const float* queries, uint64_t nq, uint64_t d,
                                    uint64_t k, uint64_t candidates, uint64_t ef, uint64_t* out_ids,
                                    float* out_dist, uint32_t* out_count);

/* ---- distance.rs ---- */
/* Distance::calculate, distance.rs:38-52. */
isl_status isl_distance(int32_t metric, const float* a, uint64_t na, const float* b, uint64_t nb,
                        float* out);
/* Distance::calculate_squared, distance.rs:54-66. */
isl_status isl_distance_squared(int32_t metric, const float* a, uint64_t na, const float* b,
                                uint64_t nb, float* out);
/* Distance::batch_calculate, distance.rs:32-34: query against n contiguous
 * rows of `row_len` floats (row_len != d -> DimensionMismatch). mem applies
 * to query, rows and out alike. */
isl_status isl_distance_batch(int32_t metric, const float* query, uint64_t d, const float* rows,
                              uint64_t n, uint64_t row_len, float* out, int32_t mem, int32_t device,
                              void* stream);
/* normalize_vector, distance.rs:125-132, over n rows in place. */
isl_status isl_normalize_rows(float* rows, uint64_t n, uint64_t d, int32_t mem, int32_t device,
                              void* stream);

/* Every (query, row) distance at once as one GEMM on the matrix cores (float32 MFMA): the
 * batch_calculate of distance.rs:32-34 / benches/vector_ops.rs:60-79 for a whole query batch.
 * out [nq][n].  Cosine, Euclidean (sqrt(|q|^2 + |r|^2 - 2 q.r), clamped at 0) and DotProduct;
 * Manhattan is not a contraction (Unsupported).  The MFMA accumulates in its own order: values
 * agree with the sequential reference sums to float32 rounding, not bit for bit -- the search
 * itself keeps the exact-order kernels. */
isl_status isl_distance_matrix(int32_t metric, const float* queries, uint64_t nq, const float* rows,
                               uint64_t n, uint64_t d, float* out, int32_t mem, int32_t device,
                               void* stream);
/* Exact k nearest rows of every query by brute force over isl_distance_matrix blocks (ties
 * towards the smaller id): the ground truth of recall measurements. */
isl_status isl_bruteforce_topk(int32_t metric, const float* queries, uint64_t nq, const float* rows,
                               uint64_t n, uint64_t d, uint64_t k, uint64_t* out_ids, float* out_dist,
                               uint32_t* out_count, int32_t mem, int32_t device, void* stream);

/* ---- search.rs / indexer merge (multi-index = multi-shard) ---- */
/* MultiIndexSearcher::search merge, search.rs:211-237: per query, nlists
 * candidate lists (list-major: [list][query][k]) concatenated in list order,
 * stable-sorted by score ascending, truncated to top_k.  id_base[l] is added to
 * list l's ids (global id = shard base + local id).  counts: [list][query]. */
isl_status isl_merge_topk(uint64_t nlists, uint64_t nq, uint64_t k, const uint64_t* ids,
                          const float* scores, const uint32_t* counts, const uint64_t* id_base,
                          uint64_t top_k, uint64_t* out_ids, float* out_scores,
                          uint32_t* out_src, uint32_t* out_count, int32_t mem, int32_t device,
                          void* stream);
/* The same merge for the multi-GPU exchange, asynchronous and allocation-free: every
 * shard's answers arrive as one packed record of `list_stride` bytes -- ids u64[nq][k], then
 * distances f32[nq][k], then counts u32[nq] (isl_shard_record_bytes) -- which is what one
 * all-gather delivers in rank order.  Everything lives on the device (d_id_base: u64[nlists]);
 * the kernel is enqueued on `stream` and nothing is waited for.  *d_flags (u32, zeroed by the
 * caller once) collects bit 0 = a NaN score met (the reference panics, search.rs:231), bit 1 =
 * a list was not ascending, bit 2 = a list carried ISL_SHARD_POISON_COUNT as a query's count (its
 * producer failed that query: the list counts as empty); read it when the results are consumed. */
#define ISL_SHARD_POISON_COUNT 0xFFFFFFFFu
uint64_t isl_shard_record_bytes(uint64_t nq, uint64_t k);
isl_status isl_merge_topk_packed_async(uint64_t nlists, uint64_t nq, uint64_t k, const void* d_records,
                                       uint64_t list_stride, const uint64_t* d_id_base, uint64_t top_k,
                                       uint64_t* d_out_ids, float* d_out_scores, uint32_t* d_out_src,
                                       uint32_t* d_out_count, uint32_t* d_flags, int32_t device, void* stream);
/* ---- multi-GPU: the index sharded by node-id range, one process (rank) per GPU ----
 * Semantics = MultiIndexSearcher::search (src/core/search.rs:211-237) and the product's cross-index
 * merge (src/indexer/service.rs:775-801) with one sub-index per rank: every rank answers the whole
 * query batch in its own sub-graph (local ids), the per-rank top-k lists are concatenated in rank
 * order, stable-sorted by distance (ties -> the lower rank) and truncated to k; global id = the
 * rank's id base + local id.  The exchange is ONE collective per batch -- an all-gather of every
 * rank's packed answer record (isl_shard_record_bytes) -- issued on a side stream behind a device
 * event of the search, followed by the merge kernel on that stream: the host only submits, and the
 * exchange of batch i overlaps the traversals of batches i+1.. on the index's lanes.
 *
 * isl_shard_group = the communicator of the R ranks.  Two transports:
 *   - RCCL (xGMI): rank 0 calls isl_shard_unique_id, hands the 128 bytes to every rank by whatever
 *     means the host has (the reference product would use its own RPC; the tests use a store), and
 *     every rank calls isl_shard_group_create -- ncclCommInitRank, collective over the ranks.
 *     librccl.so is loaded on first use (the copy already in the process, if any).
 *   - host: `allgather(user, send, recv, bytes)` is a blocking all-gather of `bytes` from every rank
 *     into recv (rank-major) over host memory, supplied by the caller (MPI, gloo, a socket ...): for
 *     boxes without xGMI between the ranks' cards and for tests where ranks share one card.  The
 *     exchange is then synchronous inside isl_sharded_submit.
 * world == 1 needs no group (pass NULL to isl_sharded_searcher_new).
 *
 * Failure across ranks: MultiIndexSearcher::search propagates the first index's error (`?`,
 * search.rs:215), so one failing shard fails the whole search -- on EVERY rank, and without leaving
 * the others inside the collective.  A rank whose shard search cannot be enqueued or fails (wrong
 * dimension, no lane, a device error, a query that ends in NodeNotFound ...) still takes part in the
 * batch's all-gather with a record whose counts are ISL_SHARD_POISON_COUNT (the whole batch, or the
 * failed queries); the merge raises flag bit 2 on every rank and isl_sharded_result returns
 * ISL_ERR_SEARCH for that batch everywhere (the failing rank reports its own error).  Waits on an
 * exchange are bounded (ISL_SHARD_TIMEOUT_MS, default 60000): a peer that never arrives is
 * ISL_ERR_DEVICE naming the batch, not a hang. */
#define ISL_SHARD_UNIQUE_ID_BYTES 128
typedef struct isl_shard_group isl_shard_group;
typedef int32_t (*isl_shard_allgather_fn)(void* user, const void* send, void* recv, uint64_t bytes);
isl_status isl_shard_unique_id(uint8_t id[ISL_SHARD_UNIQUE_ID_BYTES]);
isl_status isl_shard_group_create(int32_t device, int32_t world, int32_t rank,
                                  const uint8_t id[ISL_SHARD_UNIQUE_ID_BYTES], isl_shard_group** out);
isl_status isl_shard_group_create_host(int32_t device, int32_t world, int32_t rank,
                                       isl_shard_allgather_fn allgather, void* user, isl_shard_group** out);
/* world / rank as created; *comm_ranks = what the communicator itself reports (ncclCommCount; the
 * host transport reports `world`); *is_rccl = 1 for the RCCL transport. */
isl_status isl_shard_group_info(const isl_shard_group* grp, int32_t* world, int32_t* rank, int32_t* comm_ranks,
                                int32_t* is_rccl);
/* (a group must outlive the searchers created over it) */
void isl_shard_group_free(isl_shard_group* grp);

/* The searcher of one rank: `shard` is this rank's LeannIndex over its id range (resident, provider
 * attached; borrowed, must outlive the searcher).  id_base[r] = first global id of rank r; NULL =
 * even ranges of n_total, rank r owns [r*n_total/R, (r+1)*n_total/R).  Up to `depth` (1..32)
 * batches in flight. */
typedef struct isl_sharded_searcher isl_sharded_searcher;
isl_status isl_sharded_searcher_new(const isl_index* shard, isl_shard_group* grp, uint64_t n_total,
                                    const uint64_t* id_base, int32_t depth, isl_sharded_searcher** out);
void isl_sharded_searcher_free(isl_sharded_searcher* s);
/* Buffers for `depth` batches of up to max_nq queries / max_k results, and isl_index_prepare on the
 * shard: nothing allocates on the submit path afterwards.  Collective over the ranks whenever the
 * searcher has a group (the RCCL communicator's first all-gather, which sets up its channels, is made
 * here): the 16 bytes exchanged carry every rank's local outcome, so a rank whose set-up failed still
 * enters the collective and ALL ranks return an error (the failing one its own, the others
 * ISL_ERR_SEARCH). */
isl_status isl_sharded_prepare(isl_sharded_searcher* s, uint64_t max_nq, uint64_t max_k, uint64_t max_ef);
/* Enqueues one batch (queries on the device, ordered after the work already on `stream`): shard
 * search -> all-gather of the records -> merge.  Every rank must submit the same batches (nq, k) in
 * the same order.  Returns a handle; nothing is waited for (RCCL transport).  Any free slot is taken
 * (the one released longest ago).  When this rank's search cannot be enqueued the exchange is made
 * all the same, with a poisoned record, the call returns the search's error and *handle stays 0 (the
 * slot is reclaimed behind the exchange); the other ranks learn of it from isl_sharded_result. */
isl_status isl_sharded_submit(isl_sharded_searcher* s, const float* d_queries, uint64_t nq, uint64_t d,
                              uint64_t k, uint64_t ef, void* stream, uint64_t* handle);
/* Completes a submitted batch: per-query failures of this rank's shard surface here (the first
 * failing query's CoreError), a failure of any other rank's shard as ISL_ERR_SEARCH, a NaN score in
 * this batch's merge as ISL_ERR_SEARCH (the reference panics, search.rs:231; flags are per batch);
 * the merged answers are on the device -- global ids u64[nq][k], distances f32[nq][k], source rank
 * u32[nq][k], counts u32[nq] -- and stay valid until `depth` further batches have been submitted
 * (slots are reused least-recently-released first).  `stats` (may be NULL) = this rank's search
 * counters.  The wait for the exchange is bounded (ISL_SHARD_TIMEOUT_MS -> ISL_ERR_DEVICE). */
isl_status isl_sharded_result(isl_sharded_searcher* s, uint64_t handle, const uint64_t** d_ids,
                              const float** d_dist, const uint32_t** d_src, const uint32_t** d_count,
                              isl_search_stats* stats);
/* MultiIndexSearcher::search over the shards with host buffers in and out (submit + result +
 * copies); out_src may be NULL.  A NaN score in the merge is ISL_ERR_SEARCH (the reference panics,
 * search.rs:231). */
isl_status isl_sharded_search_batch(isl_sharded_searcher* s, const float* queries, uint64_t nq, uint64_t d,
                                    uint64_t k, uint64_t ef, uint64_t* out_ids, float* out_dist,
                                    uint32_t* out_src, uint32_t* out_count);
/* Merge flags of all completed batches so far, OR-ed (bit 0: NaN score met, bit 1: a list was not
 * ascending, bit 2: a rank failed a batch); synchronises the exchange stream. */
isl_status isl_sharded_flags(isl_sharded_searcher* s, uint32_t* flags);

/* Product-level merge, src/indexer/service.rs:775-801 (IndexerService::search_with_embeddings):
 * per list the (id, distance) results of one index (searched with ef = max(top_k, 100), :781);
 * results whose id has no file entry are dropped (`files_len[l]` = stored.files.len(), host
 * array, NULL = keep all, :788), score = 1.0 - distance (:791), stable sort by score descending
 * (:800), truncate to top_k.  Layouts as in isl_merge_topk. */
isl_status isl_merge_service(uint64_t nlists, uint64_t nq, uint64_t k, const uint64_t* ids,
                             const float* distances, const uint32_t* counts,
                             const uint64_t* files_len, uint64_t top_k, uint64_t* out_ids,
                             float* out_scores, uint32_t* out_src, uint32_t* out_count,
                             int32_t mem, int32_t device, void* stream);

/* ---- pq.rs ---- */
typedef struct isl_pq isl_pq;
/* ProductQuantizer with trained codebooks: m x K x dsub floats (pq.rs:116-129). */
isl_status isl_pq_new(uint64_t dimension, uint64_t m, uint64_t K, const float* codebooks,
                      int32_t metric, int32_t device, isl_pq** out);
void isl_pq_free(isl_pq* pq);
/* build_distance_tables, pq.rs:307-338, for nq queries: tables [nq][m][K]. */
isl_status isl_pq_build_distance_tables(const isl_pq* pq, const float* queries, uint64_t nq,
                                        uint64_t d, float* tables, int32_t mem, void* stream);
/* table_distance, pq.rs:341-348: codes [n][m] u16 against ONE query's tables [m][K]. */
isl_status isl_pq_table_distance(const isl_pq* pq, const float* tables, const uint16_t* codes,
                                 uint64_t n, float* out, int32_t mem, void* stream);
/* asymmetric_distance, pq.rs:275-304: one query against n code rows. */
isl_status isl_pq_asymmetric_distance(const isl_pq* pq, const float* query, uint64_t d,
                                      const uint16_t* codes, uint64_t n, float* out, int32_t mem,
                                      void* stream);
/* encode, pq.rs:221-244: n vectors -> [n][m] u16 codes. */
isl_status isl_pq_encode(const isl_pq* pq, const float* vectors, uint64_t n, uint64_t d,
                         uint16_t* codes, int32_t mem, void* stream);

/* ---- embedding/candle_provider.rs:353-507: the recompute encoder (CandleEmbedder) ----
 * The model is candle-transformers 0.9.1 `BertModel` (third party, not in the reference tree;
 * call sites candle_provider.rs:284, :429-432); its published algorithm runs here in float32,
 * the linear layers on the matrix cores.  isl_bert_config mirrors the fields of the
 * checkpoint's config.json that the forward pass uses. */
typedef struct isl_bert_config {
  uint32_t vocab_size;
  uint32_t hidden;        /* hidden_size */
  uint32_t layers;        /* num_hidden_layers */
  uint32_t heads;         /* num_attention_heads; hidden / heads in {16, 32, 64} */
  uint32_t intermediate;  /* intermediate_size */
  uint32_t max_position;  /* max_position_embeddings */
  uint32_t type_vocab;    /* type_vocab_size */
  float layer_norm_eps;
  uint32_t gelu_tanh;     /* 0: hidden_act "gelu" (erf), 1: "gelu_new"/approximate (tanh) */
} isl_bert_config;
typedef struct isl_encoder isl_encoder;
isl_status isl_encoder_new(const isl_bert_config* cfg, int32_t device, isl_encoder** out);
void isl_encoder_free(isl_encoder* enc);
/* One tensor of the checkpoint by its HuggingFace name ("embeddings.word_embeddings.weight",
 * "encoder.layer.0.attention.self.query.weight", ...; an optional "bert." prefix is ignored), the
 * names candle's VarBuilder resolves (candle_provider.rs:267-284).  A wrong element count is
 * DimensionMismatch{expected, actual}. */
isl_status isl_encoder_set_weight(isl_encoder* enc, const char* name, const float* data,
                                  uint64_t count, int32_t mem);
/* Optional precision of the Linear layers: ISL_DTYPE_F32 (default) is the reference's float32
 * model; ISL_DTYPE_BF16 rounds weights and GEMM inputs to bf16 (float32 accumulation on the bf16
 * matrix cores) -- several times faster, embeddings differ from the float32 ones by about 1e-2
 * relative.  Call after the weights are set (changing a weight afterwards needs a new call). */
isl_status isl_encoder_set_precision(isl_encoder* enc, int32_t dtype);
/* BertModel::forward(input_ids, token_type_ids, Some(attention_mask)), candle_provider.rs:429-432:
 * ids [B, L] (already padded per :385-402), token_type_ids NULL = zeros, attention_mask [B, L]
 * of 0.0 / 1.0, NULL = ones -> last hidden state [B, L, hidden]. */
isl_status isl_encoder_forward(isl_encoder* enc, const int64_t* input_ids,
                               const int64_t* token_type_ids, const float* attention_mask,
                               uint64_t B, uint64_t L, float* out_hidden, int32_t mem, void* stream);
/* embed_texts_raw after tokenisation (candle_provider.rs:404-507): forward, masked mean pooling,
 * L2 normalisation when `normalize` -> [B, hidden]. */
isl_status isl_encoder_embed(isl_encoder* enc, const int64_t* input_ids, const int64_t* token_type_ids,
                             const float* attention_mask, uint64_t B, uint64_t L, int32_t normalize,
                             float* out, int32_t mem, void* stream);

/* Recompute provider: EmbeddingProvider (leann.rs:82-99) backed by the encoder, the mode the
 * paper and `LeannConfig::is_recompute` (leann.rs:366-371) describe -- no stored embeddings, the
 * vectors of the nodes a search visits are computed on the fly from their text.  `tokens` holds
 * node i's tokenised text in row i (n rows of L slots, `lengths[i]` of them used, NULL = all L;
 * tokenisation itself is third-party code outside this library).  After the call searches on
 * `idx` re-encode what they visit: the rows a batch misses are encoded once each, in batches
 * across all its queries.  keep_rows = 0 forgets every row when a call returns (pure recompute),
 * 1 keeps them as an embedding cache.  The encoder is borrowed and must outlive the index;
 * its hidden size becomes the index dimension; `normalize` as in isl_encoder_embed.
 * Results equal those of the in-memory provider holding the same embeddings.  Every search kernel
 * parks a query that meets an absent row and resumes it there once the row is encoded, so the row
 * cache may be far smaller than a traversal (floor: 256 rows). */
isl_status isl_set_recompute_provider(isl_index* idx, isl_encoder* enc, const uint16_t* tokens,
                                      const uint16_t* lengths, uint64_t n, uint64_t L,
                                      int32_t normalize, int32_t keep_rows, int32_t mem);
/* The recompute provider does not store embeddings (leann.rs:366-371); what it keeps on the device
 * is the token table and a bounded row cache: a slab of `rows` embedding rows (default 2^20, or
 * every node of a smaller index; at least 256) plus 4 bytes of slot map per node.  Slots are handed
 * out round-robin, the oldest rows make room.  isl_index_recompute_cache_bytes = what that costs. */
isl_status isl_index_set_recompute_cache_rows(isl_index* idx, uint64_t rows);
uint64_t isl_index_recompute_cache_bytes(const isl_index* idx);

/* ---- embedding/candle_provider.rs:434-488: masked mean-pool + optional L2 normalise ----
 * hidden [B][L][H] f32, mask [B][L] (0/1 as f32), out [B][H].  The BERT forward that
 * produces `hidden` is third-party code (candle-transformers) and out of this round. */
isl_status isl_mean_pool_normalize(const float* hidden, const float* mask, uint64_t B, uint64_t L,
                                   uint64_t H, int32_t normalize, float* out, int32_t mem,
                                   int32_t device, void* stream);

/* ---- HnswGraph, src/core/hnsw.rs:149-515 ---- */
typedef struct isl_hnsw isl_hnsw;
/* Builds a device-resident HnswGraph from its parts: `levels[i]` = node i's top layer;
 * layer L adjacency in CSR form over ALL nodes (rows of nodes below layer L are empty):
 * layer_offsets[L] has num_nodes + 1 entries, layer_neighbors[L] the ids.  vectors: num_nodes
 * rows of d floats (HnswNode::vector).  m/m0/ef_construction are carried for completeness. */
isl_status isl_hnsw_from_layers(uint64_t m, uint64_t m0, uint64_t ef_construction, int32_t metric,
                                uint64_t num_nodes, uint64_t d, uint64_t num_layers,
                                const uint64_t* const* layer_offsets,
                                const uint64_t* const* layer_neighbors, const uint64_t* levels,
                                int32_t has_entry, uint64_t entry_point, uint64_t max_level,
                                const float* vectors, int32_t device, isl_hnsw** out);
/* isl_hnsw_from_layers over rows of either stored type: a finished graph handed over with its rows.  dtype
 * ISL_DTYPE_F32: rows = num_nodes x d float, the call IS isl_hnsw_from_layers.  dtype ISL_DTYPE_BF16: rows =
 * num_nodes x d bf16 bit patterns (u16) in host memory; the graph's vectors are their exact float32 images and the
 * rows stay bf16 on the device (one table of 2-byte elements, isl_hnsw_row_storage).  Checked first, in this order:
 * NULL out -> ISL_ERR_INVALID_ARGUMENT; an unknown dtype -> ISL_ERR_INVALID_ARGUMENT, ISL_DTYPE_FP8_E4M3 ->
 * ISL_ERR_UNSUPPORTED; then everything isl_hnsw_from_layers checks. */
isl_status isl_hnsw_from_layers_rows(uint64_t m, uint64_t m0, uint64_t ef_construction, int32_t metric,
                                     uint64_t num_nodes, uint64_t d, uint64_t num_layers,
                                     const uint64_t* const* layer_offsets,
                                     const uint64_t* const* layer_neighbors, const uint64_t* levels,
                                     int32_t has_entry, uint64_t entry_point, uint64_t max_level,
                                     const void* rows, int32_t dtype, int32_t device, isl_hnsw** out);
/* HnswGraph::from_bytes, hnsw.rs:511-514: reads the bincode image of a HnswGraph (1.x default
 * layout; HashMap entries in any order, node ids 0..n-1) and makes it resident on `device`.
 * Truncated or inconsistent input -> ISL_ERR_DESERIALIZATION.  (isl_hnsw_to_bytes writes ascending ids;
 * HashMap order makes the reference's own bytes non-deterministic) */
isl_status isl_hnsw_from_bytes(const uint8_t* bytes, size_t len, int32_t device, isl_hnsw** out);
void isl_hnsw_free(isl_hnsw* h);
uint64_t isl_hnsw_len(const isl_hnsw* h);
/* HnswGraph::search (hnsw.rs:458-504) for a batch of queries: greedy descent through layers
 * max_level..1, then search_layer on layer 0 with ef = max(ef, k); heap order on distance only
 * (hnsw.rs:136-141), reproduced with an exact BinaryHeap emulation.  A graph over bf16 rows is searched with
 * float32 queries all the same: ids and distances are those of the graph over the rows' float32 images. */
isl_status isl_hnsw_search_batch(const isl_hnsw* h, const float* queries, uint64_t nq, uint64_t d,
                                 uint64_t k, uint64_t ef, uint64_t* out_ids, float* out_dist,
                                 uint32_t* out_count);
/* Work counters of the most recent search on this graph (see isl_search_last_stats);
 * exact_path = queries in which two equal distances met and the heap-exact kernel decided. */
isl_status isl_hnsw_last_stats(const isl_hnsw* h, isl_search_stats* out);
/* The reachability report of layer `layer` (see "graph reachability" above). */
isl_status isl_hnsw_reachability(const isl_hnsw* h, uint64_t layer, const uint64_t* sources, uint64_t n_sources,
                                 uint32_t* out_depth, uint32_t* out_in_degree, int32_t mem, isl_reach_report* report);

/* ---- HnswGraph construction on the device: HnswGraph::insert, hnsw.rs:214-329 ---- */
typedef struct isl_hnsw_config { /* HnswConfig, hnsw.rs:15-28 */
  uint64_t m, m0, ef_construction;
  double ml;
  uint32_t metric;
  uint64_t max_layers;
} isl_hnsw_config;
void isl_hnsw_config_default(isl_hnsw_config* cfg); /* 16, 32, 200, 1/ln 16, Cosine, 16: hnsw.rs:37-48 */
/* random_level (hnsw.rs:206-211) with a seeded generator in place of thread_rng:
 * out[i] = min(floor(-ln(r_i) * ml), max_layers - 1), r_i = ((x_i >> 11) + 0.5) * 2^-53 in (0, 1),
 * x_i = splitmix64 output number i of state `seed` (z = seed + (i + 1) * 0x9E3779B97F4A7C15;
 * z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; x_i = z ^ z >> 31).
 * Host only.  max_layers == 0 or ml not finite -> ISL_ERR_INVALID_ARGUMENT. */
isl_status isl_hnsw_random_levels(uint64_t seed, uint64_t n, double ml, uint64_t max_layers, uint64_t* out);
/* Inserts rows 0 .. n-1 in id order into an empty HnswGraph on `device`; `levels[i]` stands for
 * random_level() (NULL: isl_hnsw_random_levels(level_seed, n, cfg->ml, cfg->max_layers)).  cfg NULL =
 * the default config; opts NULL = isl_build_options_default.
 * ISL_SELECT_REFERENCE, batch 1: HnswGraph::insert as written -- greedy descent over layers max_level ..
 * level + 1, per layer level .. 0 a search_layer with ef_construction from `current`, the first M_L results
 * (M_L = m0 on layer 0, m above) as the node's list, the new id appended to every selected neighbour that
 * has the layer, and a list past M_L re-sorted by prune_connections -- which cannot see the node being
 * inserted (hnsw.rs:417-429 reads a map the node enters at :327) and so drops it again.  Layer lists,
 * levels, entry point and max level equal the reference's; so does the consequence: once the graph holds
 * more than m0 nodes no later node receives an inbound edge.
 * ISL_SELECT_DIVERSE (extension, select() as defined above for isl_index_build_ex): the same loop with the
 * node's list on layer L = select(i, search result with the search's distances, M_L), and a list that
 * reaches M_L + 1 ids after the append replaced by select(s, the list stable-sorted by d(s, .), M_L) -- the
 * new node takes part.  The rule is not recorded in the graph.
 * opts->batch > 1 (both rules): a throughput mode with the same rules and no parity claim.  A step takes
 * min(batch, n - id0, max(1, id0 / 8)) nodes, cut so that a node above the current max level is alone in
 * its step (entry point and max level are the sequential ones for any batch); all of a step's nodes
 * descend on the graph as of the step's start, then per layer from the step's highest down to 0 they
 * search, select and link (per-list locks; the order in which back links land is unspecified).
 * Checked in this order before any device call: opts as in isl_index_build_ex; HnswConfig::validate
 * (ISL_ERR_INVALID_CONFIG); n == 0 -> an empty graph; d == 0 -> ISL_ERR_EMPTY_COLLECTION; levels[i] >=
 * max_layers -> ISL_ERR_INVALID_ARGUMENT; m0 > 128, ef_construction > 512 or n beyond the device id range
 * -> ISL_ERR_UNSUPPORTED.  `vectors`: n rows of d f32 on the host or on `device` (mem = ISL_MEM_*). */
isl_status isl_hnsw_build(const isl_hnsw_config* cfg, const isl_build_options* opts, const float* vectors,
                          uint64_t n, uint64_t d, const uint64_t* levels, uint64_t level_seed, int32_t mem,
                          int32_t device, isl_hnsw** out);
/* isl_hnsw_build over rows of either stored type.  dtype ISL_DTYPE_F32: rows = n x d float, the call IS
 * isl_hnsw_build.  dtype ISL_DTYPE_BF16: rows = n x d bf16 bit patterns (u16), on the host or on `device`; the
 * graph's vectors are their exact float32 images, so the graph is -- list for list on every layer, under both rules
 * and any batch -- the one isl_hnsw_build makes of the widened rows, and every search answers as that graph does.
 * The rows stay bf16: one table of 2-byte elements (isl_hnsw_row_storage) and no float32 copy of them on the device
 * once the call has returned.  The descent, the selections and the re-selections measure the bf16 rows with the
 * library's exact-order float32 chain over the images.
 * Checked in this order before any device call: NULL out, or NULL rows with n > 0 -> ISL_ERR_INVALID_ARGUMENT; opts
 * as in isl_index_build_ex; an unknown dtype -> ISL_ERR_INVALID_ARGUMENT, ISL_DTYPE_FP8_E4M3 -> ISL_ERR_UNSUPPORTED
 * (the builders do not take fp8 rows for a LeannIndex either); then as isl_hnsw_build: HnswConfig::validate; n == 0
 * -> the empty graph (it stores nothing: isl_hnsw_row_storage reports ISL_DTYPE_F32 and 0 bytes); d == 0 ->
 * ISL_ERR_EMPTY_COLLECTION; levels[i] >= max_layers -> ISL_ERR_INVALID_ARGUMENT; the shape limits ->
 * ISL_ERR_UNSUPPORTED.  *out is written only on ISL_OK. */
isl_status isl_hnsw_build_rows(const isl_hnsw_config* cfg, const isl_build_options* opts, const void* rows,
                               int32_t dtype, uint64_t n, uint64_t d, const uint64_t* levels, uint64_t level_seed,
                               int32_t mem, int32_t device, isl_hnsw** out);
/* HnswGraph::insert (hnsw.rs:214-251) for n_new more rows: nodes len .. len + n_new - 1 enter `h` in id order,
 * in place, under the config the handle carries (m, m0, ef_construction, metric, ml, max_layers).  `h` may
 * have been built here, read by isl_hnsw_from_bytes or handed over with isl_hnsw_from_layers.  *first_id
 * (may be NULL) = the old len, written only where the call returns ISL_OK.  `opts` is the rule and batch of THIS call, as for isl_hnsw_build (NULL = the
 * defaults; the rule is still not recorded in the graph).  `levels[i]` stands for random_level() of node
 * len + i; NULL: positions len .. len + n_new - 1 of the `level_seed` stream of isl_hnsw_random_levels (the
 * stream is addressed by position), so isl_hnsw_build(v, seed) equals isl_hnsw_build(v[:n0], seed) followed
 * by isl_hnsw_insert(v[n0:], seed).
 * opts->batch == 1, either rule: the graph after the call is the graph isl_hnsw_build makes of all
 * len + n_new rows with the concatenated levels -- the same lists on every layer, levels, entry point, max
 * level and isl_hnsw_to_bytes image.  batch > 1: the throughput mode of isl_hnsw_build (a step takes
 * min(batch, n - id0, max(1, id0 / 8)) nodes, id0 starting at the old len; a node above the current max
 * level is alone in its step), same rules, no parity claim.
 * An empty handle (len 0, no entry point, no dimension) takes the rows as isl_hnsw_build would with the
 * handle's config, on the device it was made for; d becomes its dimension.
 * Strong guarantee: on any failure `h` is unchanged (lists, rows, bytes, search answers).  The grown graph
 * is built beside the old one and swapped into the handle at the end.  Peak device memory is therefore the
 * old graph, plus one row table of len + n_new rows, plus the per-layer construction tables ([n][m0 + 1]
 * ids on layer 0, [n][m + 1] per layer above): about twice the rows for the duration of the call.
 * The call is the `&mut self` of the reference: it must not run beside searches on the same handle; if a
 * lane of the handle's index is busy it returns ISL_ERR_SEARCH, as the provider setters do.  Lanes and the
 * padded adjacency of the grown graph are set up again at its first search.
 * Checked in this order before any device call: NULL h, or NULL vectors with n_new > 0 ->
 * ISL_ERR_INVALID_ARGUMENT; opts as in isl_hnsw_build; n_new == 0 -> ISL_OK, nothing changed; a non-empty
 * graph and d != its dimension -> ISL_ERR_DIMENSION_MISMATCH (payload expected, actual: hnsw.rs:216-222);
 * d == 0 -> ISL_ERR_EMPTY_COLLECTION; levels[i] >= max_layers -> ISL_ERR_INVALID_ARGUMENT; m0 > 128,
 * ef_construction > 512, len + n_new beyond the device id range or more than 64 layers ->
 * ISL_ERR_UNSUPPORTED; and ISL_ERR_UNSUPPORTED, with a message that says which, for a handle whose rows are
 * not resident f32 or bf16 rows, a handle whose rows are bf16 (isl_hnsw_insert_rows takes those), a handle
 * with a list longer than its layer's M_L (isl_hnsw_from_bytes accepts such
 * images; the tables hold M_L + 1 ids -- lists above layer 0 are measured while they are imported), a
 * handle whose layer-0 device copy is not the list verbatim because ids repeated inside a list were removed
 * at upload, and a handle whose levels do not match its layers (the entry point's level is not max_level,
 * or a level exceeds it: isl_hnsw_from_layers with levels == NULL and layers above 0). */
isl_status isl_hnsw_insert(isl_hnsw* h, const isl_build_options* opts, const float* vectors, uint64_t n_new,
                           uint64_t d, const uint64_t* levels, uint64_t level_seed, int32_t mem,
                           uint64_t* first_id);
/* isl_hnsw_insert over rows of either stored type; isl_hnsw_insert IS this call with ISL_DTYPE_F32.  rows = n_new x d
 * elements of `dtype` (float, or bf16 bit patterns as u16), on the host or on the graph's device.  On a non-empty
 * graph `dtype` must be the stored type of its rows (isl_hnsw_row_storage): the grown graph keeps one table of that
 * type, the old rows and norms copied beside the new ones on the device.  An empty handle takes the type of the rows
 * it is given.  The strong guarantee, the `&mut self` rule and the batch == 1 identity are isl_hnsw_insert's: over
 * bf16 rows the graph after the call is the graph isl_hnsw_build_rows makes of all len + n_new rows.
 * Checked in this order before any device call: NULL h, or NULL rows with n_new > 0 -> ISL_ERR_INVALID_ARGUMENT;
 * opts as in isl_hnsw_build; an unknown dtype -> ISL_ERR_INVALID_ARGUMENT, ISL_DTYPE_FP8_E4M3 ->
 * ISL_ERR_UNSUPPORTED; then as isl_hnsw_insert from n_new == 0 on, with one refusal more behind the residency of
 * the rows: a non-empty graph that stores another type than `dtype` -> ISL_ERR_UNSUPPORTED (isl_index_insert's
 * rule).  *first_id is written only on ISL_OK. */
isl_status isl_hnsw_insert_rows(isl_hnsw* h, const isl_build_options* opts, const void* rows, int32_t dtype,
                                uint64_t n_new, uint64_t d, const uint64_t* levels, uint64_t level_seed, int32_t mem,
                                uint64_t* first_id);
/* Rows out of a built HnswGraph, in place (extension: the reference has no removal).  `h` may have been built
 * here, grown by isl_hnsw_insert, read by isl_hnsw_from_bytes or handed over with isl_hnsw_from_layers.  ids =
 * n_ids node ids in host memory, repeated ids counting once: the set D.  opts = the selection rule of this call
 * (select_rule, alpha, keep_pruned; NULL: the defaults; batch is not used); the rule is not recorded in the graph,
 * as with isl_hnsw_insert.  out_remap [old len] (may be NULL) receives the new id of every old node or ISL_REMOVED,
 * *out_len (may be NULL) the new len; both are written only on ISL_OK.
 * Definition, over a graph with layers 0 .. max_level, L_L[p] = neighbors_at(L) of node p in stored order,
 * M_L = m0 on layer 0 and m above, and resident f32 or bf16 rows (the vectors of bf16 rows are their exact float32
 * images; the shrunk graph keeps the stored type, fp8 rows stay refused):
 * 1. Repair, per layer.  Every layer is repaired independently and every list comes from the OLD lists of that
 *    layer only.  For every layer L and every survivor p with level[p] >= L: if no id of L_L[p] is in D,
 *    L'_L[p] = L_L[p].  Otherwise the candidate list C_L(p), built as isl_index_remove builds C(p) but on layer L:
 *    walk L_L[p] in stored order; a survivor x emits x, also where x does not have layer L (HnswGraph::insert
 *    leaves such lists behind a node that rises above the top layer, and they are kept as they are); a removed x
 *    emits every y of L_L[x], in stored order, with y not in D and y != p, and nothing where it does not have
 *    layer L; first occurrences only; the walk stops after ISL_REMOVE_MAX_CANDIDATES distinct ids.  If
 *    |C_L(p)| <= M_L, L'_L[p] = C_L(p).  If |C_L(p)| > M_L: d(p, c) = Distance::calculate(vec[p], vec[c]) through
 *    the library's exact-order chain, a stable ascending sort (NaN last, -0 == +0), then ISL_SELECT_REFERENCE
 *    keeps the first M_L and ISL_SELECT_DIVERSE keeps select(p, sorted C_L(p), M_L).  A list whose candidates are
 *    all gone ends EMPTY: nothing is invented.
 * 2. Compaction, order kept.  New id = old id minus the removed ids below it; the levels of the survivors are
 *    kept; their rows and norms are copied bit for bit on the device.  Entry point: one that survives is kept
 *    (remapped) and max_level stays; otherwise the lowest new id among the survivors of the highest surviving
 *    level takes over and max_level becomes that level; the layers above the new max_level cease to exist.
 *    isl_hnsw_to_bytes afterwards writes next_id = the new len.  Removing every node leaves what isl_hnsw_build
 *    gives for n == 0 under the handle's config (m, m0, ef_construction, metric, ml, max_layers, device): no entry
 *    point, no dimension; a later isl_hnsw_insert starts the graph again.
 * After ISL_OK the handle satisfies every precondition of isl_hnsw_insert (levels match layers, lists <= M_L,
 * layer 0 verbatim) and serves isl_hnsw_search_batch; lanes and the padded adjacency are set up again at the
 * first search, as after isl_hnsw_insert.
 * Strong guarantee: the shrunk graph is built beside the old one and swapped into the handle at the end; on any
 * failure `h` is unchanged (bytes, rows, search answers).  Peak device memory: the old graph whole, plus one table
 * per old layer over the OLD nodes ([len][m0 + 1] ids on layer 0, [len][m + 1] per layer above, and len degrees
 * each), the touched list (8 bytes per surviving list), the shrunk layer 0 twice and its padded adjacency, the
 * shrunk upper layers (len' + 1 offsets each) and the survivors' rows.
 * The call is the reference's &mut self: not beside searches on the same handle.  Checked in this order before any
 * device call: NULL h, or NULL ids with n_ids > 0 -> ISL_ERR_INVALID_ARGUMENT; opts as in isl_hnsw_build;
 * n_ids == 0 -> ISL_OK, nothing changed, out_remap the identity; an id >= len -> ISL_ERR_NODE_NOT_FOUND (node); a
 * non-empty graph whose rows are not resident f32 or bf16 rows -> ISL_ERR_UNSUPPORTED; nodes but no entry point, or levels
 * that do not match the layers (as isl_hnsw_insert refuses them) -> ISL_ERR_UNSUPPORTED; m0 > 128 or more than 64
 * layers -> ISL_ERR_UNSUPPORTED; a busy lane -> ISL_ERR_SEARCH.  Refused once the import kernel has looked, each
 * with ISL_ERR_UNSUPPORTED and a message that says which: a list longer than its layer's M_L; a layer-0 device
 * copy that is not the lists verbatim; an id or offset outside the graph.
 * isl_index_remove on the core index of an HnswGraph stays ISL_ERR_UNSUPPORTED. */
isl_status isl_hnsw_remove(isl_hnsw* h, const isl_build_options* opts, const uint64_t* ids, uint64_t n_ids,
                           uint64_t* out_remap /* [old len], may be NULL */, uint64_t* out_len /* may be NULL */);
/* Read-back into host buffers, for every isl_hnsw handle (built, from_layers, from_bytes). */
isl_status isl_hnsw_info(const isl_hnsw* h, int32_t* has_entry, uint64_t* entry, uint64_t* max_level,
                         uint64_t* dim);
isl_status isl_hnsw_levels(const isl_hnsw* h, uint64_t* out /* [len] */);
/* neighbors_at(layer) of `node`: *count = the list's length (also when cap is smaller: then the first
 * cap ids are written).  *has_layer (may be NULL) = 1 if the node has the layer (Some), 0 above its level
 * (None; *count = 0).  node >= len -> ISL_ERR_NODE_NOT_FOUND. */
isl_status isl_hnsw_get_neighbors(const isl_hnsw* h, uint64_t node, uint64_t layer, uint64_t* out,
                                  uint64_t cap, uint64_t* count, int32_t* has_layer);
/* HnswNode::vector as float32.  Over bf16 rows: the exact float32 images of the stored bits. */
isl_status isl_hnsw_get_vector(const isl_hnsw* h, uint64_t node, float* out /* [dim] */);
/* What the graph's rows cost on the device (isl_index_row_storage of the facade): their stored type (ISL_DTYPE_F32
 * or ISL_DTYPE_BF16) and the bytes of the row table.  Either out pointer may be NULL.  An empty graph stores
 * nothing: ISL_DTYPE_F32 and 0 bytes.  NULL h -> ISL_ERR_INVALID_ARGUMENT. */
isl_status isl_hnsw_row_storage(const isl_hnsw* h, int32_t* dtype, uint64_t* block_bytes);
/* HnswGraph::to_bytes, hnsw.rs:507-509: the bincode image isl_hnsw_from_bytes reads, nodes in ascending
 * id (the reference's HashMap order is arbitrary), next_id = len; ml / max_layers as built or parsed
 * (isl_hnsw_from_layers: the default config's).  Free with isl_free_bytes.
 * The format has one vector field, Vec<f32>: over bf16 rows the widened values are written, so the image of a bf16
 * graph is byte for byte the image of the float32 graph over the widened rows, and isl_hnsw_from_bytes of it gives a
 * graph that stores float32 rows. */
isl_status isl_hnsw_to_bytes(const isl_hnsw* h, uint8_t** out, size_t* len);

/* isl_distance_matrix for bf16 queries and rows (bit patterns; BASELINE config 5: d = 4096 bf16): the
 * same batch_calculate (distance.rs:32-34) over the exact float32 images of the stored values, on
 * the bf16 matrix cores (v_mfma_f32_32x32x16_bf16, float32 accumulation).  out [nq][n] f32.
 * d must be a multiple of 64; Manhattan -> Unsupported.  Agreement with the sequential sums:
 * float32 rounding of the accumulation order (<= 1e-5 on normalised rows), not bit for bit. */
isl_status isl_distance_matrix_bf16(int32_t metric, const uint16_t* queries, uint64_t nq, const uint16_t* rows,
                                    uint64_t n, uint64_t d, float* out, int32_t mem, int32_t device,
                                    void* stream);
/* Sum of squares of every row of a bf16 matrix (of the exact float32 images), as the cosine / Euclidean
 * epilogues of isl_distance_matrix_bf16 take it; out [n] f32. */
isl_status isl_row_sumsq_bf16(const uint16_t* rows, uint64_t n, uint64_t d, float* out, int32_t mem, int32_t device,
                              void* stream);
/* isl_distance_matrix_bf16 for callers that keep the rows (or the queries) resident across calls:
 * q_sumsq [nq] / row_sumsq [n] = isl_row_sumsq_bf16 of them, in the matrices' memory space, computed
 * once instead of per call (NULL = computed here).  Same outputs, bit for bit. */
isl_status isl_distance_matrix_bf16_norms(int32_t metric, const uint16_t* queries, uint64_t nq, const uint16_t* rows,
                                          uint64_t n, uint64_t d, const float* q_sumsq, const float* row_sumsq,
                                          float* out, int32_t mem, int32_t device, void* stream);
/* The same GEMM, enqueued on `stream` and nothing else: device buffers only, q_sumsq / row_sumsq required
 * (except for ISL_METRIC_DOT), no allocation, no synchronisation -- the caller's next work on `stream`
 * finds the distances in `out`.  For callers that walk resident rows block by block (config 5: 153 blocks
 * of 65536 rows per query batch) and must not let the chip idle between two blocks.  Same outputs, bit
 * for bit.  Replaces Distance::batch_calculate (distance.rs:32-34) over a block of rows. */
isl_status isl_distance_matrix_bf16_enqueue(int32_t metric, const uint16_t* queries, uint64_t nq, const uint16_t* rows,
                                            uint64_t n, uint64_t d, const float* q_sumsq, const float* row_sumsq,
                                            float* out, int32_t device, void* stream);
/* isl_bruteforce_topk over bf16 rows and queries: blocks of isl_distance_matrix_bf16 + the same running
 * top-k (ties towards the smaller id), exact under the bf16 GEMM's distances.  Ground truth and exact
 * kNN lists at sizes where the float32 GEMM would take tens of minutes (10M x 10M x 768). */
isl_status isl_bruteforce_topk_bf16(int32_t metric, const uint16_t* queries, uint64_t nq, const uint16_t* rows,
                                    uint64_t n, uint64_t d, uint64_t k, uint64_t* out_ids, float* out_dist,
                                    uint32_t* out_count, int32_t mem, int32_t device, void* stream);

/* ---- EXTENSION: two-level search with a PQ filter ----
 * "Algorithm 2: Two-Level Search with Hybrid Distance", docs/leann-specification.md:223-275; the
 * reference promises it (leann.rs:54-56, :855-857: "a two-level search with PQ filtering should
 * be used") and ships no implementation, so there is no reference result to be identical to.
 * The rules the pseudo-code leaves open are fixed in oracle/islands_oracle.c
 * (orc_two_level_search), which the device path matches bit for bit: every new neighbour gets
 * ProductQuantizer::table_distance (pq.rs:341-348) on the tables of build_distance_tables
 * (pq.rs:307-338); after each expansion the not yet promoted members of the first
 * ceil(rerank_ratio * |AQ|) entries of the approximate queue get their exact distance from the
 * index's embedding provider (in-memory or recompute) and enter the result set.
 *
 * isl_index_set_pq_codes: codes [n][pq->m] u16 as ProductQuantizer::encode writes them
 * (pq.rs:221-244), copied to the device; `pq` is borrowed and must outlive the index.  A code
 * >= num_centroids -> ISL_ERR_PQ (the reference's tables[sq][code] would panic). */
isl_status isl_index_set_pq_codes(isl_index* idx, const isl_pq* pq, const uint16_t* codes, uint64_t n,
                                  int32_t mem);
/* Same outputs and error behaviour as isl_search_batch / isl_search_batch_device.
 * isl_search_last_stats afterwards: evals = exact distance evaluations, pushes = approximate
 * (table) evaluations.  ISL_ERR_SEARCH when ceil(rerank_ratio * |AQ|) outgrows the queue window a
 * wave keeps in LDS (up to 16384 entries) -- never a different answer. */
isl_status isl_search_two_level_batch(const isl_index* idx, const float* queries, uint64_t nq, uint64_t d,
                                      uint64_t k, uint64_t ef, float rerank_ratio, uint64_t* out_ids,
                                      float* out_dist, uint32_t* out_count);
isl_status isl_search_two_level_batch_device(const isl_index* idx, const float* d_queries, uint64_t nq,
                                             uint64_t d, uint64_t k, uint64_t ef, float rerank_ratio,
                                             uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count,
                                             void* stream);
/* Asynchronous form (see isl_search_batch_device_async): up to 32 calls in flight on the index's
 * lanes, completed with isl_search_wait[_stats](*token).  The call runs on a host thread of the
 * library's (a query whose queue window was too small is re-run with a larger one before the call
 * completes), so isl_search_stream_wait for such a token waits on the host. */
isl_status isl_search_two_level_batch_device_async(const isl_index* idx, const float* d_queries, uint64_t nq,
                                                   uint64_t d, uint64_t k, uint64_t ef, float rerank_ratio,
                                                   uint64_t* d_out_ids, float* d_out_dist, uint32_t* d_out_count,
                                                   void* stream, uint64_t* token);

#ifdef __cplusplus
}
#endif
#endif /* ISLANDS_AMD_H */
