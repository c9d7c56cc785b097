// Host-only arithmetic of the refine table and the rescoring kernel (search_refine.hip): the argument checks that
// precede every device call, the launch grid, the kernel's LDS and the scratch of a refined search.  Plain C++
// without a device header, in the manner of graph_reach_plan.hpp: tests/cpp/search_refine_plan_dump.cpp prints it
// with g++ alone (tests/test_refine_cpu.py compares with a Python restatement).
#pragma once

#include <algorithm>
#include <cstdint>

#include "../../include/islands_amd.h"

namespace isl_refine {

// ---- the kernel's shape
// One wave per query: the candidates go 64 at a time through direct_distances, which wants lane == threadIdx.x.
constexpr uint32_t kBlock = 64;
constexpr uint32_t kChunk = 64;         // candidates scored per pass of the wave
constexpr uint32_t kQueryPad = 32;      // the staged query is zero-padded to this many floats
constexpr uint32_t kKeyBytes = 8;       // (ordkey << 32 | position) per candidate
constexpr uint32_t kScoreBytes = 4;     // ... and its score as computed (the key forgets -0 and NaN payloads)
// The query waits in LDS as f32 beside keys and scores: 128 KiB + 6 KiB of the CU's 160.
constexpr uint64_t kMaxDim = 32768;

inline uint32_t padded_dim(uint64_t d) { return (uint32_t)((d + kQueryPad - 1) / kQueryPad * kQueryPad); }
// LDS of one workgroup: the padded query, then a key and a score per candidate slot of the call
inline uint64_t lds_bytes(uint64_t d, uint64_t pitch) {
  return (uint64_t)padded_dim(d) * 4 + pitch * (kKeyBytes + kScoreBytes);
}
// workgroups of a call: one per query
inline uint32_t grid(uint64_t nq) { return (uint32_t)nq; }
// passes of the wave over a row of c candidates
inline uint32_t passes(uint64_t c) { return (uint32_t)((c + kChunk - 1) / kChunk); }
// comparisons of the rank-by-counting pass per lane: every candidate the lane owns against all c keys
inline uint64_t rank_compares_per_lane(uint64_t c) { return (uint64_t)passes(c) * c; }

// ---- the scratch of a refined search: the inner search's answers
struct Scratch { uint64_t ids, dist, count; };  // elements: u64, f32, u32
inline Scratch scratch_elems(uint64_t nq, uint64_t candidates) { return Scratch{nq * candidates, nq * candidates, nq}; }
inline uint64_t scratch_bytes(uint64_t nq, uint64_t candidates) {
  const Scratch s = scratch_elems(nq, candidates);
  return s.ids * 8 + s.dist * 4 + s.count * 4;
}

// ---- argument checks, in the order the header states them.  Each returns the status alone; the caller words the message.
// What the handle looks like to the checks.
struct Handle {
  bool null_idx, is_hnsw, on_device, recompute, has_dimension;
  uint64_t len, dimension;
  uint64_t table_rows, table_d;  // the refine table (0 rows: none)
};

// Which check refused (the entry point words the message from it); kPass = none.
enum Why {
  kPass = 0, kNull, kUnknownEnum, kFp8, kHnsw, kNoDevice, kRowCount, kNoDim, kDimMismatch, kDimLimit,
  kNoTable, kZeroK, kKAboveCandidates, kCandidatesAboveEf, kCandidateLimit, kRecompute, kQueryLimit
};
struct Verdict { isl_status status; Why why; };

// isl_index_set_refine_rows up to the busy-lane check.  *drops = the call drops the table (n == 0).
inline Verdict check_set_rows(const Handle& h, bool rows_null, uint64_t n, uint64_t d, int32_t dtype, int32_t mem,
                              int32_t placement, bool* drops) {
  *drops = false;
  if (h.null_idx || (rows_null && n > 0)) return {ISL_ERR_INVALID_ARGUMENT, kNull};
  if (dtype != ISL_DTYPE_F32 && dtype != ISL_DTYPE_BF16 && dtype != ISL_DTYPE_FP8_E4M3) return {ISL_ERR_INVALID_ARGUMENT, kUnknownEnum};
  if (mem != ISL_MEM_HOST && mem != ISL_MEM_DEVICE) return {ISL_ERR_INVALID_ARGUMENT, kUnknownEnum};
  if (placement != ISL_REFINE_DEVICE && placement != ISL_REFINE_HOST) return {ISL_ERR_INVALID_ARGUMENT, kUnknownEnum};
  if (dtype == ISL_DTYPE_FP8_E4M3) return {ISL_ERR_UNSUPPORTED, kFp8};
  if (h.is_hnsw) return {ISL_ERR_UNSUPPORTED, kHnsw};
  if (!h.on_device) return {ISL_ERR_UNSUPPORTED, kNoDevice};
  if (n == 0) {
    *drops = true;
    return {ISL_OK, kPass};
  }
  if (n != h.len) return {ISL_ERR_INVALID_ARGUMENT, kRowCount};
  if (d == 0) return {ISL_ERR_EMPTY_COLLECTION, kNoDim};
  if (h.has_dimension && h.dimension != d) return {ISL_ERR_DIMENSION_MISMATCH, kDimMismatch};
  if (d > kMaxDim) return {ISL_ERR_UNSUPPORTED, kDimLimit};
  return {ISL_OK, kPass};
}

// isl_search_refined_batch[_device]; isl_rescore_device with pitch in the place of candidates and of ef
inline Verdict check_refined(const Handle& h, bool buffers_null, uint64_t nq, uint64_t d, uint64_t k,
                             uint64_t candidates, uint64_t ef) {
  if (h.null_idx || (buffers_null && nq > 0)) return {ISL_ERR_INVALID_ARGUMENT, kNull};
  if (h.table_rows == 0) return {ISL_ERR_INVALID_ARGUMENT, kNoTable};
  if (k == 0) return {ISL_ERR_INVALID_ARGUMENT, kZeroK};
  if (k > candidates) return {ISL_ERR_INVALID_ARGUMENT, kKAboveCandidates};
  if (candidates > ef) return {ISL_ERR_INVALID_ARGUMENT, kCandidatesAboveEf};
  if (candidates > ISL_REFINE_MAX_CANDIDATES) return {ISL_ERR_UNSUPPORTED, kCandidateLimit};
  if (d != h.table_d) return {ISL_ERR_DIMENSION_MISMATCH, kDimMismatch};
  if (h.recompute) return {ISL_ERR_UNSUPPORTED, kRecompute};
  if (h.is_hnsw) return {ISL_ERR_UNSUPPORTED, kHnsw};
  if (nq > 0x7FFFFFFFull) return {ISL_ERR_INVALID_ARGUMENT, kQueryLimit};
  return {ISL_OK, kPass};
}

}  // namespace isl_refine
