// Host-only arithmetic of a row table (row_table.hpp): how rows of any stored type are laid out on the
// device and what the passes over them are cut into.  Plain C++ without a device header, so that
// tests/cpp/row_table_dump.cpp prints it without a device.  This is the one place the layout rule is written:
// a row starts 16-byte aligned, the block ends in 1 KiB of slack for whole-tile reads past the last row,
// padding and slack are zero.
#pragma once

#include <algorithm>
#include <cstdint>

#include "../../include/islands_amd.h"

namespace isl_rows {

constexpr uint64_t kRowAlignBytes = 16, kSlackBytes = 1024;
constexpr uint64_t kNormChunkBytes = 256ull << 20;  // f32 images of bf16 / fp8 rows widened at a time for their norms
constexpr int32_t kMinScaleExp = -32, kMaxScaleExp = 32;  // the power-of-two scale of an fp8 table

// bytes of one element of a row of `dtype` (ISL_DTYPE_F32 / ISL_DTYPE_BF16 / ISL_DTYPE_FP8_E4M3)
inline uint64_t elem_size(int32_t dtype) { return dtype == ISL_DTYPE_FP8_E4M3 ? 1 : dtype == ISL_DTYPE_BF16 ? 2 : 4; }
// elements from one row to the next: d rounded up to 4 floats / 8 bf16 / 16 fp8 codes
inline uint64_t stride(int32_t dtype, uint64_t d) {
  const uint64_t per = kRowAlignBytes / elem_size(dtype);
  return (d + per - 1) / per * per;
}
// elements of slack behind the last row: 256 floats / 512 bf16 / 1024 fp8 codes
inline uint64_t slack(int32_t dtype) { return kSlackBytes / elem_size(dtype); }
// elements of a block of n rows (a table with a capacity: of `capacity` rows)
inline uint64_t alloc_elems(int32_t dtype, uint64_t n, uint64_t d) { return n * stride(dtype, d) + slack(dtype); }

// A table with room for `capacity` rows keeps every element behind its last row zero, to the end of the slack.
// What the passes that write rows must clear to keep that:
// ... fill of rows [first, first + count): the slack, when the rows end the block (elements behind the rows)
inline uint64_t fill_tail_elems(int32_t dtype, uint64_t capacity, uint64_t first, uint64_t count) {
  return first + count == capacity ? slack(dtype) : 0;
}
// ... the elements from row `first` to the end of the block (a fresh reservation, a failed append)
inline uint64_t tail_elems(int32_t dtype, uint64_t capacity, uint64_t d, uint64_t first) {
  return (capacity - first) * stride(dtype, d) + slack(dtype);
}
// ... the compaction of n0 rows to n: the vacated rows [n, n0) (what lies behind them is zero already)
inline uint64_t vacated_elems(int32_t dtype, uint64_t d, uint64_t n, uint64_t n0) { return (n0 - n) * stride(dtype, d); }

// The norms of bf16 and fp8 rows come from the f32 kernel over widened chunks: rows per chunk, and the floats of the
// chunk buffer (an f32 table of that many rows).
inline uint64_t norm_chunk_rows(uint64_t n, uint64_t d) {
  return std::max<uint64_t>(1, std::min<uint64_t>(n, kNormChunkBytes / (stride(ISL_DTYPE_F32, d) * 4)));
}
inline uint64_t norm_chunk_floats(uint64_t chunk, uint64_t d) { return alloc_elems(ISL_DTYPE_F32, chunk, d); }

// Device bytes of the recompute provider's row cache: an f32 slab of `slab` rows, 12 bytes per slot (norm, owner,
// stamp) and the slot map of nvec + 1 entries.
inline uint64_t recompute_cache_bytes(uint64_t slab, uint64_t d, uint64_t nvec) {
  return alloc_elems(ISL_DTYPE_F32, slab, d) * 4 + slab * 12 + (nvec + 1) * 4;
}

}  // namespace isl_rows
