// leann_search_fast<S = ISL_FAST_S> for every metric, row type and row width (see
// search_kernels.hip.h).  The Makefile compiles this file once per S (1, 2, 4, 8) into
// search_fast<S>.o: four units that build side by side.
#include "search_kernels.hip.h"

#ifndef ISL_FAST_S
#error "compile with -DISL_FAST_S=1, 2, 4 or 8"
#endif

namespace {
template <typename ROWT, bool WIDE, bool RESUME = false, bool QH = false>
void launch_t(int metric, uint32_t grid, size_t lds, hipStream_t st, const SearchParams& p) {
  switch (metric) {
    case ISL_METRIC_COSINE: launch_one(leann_search_fast<ISL_FAST_S, ISL_METRIC_COSINE, ROWT, WIDE, RESUME, QH>, grid, lds, st, p); break;
    case ISL_METRIC_EUCLIDEAN: launch_one(leann_search_fast<ISL_FAST_S, ISL_METRIC_EUCLIDEAN, ROWT, WIDE, RESUME, QH>, grid, lds, st, p); break;
    case ISL_METRIC_DOT: launch_one(leann_search_fast<ISL_FAST_S, ISL_METRIC_DOT, ROWT, WIDE, RESUME, QH>, grid, lds, st, p); break;
    default: launch_one(leann_search_fast<ISL_FAST_S, ISL_METRIC_MANHATTAN, ROWT, WIDE, RESUME, QH>, grid, lds, st, p); break;
  }
}
}  // namespace

template <int S>
void isl_launch::launch_fast_segments(const FastKernel& k, uint32_t grid, size_t lds, hipStream_t st, const void* params) {
  static_assert(S == ISL_FAST_S, "this unit holds one S");
  const SearchParams& p = *static_cast<const SearchParams*>(params);
  if (k.qh) {  // bf16 rows, bf16-valued queries: the query operand stays bf16 in LDS
    launch_t<uint16_t, false, false, true>(k.metric, grid, lds, st, p);
  } else if (k.resume) {  // searches over the recompute provider (f32 rows) that park and resume
    if (k.wide) launch_t<float, true, true>(k.metric, grid, lds, st, p);
    else launch_t<float, false, true>(k.metric, grid, lds, st, p);
  } else if (k.dtype == ISL_DTYPE_BF16) {
    if (k.wide) launch_t<uint16_t, true>(k.metric, grid, lds, st, p);
    else launch_t<uint16_t, false>(k.metric, grid, lds, st, p);
  } else if (k.dtype == ISL_DTYPE_FP8_E4M3) {  // f32 queries over fp8 codes: the f32-query launch geometry
    if (k.wide) launch_t<isl::fp8_e4m3, true>(k.metric, grid, lds, st, p);
    else launch_t<isl::fp8_e4m3, false>(k.metric, grid, lds, st, p);
  } else {
    if (k.wide) launch_t<float, true>(k.metric, grid, lds, st, p);
    else launch_t<float, false>(k.metric, grid, lds, st, p);
  }
}
template void isl_launch::launch_fast_segments<ISL_FAST_S>(const FastKernel&, uint32_t, size_t, hipStream_t, const void*);
