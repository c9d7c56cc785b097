// Row conversions on the device: rows of one stored type (f32, bf16 bit patterns, e4m3 codes under one
// power-of-two scale) become rows of another, element by element, new = narrow_T(image(old)) with the
// definitions of row_convert_plan.hpp.  Two passes, both bandwidth-bound streams without LDS tiles:
//   absmax   the largest |image| of a table as an unsigned maximum of the bit patterns (automatic scale only)
//   convert  template <SRC, DST>: a lane owns 16 consecutive elements of a row -- four 16-byte loads of f32,
//            two of bf16, one of fp8 -- and writes them with whole 16-byte stores, following the source's and
//            the destination's stride; the padding of the destination is written as zero
// The narrowing is the integer arithmetic of the plan header compiled for the device, so the host test of that
// header pins what runs here; the widening of a code is the hardware's scaled convert (fp8_image), which the
// search kernels already rely on for every code and scale.
// Entry points: isl_quantize_fp8_e4m3, isl_round_bf16 (dense buffers of the caller's), isl_index_convert_rows
// (the resident table of a LeannIndex, built beside the old one and moved in at the end) and isl_index_read_rows.
#include "device_common.hip.h"
#include "row_convert_plan.hpp"

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

namespace {

using isl::fail;
using isl::fp8_e4m3;
using isl::RowTable;
using namespace isl_convert;

constexpr uint32_t kBlock = 256, kMaxGrid = 2048;  // 8 workgroups per CU, the rest is a grid stride
constexpr uint32_t kFlagNaN = 1u;

// what the passes leave for the host: 8 bytes
struct PassResult { uint32_t absmax_bits, flags; };

template <typename T> struct is_fp8 : std::is_same<T, fp8_e4m3> {};

// ------------------------------------------------------------------ absmax
// The maximum of bits & 0x7FFFFFFF over the images of `vectors` 16-byte words at `p` (16-byte aligned) and of
// the `head` elements in front of them and the `tail` elements behind: a NaN is the only pattern above
// infinity's, so it both wins the maximum and raises the flag.  SRC = float or uint16_t (an fp8 table never
// needs a scale).  A wave reduction, the waves' maxima through LDS, one atomicMax per workgroup.
template <typename SRC>
__global__ __launch_bounds__(kBlock) void absmax_kernel(const SRC* __restrict__ elems, uint64_t head, uint64_t vectors,
                                                        uint64_t tail, PassResult* __restrict__ out) {
  constexpr uint32_t per = 16 / sizeof(SRC);
  const uint4* p = reinterpret_cast<const uint4*>(elems + head);
  uint32_t m = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < vectors; i += (uint64_t)gridDim.x * kBlock) {
    const uint4 v = p[i];
    if constexpr (sizeof(SRC) == 4) {
      m = max(max(m, v.x & kAbsMask), max(max(v.y & kAbsMask, v.z & kAbsMask), v.w & kAbsMask));
    } else {
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) m = max(m, max((w[j] << 16) & kAbsMask, w[j] & 0x7FFF0000u));
    }
  }
  if (blockIdx.x == 0) {  // the few elements an unaligned dense buffer leaves at either end
    const uint64_t t = threadIdx.x;
    auto bits = [](SRC e) -> uint32_t {
      if constexpr (sizeof(SRC) == 4) return __float_as_uint(e) & kAbsMask;
      else return ((uint32_t)e << 16) & kAbsMask;
    };
    if (t < head) m = max(m, bits(elems[t]));
    if (t < tail) m = max(m, bits(elems[head + vectors * per + t]));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
  __shared__ uint32_t wave_max[kBlock / 64];
  if ((threadIdx.x & 63u) == 0) wave_max[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (uint32_t w = 1; w < kBlock / 64; ++w) m = max(m, wave_max[w]);
    if (m) atomicMax(&out->absmax_bits, m);
    if (m > kInfBits) atomicOr(&out->flags, kFlagNaN);
  }
}

// ------------------------------------------------------------------ convert
struct ConvertParams {
  const void* src;
  void* dst;
  uint64_t n, d;              // rows and elements per row
  uint64_t sstride, dstride;  // in elements of either type
  float src_scale;            // SRC = fp8: 2^scale_exp of the source table
  int32_t dst_exp;            // DST = fp8: the exponent the codes are made under
  uint32_t vec;               // every row of both sides starts 16-byte aligned
  PassResult* out;            // flags |= kFlagNaN when a NaN image meets DST = fp8
};

// the f32 image of one stored element, as bits
__device__ __forceinline__ uint32_t image_bits(float v, float) { return __float_as_uint(v); }
__device__ __forceinline__ uint32_t image_bits(uint16_t v, float) { return (uint32_t)v << 16; }
__device__ __forceinline__ uint32_t image_bits(fp8_e4m3 v, float scale) {
  return __float_as_uint(isl_dev::fp8_image(v.v, scale));
}

// the images of 16 consecutive elements from 16-byte loads
template <typename SRC>
__device__ __forceinline__ void load16(const SRC* __restrict__ at, float scale, uint32_t (&img)[16]) {
  const uint4* p = reinterpret_cast<const uint4*>(at);
  if constexpr (std::is_same<SRC, float>::value) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint4 v = p[i];
      img[4 * i] = v.x; img[4 * i + 1] = v.y; img[4 * i + 2] = v.z; img[4 * i + 3] = v.w;
    }
  } else if constexpr (std::is_same<SRC, uint16_t>::value) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const uint4 v = p[i];
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        img[8 * i + 2 * j] = w[j] << 16;
        img[8 * i + 2 * j + 1] = w[j] & 0xFFFF0000u;
      }
    }
  } else {
    const uint4 v = p[0];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const isl_dev::v2f lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[j], scale, false),
                         hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[j], scale, true);
      img[4 * j] = __float_as_uint(lo.x); img[4 * j + 1] = __float_as_uint(lo.y);
      img[4 * j + 2] = __float_as_uint(hi.x); img[4 * j + 3] = __float_as_uint(hi.y);
    }
  }
}

// ... narrowed and written with 16-byte stores
template <typename DST>
__device__ __forceinline__ void store16(DST* __restrict__ at, int32_t e, const uint32_t (&img)[16]) {
  uint4* p = reinterpret_cast<uint4*>(at);
  if constexpr (std::is_same<DST, float>::value) {
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = make_uint4(img[4 * i], img[4 * i + 1], img[4 * i + 2], img[4 * i + 3]);
  } else if constexpr (std::is_same<DST, uint16_t>::value) {
    uint32_t w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = (uint32_t)narrow_bf16(img[2 * j]) | ((uint32_t)narrow_bf16(img[2 * j + 1]) << 16);
    p[0] = make_uint4(w[0], w[1], w[2], w[3]);
    p[1] = make_uint4(w[4], w[5], w[6], w[7]);
  } else {
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      w[j] = (uint32_t)narrow_e4m3(img[4 * j], e) | ((uint32_t)narrow_e4m3(img[4 * j + 1], e) << 8) |
             ((uint32_t)narrow_e4m3(img[4 * j + 2], e) << 16) | ((uint32_t)narrow_e4m3(img[4 * j + 3], e) << 24);
    p[0] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

__device__ __forceinline__ void store1(float* at, int32_t, uint32_t img) { *at = __uint_as_float(img); }
__device__ __forceinline__ void store1(uint16_t* at, int32_t, uint32_t img) { *at = narrow_bf16(img); }
__device__ __forceinline__ void store1(fp8_e4m3* at, int32_t e, uint32_t img) { at->v = narrow_e4m3(img, e); }

// Work item = (row, chunk of 16 elements).  A chunk that lies whole inside the row's d elements goes through the
// 16-byte path; the last chunk of a row whose d is no multiple of 16 -- and every chunk when a side is not
// 16-byte aligned (a dense buffer of the caller's) -- goes element by element, up to the destination's stride:
// the elements past d are the padding, written as zero (code 0 is +0).  Every index is 64 bits wide.
template <typename SRC, typename DST>
__global__ __launch_bounds__(kBlock) void convert_rows_kernel(ConvertParams p) {
  const SRC* __restrict__ src = static_cast<const SRC*>(p.src);
  DST* __restrict__ dst = static_cast<DST*>(p.dst);
  const uint64_t cpr = (p.d + kElemsPerLane - 1) / kElemsPerLane, items = p.n * cpr;
  bool nan = false;
  for (uint64_t it = (uint64_t)blockIdx.x * kBlock + threadIdx.x; it < items; it += (uint64_t)gridDim.x * kBlock) {
    const uint64_t r = it / cpr, c0 = (it - r * cpr) * kElemsPerLane;
    const SRC* s = src + r * p.sstride + c0;
    DST* t = dst + r * p.dstride + c0;
    if (p.vec && c0 + kElemsPerLane <= p.d) {
      uint32_t img[16];
      load16<SRC>(s, p.src_scale, img);
      if constexpr (is_fp8<DST>::value) {
#pragma unroll
        for (int j = 0; j < 16; ++j) nan |= is_nan_bits(img[j]);
      }
      store16<DST>(t, p.dst_exp, img);
    } else {
      const uint64_t left = p.dstride - c0, end = left < kElemsPerLane ? left : kElemsPerLane;
      for (uint64_t j = 0; j < end; ++j) {
        const uint32_t img = c0 + j < p.d ? image_bits(s[j], p.src_scale) : 0u;
        if constexpr (is_fp8<DST>::value) nan |= is_nan_bits(img);
        store1(t + j, p.dst_exp, img);
      }
    }
  }
  if constexpr (is_fp8<DST>::value) {
    if (nan) atomicOr(&p.out->flags, kFlagNaN);
  }
}

template <typename F>
void by_row_type(int32_t dtype, F&& f) {
  if (dtype == ISL_DTYPE_FP8_E4M3) f(fp8_e4m3{});
  else if (dtype == ISL_DTYPE_BF16) f(uint16_t{});
  else f(float{});
}

bool known_dtype(int32_t dtype) {
  return dtype == ISL_DTYPE_F32 || dtype == ISL_DTYPE_BF16 || dtype == ISL_DTYPE_FP8_E4M3;
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// n rows of d elements from `src` (sdtype, sstride) to `dst` (ddtype, dstride) on `st`; nothing is waited for
void launch_convert(const void* src, int32_t sdtype, uint64_t sstride, int32_t src_exp, void* dst, int32_t ddtype,
                    uint64_t dstride, int32_t dst_exp, uint64_t n, uint64_t d, PassResult* out, hipStream_t st) {
  ConvertParams p{src, dst, n, d, sstride, dstride, std::ldexp(1.0f, src_exp), dst_exp, 0u, out};
  p.vec = aligned16(src) && aligned16(dst) && (n == 1 || ((sstride * isl_rows::elem_size(sdtype)) % 16 == 0 &&
                                                          (dstride * isl_rows::elem_size(ddtype)) % 16 == 0));
  const uint32_t grid = grid_for(n * chunks_per_row(d), kBlock, kMaxGrid);
  by_row_type(sdtype, [&](auto s) {
    by_row_type(ddtype, [&](auto t) {
      hipLaunchKernelGGL((convert_rows_kernel<decltype(s), decltype(t)>), dim3(grid), dim3(kBlock), 0, st, p);
    });
  });
}

// the largest |image| of `count` elements of f32 or bf16 at `src` on `st`; nothing is waited for
void launch_absmax(const void* src, int32_t sdtype, uint64_t count, PassResult* out, hipStream_t st) {
  const uint64_t es = isl_rows::elem_size(sdtype), per = 16 / es;
  const uint64_t off = reinterpret_cast<uintptr_t>(src) & 15u;
  // (a pointer that is not even element-aligned has no aligned middle: everything would be head, which only a
  // buffer of a few elements can be -- the entry points refuse such a pointer)
  const uint64_t head = std::min<uint64_t>(count, off ? (16 - off) / es : 0);
  const uint64_t vectors = (count - head) / per, tail = count - head - vectors * per;
  const uint32_t grid = grid_for(vectors, kBlock, kMaxGrid);
  if (sdtype == ISL_DTYPE_BF16)
    hipLaunchKernelGGL(absmax_kernel<uint16_t>, dim3(grid), dim3(kBlock), 0, st, static_cast<const uint16_t*>(src), head,
                       vectors, tail, out);
  else
    hipLaunchKernelGGL(absmax_kernel<float>, dim3(grid), dim3(kBlock), 0, st, static_cast<const float*>(src), head,
                       vectors, tail, out);
}

isl_status nan_refused(const char* who) {
  return fail(ISL_ERR_INVALID_ARGUMENT, "%s: a NaN among the rows has no e4m3 code", who);
}

// A dense n x d float32 buffer narrowed to `ddtype` (bf16 or fp8) into a dense buffer, host or device memory
// alike: the convert kernel over one row of n * d elements.  *exp_io: the exponent (fp8), ISL_FP8_SCALE_AUTO on
// entry = taken from the rows.
isl_status narrow_dense(const char* who, const float* rows, uint64_t count, int32_t ddtype, void* out, int32_t* exp_io,
                        int32_t mem, int32_t device, hipStream_t st) {
  ISL_TRY(isl::use_device(device));
  const uint64_t des = isl_rows::elem_size(ddtype);
  isl::DeviceBuffer<float> d_rows;
  isl::DeviceBuffer<unsigned char> d_out;
  isl::DeviceBuffer<PassResult> d_res;
  const float* src = rows;
  void* dst = out;
  ISL_TRY(d_res.reserve(1));
  ISL_HIP(hipMemsetAsync(d_res, 0, sizeof(PassResult), st));
  if (mem == ISL_MEM_HOST) {
    ISL_TRY(d_rows.reserve(count));
    ISL_TRY(d_out.reserve(count * des));
    ISL_HIP(hipMemcpyAsync(d_rows, rows, (size_t)count * 4, hipMemcpyHostToDevice, st));
    src = d_rows;
    dst = d_out;
  }
  PassResult res{};
  int32_t e = 0;
  if (ddtype == ISL_DTYPE_FP8_E4M3) {
    e = *exp_io;
    if (e == ISL_FP8_SCALE_AUTO) {
      launch_absmax(src, ISL_DTYPE_F32, count, d_res, st);
      ISL_HIP(hipGetLastError());
      ISL_HIP(hipMemcpyAsync(&res, d_res, sizeof(res), hipMemcpyDeviceToHost, st));
      ISL_HIP(hipStreamSynchronize(st));
      if (res.flags & kFlagNaN) return nan_refused(who);
      e = scale_exp_for(res.absmax_bits);
    }
  }
  launch_convert(src, ISL_DTYPE_F32, count, 0, dst, ddtype, count, e, 1, count, d_res, st);
  ISL_HIP(hipGetLastError());
  ISL_HIP(hipMemcpyAsync(&res, d_res, sizeof(res), hipMemcpyDeviceToHost, st));
  if (mem == ISL_MEM_HOST) ISL_HIP(hipMemcpyAsync(out, d_out, (size_t)(count * des), hipMemcpyDeviceToHost, st));
  ISL_HIP(hipStreamSynchronize(st));
  if (res.flags & kFlagNaN) return nan_refused(who);
  if (ddtype == ISL_DTYPE_FP8_E4M3) *exp_io = e;
  return ISL_OK;
}

// what the two index calls ask of the handle: rows of the in-memory provider resident on the device
isl_status check_resident(const isl_index* idx, const char* who) {
  if (idx->recompute)
    return fail(ISL_ERR_UNSUPPORTED, "%s: an index on the recompute provider stores no rows", who);
  if (idx->device < 0 || !idx->rows.resident() || !idx->rows.norm2() || idx->rows.n() != idx->nvec || idx->nvec == 0)
    return fail(ISL_ERR_UNSUPPORTED, "%s needs the index's rows resident on the device (isl_index_upload, "
                "isl_set_embeddings)", who);
  return ISL_OK;
}

}  // namespace

extern "C" {

isl_status isl_quantize_fp8_e4m3(const float* rows, uint64_t n, uint64_t d, int32_t scale_exp, uint8_t* codes,
                                 int32_t* out_scale_exp, int32_t mem, int32_t device, void* stream) {
  const uint64_t count = n * d;
  if (count && (!rows || !codes)) return fail(ISL_ERR_INVALID_ARGUMENT, "isl_quantize_fp8_e4m3: NULL buffer");
  if (mem != ISL_MEM_HOST && mem != ISL_MEM_DEVICE) return fail(ISL_ERR_INVALID_ARGUMENT, "isl_quantize_fp8_e4m3: unknown mem");
  if (scale_exp != ISL_FP8_SCALE_AUTO && (scale_exp < isl_rows::kMinScaleExp || scale_exp > isl_rows::kMaxScaleExp))
    return fail(ISL_ERR_INVALID_ARGUMENT, "isl_quantize_fp8_e4m3: scale_exp = %d is neither ISL_FP8_SCALE_AUTO nor in "
                "[%d, %d]", scale_exp, isl_rows::kMinScaleExp, isl_rows::kMaxScaleExp);
  if ((reinterpret_cast<uintptr_t>(rows) & 3u) != 0)
    return fail(ISL_ERR_INVALID_ARGUMENT, "isl_quantize_fp8_e4m3: rows is not aligned to a float");
  int32_t e = scale_exp;
  if (count == 0) e = scale_exp == ISL_FP8_SCALE_AUTO ? isl_rows::kMinScaleExp : scale_exp;
  else ISL_TRY(narrow_dense("isl_quantize_fp8_e4m3", rows, count, ISL_DTYPE_FP8_E4M3, codes, &e, mem, device,
                            (hipStream_t)stream));
  if (out_scale_exp) *out_scale_exp = e;
  return ISL_OK;
}

isl_status isl_round_bf16(const float* rows, uint64_t n, uint64_t d, uint16_t* bits, int32_t mem, int32_t device,
                          void* stream) {
  const uint64_t count = n * d;
  if (count && (!rows || !bits)) return fail(ISL_ERR_INVALID_ARGUMENT, "isl_round_bf16: NULL buffer");
  if (mem != ISL_MEM_HOST && mem != ISL_MEM_DEVICE) return fail(ISL_ERR_INVALID_ARGUMENT, "isl_round_bf16: unknown mem");
  if ((reinterpret_cast<uintptr_t>(rows) & 3u) != 0 || (reinterpret_cast<uintptr_t>(bits) & 1u) != 0)
    return fail(ISL_ERR_INVALID_ARGUMENT, "isl_round_bf16: a buffer is not aligned to its element");
  if (count == 0) return ISL_OK;
  return narrow_dense("isl_round_bf16", rows, count, ISL_DTYPE_BF16, bits, nullptr, mem, device, (hipStream_t)stream);
}

isl_status isl_index_convert_rows(isl_index* idx, int32_t dtype, int32_t scale_exp) {
  static const char* who = "isl_index_convert_rows";
  if (!idx) return fail(ISL_ERR_INVALID_ARGUMENT, "index is NULL");
  if (!known_dtype(dtype)) return fail(ISL_ERR_INVALID_ARGUMENT, "unknown row dtype");
  const bool to_fp8 = dtype == ISL_DTYPE_FP8_E4M3, auto_scale = scale_exp == ISL_FP8_SCALE_AUTO;
  if (to_fp8 && !auto_scale && (scale_exp < isl_rows::kMinScaleExp || scale_exp > isl_rows::kMaxScaleExp))
    return fail(ISL_ERR_INVALID_ARGUMENT, "fp8 rows: scale_exp = %d is neither ISL_FP8_SCALE_AUTO nor in [%d, %d]", scale_exp,
                isl_rows::kMinScaleExp, isl_rows::kMaxScaleExp);
  if (idx->is_hnsw)
    return fail(ISL_ERR_UNSUPPORTED, "%s: this is the core index of an HnswGraph, whose rows keep their type", who);
  ISL_TRY(check_resident(idx, who));
  {  // the &mut self of the reference: not beside a search on the same handle
    std::lock_guard<std::mutex> lock(idx->mu);
    if (isl::any_lane_busy(idx))
      return fail(ISL_ERR_SEARCH, "Search error: the rows cannot be converted while searches are in flight");
  }
  const RowTable& old = idx->rows;
  if (old.dtype() == dtype) {
    if (!to_fp8 || auto_scale || scale_exp == old.scale_exp()) return ISL_OK;
    return fail(ISL_ERR_UNSUPPORTED, "%s: fp8 rows under scale_exp = %d are not made into fp8 rows under %d (widen them "
                "first)", who, old.scale_exp(), scale_exp);
  }
  ISL_TRY(isl::use_device(idx->device));
  // the new table beside the old one, which nothing below writes
  const uint64_t n = old.n(), d = old.d();
  RowTable fresh;
  isl::DeviceBuffer<PassResult> d_res;
  ISL_TRY(fresh.allocate(dtype, n, d, old.capacity(), old.reserved()));  // (a reservation outlives the conversion)
  ISL_TRY(d_res.reserve(1));
  ISL_HIP(hipMemset(d_res, 0, sizeof(PassResult)));
  PassResult res{};
  int32_t e = to_fp8 ? scale_exp : 0;
  if (to_fp8 && auto_scale) {  // (the source is f32 or bf16; its padding is zero and takes no part in a maximum)
    launch_absmax(old.data(), old.dtype(), n * old.stride(), d_res, nullptr);
    ISL_HIP(hipGetLastError());
    ISL_HIP(hipMemcpy(&res, d_res, sizeof(res), hipMemcpyDeviceToHost));
    if (res.flags & kFlagNaN) return nan_refused(who);
    e = scale_exp_for(res.absmax_bits);
  }
  fresh.set_scale_exp(e);  // (before the norms: they are the images')
  launch_convert(old.data(), old.dtype(), old.stride(), old.scale_exp(), fresh.as<void>(), dtype, fresh.stride(), e, n, d,
                 d_res, nullptr);
  ISL_HIP(hipGetLastError());
  ISL_TRY(fresh.zero_from(n));  // (a table nobody reserved: the slack)
  ISL_HIP(hipMemcpy(&res, d_res, sizeof(res), hipMemcpyDeviceToHost));
  if (res.flags & kFlagNaN) return nan_refused(who);
  ISL_TRY(fresh.norms(0, n));
  // the move; entry seeds are copies of the old rows: an f32 / bf16 table gathers them again under the same ids
  // (as isl_index_remove does for its survivors), an fp8 index carries none
  std::vector<uint64_t> seeds;
  {
    std::lock_guard<std::mutex> lock(idx->mu);
    if (isl::any_lane_busy(idx))
      return fail(ISL_ERR_SEARCH, "Search error: the rows cannot be converted while searches are in flight");
    if (!to_fp8) seeds = idx->seeds.ids;
    idx->seeds = {};
    idx->rows = std::move(fresh);
    ++idx->row_allocations;
  }
  if (!seeds.empty() && isl_index_set_entry_seeds(idx, seeds.data(), seeds.size()) != ISL_OK) isl::last_error() = {};
  return ISL_OK;
}

isl_status isl_index_read_rows(const isl_index* idx, uint64_t first, uint64_t count, void* out, int32_t mem) {
  static const char* who = "isl_index_read_rows";
  if (!idx || (!out && count)) return fail(ISL_ERR_INVALID_ARGUMENT, "NULL argument");
  if (mem != ISL_MEM_HOST && mem != ISL_MEM_DEVICE) return fail(ISL_ERR_INVALID_ARGUMENT, "%s: unknown mem", who);
  ISL_TRY(check_resident(idx, who));
  std::lock_guard<std::mutex> lock(idx->mu);
  const RowTable& t = idx->rows;
  if (first > t.n() || count > t.n() - first) return isl::fail_node(std::max<uint64_t>(first, t.n()));
  if (count == 0) return ISL_OK;
  // (a caller sizes `out` by isl_index_dimension where the handle has one)
  if (idx->has_dimension && idx->dimension != t.d()) return isl::fail_dim(idx->dimension, t.d());
  ISL_TRY(isl::use_device(idx->device));
  const uint64_t es = isl_rows::elem_size(t.dtype()), row = t.d() * es, pitch = t.stride() * es;
  ISL_HIP(hipMemcpy2D(out, row, t.as<unsigned char>() + first * pitch, pitch, row, count,
                      mem == ISL_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
  return ISL_OK;
}

}  // extern "C"
