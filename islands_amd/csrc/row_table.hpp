// The rows of an index on the device: one block of n rows of d elements of one stored type, `stride` elements
// apart (row_table_plan.hpp has the layout rule), and the sum of squares of every row.  Owning and move-only;
// a moved-from or reset table is empty with every scalar 0.  The entry seeds are a second table of the same
// type at the same stride.
#pragma once

#include <utility>
#include <vector>

#include "device_buffer.hpp"
#include "row_table_plan.hpp"

namespace isl {

// the row type tag of fp8 rows (OCP e4m3fn codes): a type of its own, so that no `sizeof(ROWT)` test written for
// float and uint16_t rows takes it for one of them
struct fp8_e4m3 { uint8_t v; };

class RowTable {
 public:
  RowTable() = default;
  RowTable(RowTable&& o) noexcept { *this = std::move(o); }
  RowTable& operator=(RowTable&& o) noexcept {
    if (this != &o) {
      block_ = std::move(o.block_);
      norm2_ = std::move(o.norm2_);
      dtype_ = o.dtype_; scale_exp_ = o.scale_exp_; n_ = o.n_; d_ = o.d_; stride_ = o.stride_;
      o.reset();
    }
    return *this;
  }

  int32_t dtype() const { return dtype_; }
  bool is_bf16() const { return dtype_ == ISL_DTYPE_BF16; }
  bool is_fp8() const { return dtype_ == ISL_DTYPE_FP8_E4M3; }
  // fp8 rows: the element of code c is e4m3(c) * 2^scale_exp (0 for the other types)
  int32_t scale_exp() const { return scale_exp_; }
  void set_scale_exp(int32_t e) { scale_exp_ = e; }
  bool resident() const { return block_.get() != nullptr; }
  uint64_t n() const { return n_; }  // rows in the block
  uint64_t d() const { return d_; }
  uint64_t stride() const { return stride_; }  // in elements of the stored type
  const void* data() const { return block_.get(); }
  // the block as rows of T; f32() / bf16() / fp8() are NULL for a table of another type
  template <typename T>
  T* as() const { return reinterpret_cast<T*>(block_.get()); }
  float* f32() const { return dtype_ == ISL_DTYPE_F32 ? as<float>() : nullptr; }
  uint16_t* bf16() const { return is_bf16() ? as<uint16_t>() : nullptr; }
  uint8_t* fp8() const { return is_fp8() ? as<uint8_t>() : nullptr; }
  float* norm2() const { return norm2_.get(); }  // [n], the reference's summation order

  // f(float{}), f(uint16_t{}) or f(fp8_e4m3{}): the one place a kernel template's row type is chosen at run
  // time.  A caller whose kernels do not take fp8 rows (build, repair, entry seeds) refuses such a table before
  // it gets here and leaves the third tag's branch empty (`if constexpr`), so that nothing is instantiated for it.
  template <typename F>
  void with_row_type(F&& f) const {
    if (is_fp8()) f(fp8_e4m3{});
    else if (is_bf16()) f(uint16_t{});
    else f(float{});
  }

  // the type alone, for a table that holds no block (what the launch geometry reads)
  void set_dtype(int32_t dtype) { dtype_ = dtype; }
  void reset() {
    block_.reset();
    norm2_.reset();
    dtype_ = ISL_DTYPE_F32;
    scale_exp_ = 0;
    n_ = d_ = stride_ = 0;
  }
  // A block and norms for n rows of d elements, contents undefined.  What the table held goes first (it may be
  // most of the card); after a failure the table is empty.
  isl_status allocate(int32_t dtype, uint64_t n, uint64_t d) {
    reset();
    if (block_.reserve(isl_rows::alloc_elems(dtype, n, d) * isl_rows::elem_size(dtype)) != ISL_OK ||
        norm2_.reserve(n) != ISL_OK) {
      reset();
      return ISL_ERR_DEVICE;
    }
    dtype_ = dtype; n_ = n; d_ = d; stride_ = isl_rows::stride(dtype, d);
    return ISL_OK;
  }
  // api_index.hip -- rows [first, first + count) from `src` (count x d elements of the table's type, host or
  // device memory as `mem` says), their padding zeroed, and their norms; when they are the table's last rows the
  // slack is zeroed with them.  Returns once the device is done.
  isl_status fill(uint64_t first, uint64_t count, const void* src, int32_t mem);
  // api_index.hip -- the norms of rows [first, first + count) from the rows' images as the block holds them (fill's
  // own second half: whatever writes rows into the block itself, as the conversion does, ends with this).  Returns
  // once the device is done.
  isl_status norms(uint64_t first, uint64_t count);
  // ... every row, norm and the slack zero (the recompute provider's slab: nothing is uploaded)
  isl_status zero();

 private:
  DeviceBuffer<unsigned char> block_;
  DeviceBuffer<float> norm2_;
  int32_t dtype_ = ISL_DTYPE_F32, scale_exp_ = 0;
  uint64_t n_ = 0, d_ = 0, stride_ = 0;
};

// Entry seeds (entry_seeds.hip): node ids and a contiguous copy of their rows and norms, of the type and at the
// stride of the table they were gathered from.  No seeds = an empty table (the default); whatever replaces the
// rows they were copied from assigns an empty one.
struct EntrySeeds {
  std::vector<uint64_t> ids;
  DeviceBuffer<uint32_t> d_ids;  // [count()]
  RowTable rows;
  uint64_t count() const { return rows.n(); }
};

}  // namespace isl
