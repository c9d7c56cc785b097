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
  ~RowTable() { reset(); }  // (a view lets go of blocks that are not its own)
  RowTable& operator=(RowTable&& o) noexcept {
    if (this != &o) {
      reset();  // (a view lets go of its blocks, it does not free them)
      block_ = std::move(o.block_);
      norm2_ = std::move(o.norm2_);
      dtype_ = o.dtype_; scale_exp_ = o.scale_exp_; n_ = o.n_; d_ = o.d_; stride_ = o.stride_;
      capacity_ = o.capacity_; reserved_ = o.reserved_; borrowed_ = o.borrowed_;
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
  uint64_t n() const { return n_; }  // rows the table holds
  // Rows the block and the norms are allocated for, >= n().  Outside a call every element of the block from row n()
  // to the end of the slack is zero (code 0 is +0 for all three types), so whole-tile reads past the last row land
  // on zeros whatever the capacity.  A table nobody reserved has capacity() == n().
  uint64_t capacity() const { return capacity_; }
  // made by a reservation (isl_index_reserve): inserts append into it and removals compact it in place
  bool reserved() const { return reserved_; }
  // a view (view_of): the blocks belong to another table and are not freed with this one
  bool borrowed() const { return borrowed_; }
  // bytes of the allocated block
  uint64_t block_bytes() const { return isl_rows::alloc_elems(dtype_, capacity_, d_) * isl_rows::elem_size(dtype_); }
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
    if (borrowed_) { (void)block_.release(); (void)norm2_.release(); }
    block_.reset();
    norm2_.reset();
    dtype_ = ISL_DTYPE_F32;
    scale_exp_ = 0;
    n_ = d_ = stride_ = capacity_ = 0;
    reserved_ = borrowed_ = false;
  }
  // A block and norms for n rows of d elements, contents undefined.  What the table held goes first (it may be
  // most of the card); after a failure the table is empty.
  isl_status allocate(int32_t dtype, uint64_t n, uint64_t d) { return allocate(dtype, n, d, n, false); }
  // ... with room for `capacity` >= n rows.  The caller zeroes what lies behind row n (zero_from) once the rows are in.
  isl_status allocate(int32_t dtype, uint64_t n, uint64_t d, uint64_t capacity, bool reserved) {
    reset();
    if (block_.reserve(isl_rows::alloc_elems(dtype, capacity, d) * isl_rows::elem_size(dtype)) != ISL_OK ||
        norm2_.reserve(capacity) != ISL_OK) {
      reset();
      return ISL_ERR_DEVICE;
    }
    dtype_ = dtype; n_ = n; d_ = d; stride_ = isl_rows::stride(dtype, d);
    capacity_ = capacity; reserved_ = reserved;
    return ISL_OK;
  }
  // The first `n` <= t.capacity() rows of `t` as a table that owns nothing: what a construction graph reads while it
  // appends into the reserved table of the index that grows.
  static RowTable view_of(const RowTable& t, uint64_t n) {
    RowTable v;
    v.block_.adopt(t.block_.get(), t.block_.capacity());
    v.norm2_.adopt(t.norm2_.get(), t.norm2_.capacity());
    v.dtype_ = t.dtype_; v.scale_exp_ = t.scale_exp_; v.n_ = n; v.d_ = t.d_; v.stride_ = t.stride_;
    v.capacity_ = t.capacity_; v.reserved_ = t.reserved_; v.borrowed_ = true;
    return v;
  }
  // n rows of d elements of `dtype` in a block and norms that belong to someone else (the refine table's pinned host
  // block, through its device pointer): laid out as allocate() lays a table out, block_elems >= alloc_elems(dtype, n, d)
  static RowTable view_over(void* block, uint64_t block_elems, float* norm2, int32_t dtype, uint64_t n, uint64_t d) {
    RowTable v;
    v.block_.adopt(static_cast<unsigned char*>(block), block_elems * isl_rows::elem_size(dtype));
    v.norm2_.adopt(norm2, n);
    v.dtype_ = dtype; v.n_ = n; v.d_ = d; v.stride_ = isl_rows::stride(dtype, d);
    v.capacity_ = n; v.borrowed_ = true;
    return v;
  }
  // the row count of a table with room: rows appended in place become visible, or a compacted table ends earlier
  void set_n(uint64_t n) { n_ = n; }
  // api_index.hip -- rows [first, first + count) from `src` (count x d elements of the table's type, host or
  // device memory as `mem` says), their padding zeroed, and their norms; when they end the block (row capacity())
  // the slack is zeroed with them.  Rows filled behind n() stay invisible until set_n.  Returns once the device is done.
  isl_status fill(uint64_t first, uint64_t count, const void* src, int32_t mem);
  // api_index.hip -- the norms of rows [first, first + count) from the rows' images as the block holds them (fill's
  // own second half: whatever writes rows into the block itself, as the conversion does, ends with this).  Returns
  // once the device is done.
  isl_status norms(uint64_t first, uint64_t count);
  // ... every row, norm and the slack zero (the recompute provider's slab: nothing is uploaded)
  isl_status zero();
  // ... the block from row `first` to the end of the slack, and the norms of rows [first, capacity()), zero
  isl_status zero_from(uint64_t first);

 private:
  DeviceBuffer<unsigned char> block_;
  DeviceBuffer<float> norm2_;
  int32_t dtype_ = ISL_DTYPE_F32, scale_exp_ = 0;
  uint64_t n_ = 0, d_ = 0, stride_ = 0, capacity_ = 0;
  bool reserved_ = false, borrowed_ = false;
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

// The refine table (search_refine.hip): a second table of len rows, f32 or bf16, that a refined search re-scores its
// candidates against.  ISL_REFINE_DEVICE: `dev` is a table like the provider's.  ISL_REFINE_HOST: the rows lie in
// `host`, one pinned, device-mapped block in the same layout, and `view` reads it through its device pointer beside
// `host_norm2`, the norms on the device.  No table = both empty (the default).
struct RefineTable {
  int32_t placement = 0;  // ISL_REFINE_*
  RowTable dev;
  PinnedBuffer<unsigned char> host;
  DeviceBuffer<float> host_norm2;
  RowTable view;  // borrowed: over `host` and `host_norm2`
  const RowTable& rows() const { return placement == 1 ? view : dev; }
  uint64_t n() const { return rows().n(); }
  // (the view lets go before the blocks it reads are freed)
  void reset() { view.reset(); host.reset(); host_norm2.reset(); dev.reset(); placement = 0; }
};

}  // namespace isl
