// Ownership of device and pinned-host memory: plain C++ over the HIP runtime API, no kernels.
// A Buffer member frees its block when its owner goes away, a TempScope frees the temporaries of
// one call when the call returns -- by whichever path, so ISL_HIP / ISL_TRY may return early.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/islands_amd.h"

namespace isl {

isl_status fail(isl_status st, const char* fmt, ...);

struct DeviceMemory {
  static hipError_t allocate(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void* p) { (void)hipFree(p); }
  static constexpr const char* kAllocator = "hipMalloc";
};
struct PinnedMemory {
  static hipError_t allocate(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void release(void* p) { (void)hipHostFree(p); }
  static constexpr const char* kAllocator = "hipHostMalloc";
};

// what a request for `count` elements of T asks the allocator for: never zero bytes
template <typename T>
constexpr size_t alloc_bytes(uint64_t count) {
  return count * sizeof(T) < 4 ? 4 : (size_t)(count * sizeof(T));
}

// Owning, move-only array of T.  Reads as a T* wherever one is expected.
template <typename T, typename Space = DeviceMemory>
class Buffer {
 public:
  Buffer() = default;
  Buffer(Buffer&& o) noexcept : ptr_(o.ptr_), cap_(o.cap_) { o.ptr_ = nullptr; o.cap_ = 0; }
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) {
      const uint64_t cap = o.cap_;
      adopt(o.release(), cap);
    }
    return *this;
  }
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  ~Buffer() { reset(); }

  operator T*() const { return ptr_; }
  T* get() const { return ptr_; }
  uint64_t capacity() const { return cap_; }  // in elements

  // Room for `count` elements.  A buffer that has it stays as it is; otherwise the old block is freed
  // first and a new one allocated (contents are not carried over).  *events counts allocations made.
  isl_status reserve(uint64_t count, uint64_t* events = nullptr) {
    if (ptr_ && cap_ >= count) return ISL_OK;
    reset();
    void* p = nullptr;
    const hipError_t e = Space::allocate(&p, alloc_bytes<T>(count));
    if (e != hipSuccess)
      return fail(ISL_ERR_DEVICE, "%s of %zu bytes failed: %s", Space::kAllocator, alloc_bytes<T>(count),
                  hipGetErrorString(e));
    ptr_ = static_cast<T*>(p);
    cap_ = count;
    if (events) ++*events;
    return ISL_OK;
  }
  void reset() {
    if (ptr_) Space::release(ptr_);
    ptr_ = nullptr;
    cap_ = 0;
  }
  // hand-overs: the caller takes the block / this buffer takes a block allocated elsewhere (a
  // Buffer<unsigned char> that adopts with count 0 merely owns a block whose type it does not know)
  T* release() {
    T* p = ptr_;
    ptr_ = nullptr;
    cap_ = 0;
    return p;
  }
  void adopt(T* p, uint64_t count) {
    reset();
    ptr_ = p;
    cap_ = p ? count : 0;
  }

 private:
  T* ptr_ = nullptr;
  uint64_t cap_ = 0;
};

template <typename T>
using DeviceBuffer = Buffer<T, DeviceMemory>;
template <typename T>
using PinnedBuffer = Buffer<T, PinnedMemory>;

// Device temporaries of one call: alloc() returns NULL when the allocation fails, everything
// handed out is freed when the scope is left.
class TempScope {
 public:
  TempScope() = default;
  TempScope(const TempScope&) = delete;
  TempScope& operator=(const TempScope&) = delete;
  ~TempScope() {
    for (void* p : owned_) (void)hipFree(p);
  }
  template <typename T>
  T* alloc(uint64_t count) {
    void* p = nullptr;
    if (hipMalloc(&p, alloc_bytes<T>(count)) != hipSuccess) return nullptr;
    owned_.push_back(p);
    return static_cast<T*>(p);
  }

 private:
  std::vector<void*> owned_;
};

}  // namespace isl
