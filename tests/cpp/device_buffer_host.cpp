// islands_amd/csrc/device_buffer.hpp on the host, under AddressSanitizer: the owning buffers and the
// scope of one-call temporaries over fake hipMalloc / hipFree / hipHostMalloc / hipHostFree (malloc
// underneath, a count of live blocks, a "fail the N-th allocation" switch).  Allocation failures are
// not provoked on a device, so the failure paths are pinned here: nothing leaks, nothing is freed
// twice (ASan reports either), a failed reserve leaves an empty buffer.
// Built by `make -C islands_amd/csrc asan`; stand-alone, no device is touched.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "../../islands_amd/csrc/device_buffer.hpp"

static int live = 0;             // blocks handed out and not yet freed
static int allocs = 0;           // allocation calls so far (device and pinned together)
static int fail_at = 0;          // the allocation call with this number fails (0 = none)
static int live_at_alloc = 0;    // `live` when the last allocation was asked for
static size_t last_bytes = 0;    // what it asked for
static int failures = 0;

static hipError_t fake_alloc(void** p, size_t bytes) {
  live_at_alloc = live;
  last_bytes = bytes;
  if (++allocs == fail_at) { *p = nullptr; return hipErrorOutOfMemory; }
  *p = std::malloc(bytes);
  ++live;
  return hipSuccess;
}
static hipError_t fake_free(void* p) {
  if (p) --live;
  std::free(p);
  return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return fake_alloc(p, bytes); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return fake_alloc(p, bytes); }
hipError_t hipFree(void* p) { return fake_free(p); }
hipError_t hipHostFree(void* p) { return fake_free(p); }
}

namespace isl {
isl_status fail(isl_status st, const char*, ...) { return st; }
}  // namespace isl

#define EXPECT(cond)                                                                        \
  do {                                                                                      \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)

using isl::DeviceBuffer;
using isl::PinnedBuffer;

struct Group {  // how SearchWorkspace and ExactPool hold their arrays
  DeviceBuffer<float> a;
  DeviceBuffer<uint64_t> b;
  PinnedBuffer<uint32_t> h;
};

int main() {
  uint64_t events = 0;
  {  // reserve: within capacity, above it, zero elements
    DeviceBuffer<uint32_t> b;
    EXPECT(b.get() == nullptr && b.capacity() == 0);
    EXPECT(b.reserve(100, &events) == ISL_OK && events == 1 && b.capacity() == 100 && last_bytes == 400);
    uint32_t* p = b;
    p[99] = 7;  // (ASan: the block really has 100 elements)
    EXPECT(b.reserve(100, &events) == ISL_OK && b.reserve(10, &events) == ISL_OK);
    EXPECT(events == 1 && b.get() == p && b.capacity() == 100 && live == 1);
    EXPECT(b.reserve(101, &events) == ISL_OK && events == 2 && b.capacity() == 101 && last_bytes == 404);
    EXPECT(live_at_alloc == 0 && live == 1);  // the old block went first
    DeviceBuffer<uint16_t> z;
    EXPECT(z.reserve(0, &events) == ISL_OK && events == 3 && last_bytes == 4 && z.get() != nullptr && live == 2);
    EXPECT(z.reserve(1) == ISL_OK && last_bytes == 4 && events == 3);  // no counter handed in
  }
  EXPECT(live == 0);

  {  // a failing reserve
    PinnedBuffer<float> b;
    EXPECT(b.reserve(8, &events) == ISL_OK && live == 1);
    const uint64_t before = events;
    fail_at = allocs + 1;
    EXPECT(b.reserve(16, &events) == ISL_ERR_DEVICE);
    EXPECT(b.get() == nullptr && b.capacity() == 0 && events == before && live == 0);
    EXPECT(b.reserve(16, &events) == ISL_OK && events == before + 1 && b.capacity() == 16 && live == 1);
  }
  EXPECT(live == 0);

  {  // moves leave the source empty; the destination's old block is freed
    DeviceBuffer<float> a, c;
    EXPECT(a.reserve(4) == ISL_OK && c.reserve(6) == ISL_OK && live == 2);
    float* pa = a;
    DeviceBuffer<float> m(std::move(a));
    EXPECT(a.get() == nullptr && a.capacity() == 0 && m.get() == pa && m.capacity() == 4 && live == 2);
    c = std::move(m);
    EXPECT(m.get() == nullptr && m.capacity() == 0 && c.get() == pa && c.capacity() == 4 && live == 1);
  }
  EXPECT(live == 0);

  {  // release() then adopt() on another buffer: freed once
    DeviceBuffer<uint64_t> a, b;
    EXPECT(a.reserve(3) == ISL_OK && b.reserve(5) == ISL_OK && live == 2);
    uint64_t* raw = a.release();
    EXPECT(a.get() == nullptr && a.capacity() == 0 && live == 2);
    b.adopt(raw, 3);
    EXPECT(b.get() == raw && b.capacity() == 3 && live == 1);
    b.reset();
    EXPECT(b.get() == nullptr && live == 0);
    b.reset();  // (idempotent)
  }
  EXPECT(live == 0);

  for (int failing : {3, 0}) {  // a scope of five temporaries, the third allocation failing / none
    int got = 0;
    {
      isl::TempScope tmp;
      fail_at = failing ? allocs + failing : 0;
      for (int i = 0; i < 5; ++i) got += tmp.alloc<float>(16 + i) != nullptr;
      EXPECT(live == got);
    }
    EXPECT(got == (failing ? 4 : 5) && live == 0);
  }
  {
    isl::TempScope tmp;
    EXPECT(tmp.alloc<uint16_t>(0) != nullptr && last_bytes == 4);
    uint16_t* p = tmp.alloc<uint16_t>(3);
    EXPECT(p != nullptr && last_bytes == 6);
    p[2] = 1;
  }
  EXPECT(live == 0);

  {  // a struct of buffers reset by assigning a default-constructed one
    Group g;
    EXPECT(g.a.reserve(10) == ISL_OK && g.b.reserve(10) == ISL_OK && g.h.reserve(10) == ISL_OK && live == 3);
    g = Group{};
    EXPECT(live == 0 && g.a.get() == nullptr && g.b.capacity() == 0 && g.h.get() == nullptr);
    EXPECT(g.h.reserve(2) == ISL_OK && live == 1);
  }
  EXPECT(live == 0);

  if (failures) { std::printf("device buffer host: %d failures\n", failures); return 1; }
  std::printf("device buffer host: ok (%d allocations)\n", allocs);
  return 0;
}
