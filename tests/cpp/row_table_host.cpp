// islands_amd/csrc/row_table.hpp on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: the
// owning row table and the entry-seed group over fake hipMalloc / hipFree as in device_buffer_host.cpp (malloc
// underneath, a count of live blocks, a "fail the N-th allocation" switch) that also record the order of the
// calls.  Nothing leaks, nothing is freed twice (ASan reports either), a moved-from table is empty.
// Built by `make -C islands_amd/csrc ../lib/asan/row_table_host`; stand-alone, no device is touched.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>

#include "../../islands_amd/csrc/row_table.hpp"

static int live = 0;       // blocks handed out and not yet freed
static int allocs = 0;     // allocation calls so far
static int frees = 0;      // blocks freed so far
static int fail_at = 0;    // the allocation call with this number fails (0 = none)
static std::string order;  // 'a' per allocation asked for, 'f' per block freed
static size_t last_bytes[2] = {0, 0};  // what the last two allocations asked for, oldest first
static int failures = 0;

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
  order += 'a';
  last_bytes[0] = last_bytes[1];
  last_bytes[1] = bytes;
  if (++allocs == fail_at) { *p = nullptr; return hipErrorOutOfMemory; }
  *p = std::malloc(bytes);
  ++live;
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  if (p) { --live; ++frees; order += 'f'; }
  std::free(p);
  return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return hipMalloc(p, bytes); }
hipError_t hipHostFree(void* p) { return hipFree(p); }
}

namespace isl {
isl_status fail(isl_status st, const char*, ...) { return st; }
}  // namespace isl

#define EXPECT(cond)                                                                        \
  do {                                                                                      \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)

using isl::EntrySeeds;
using isl::RowTable;

static bool empty(const RowTable& t) {
  return !t.resident() && t.data() == nullptr && t.f32() == nullptr && t.bf16() == nullptr && t.norm2() == nullptr &&
         t.n() == 0 && t.d() == 0 && t.stride() == 0 && t.dtype() == ISL_DTYPE_F32 && !t.is_bf16();
}

int main() {
  {  // allocate: sizes from the plan header, typed accessors follow the dtype
    RowTable t;
    EXPECT(empty(t));
    EXPECT(t.allocate(ISL_DTYPE_F32, 10, 13) == ISL_OK && live == 2);
    EXPECT(last_bytes[0] == (10 * 16 + 256) * 4 && last_bytes[1] == 10 * 4);
    EXPECT(t.resident() && !t.is_bf16() && t.n() == 10 && t.d() == 13 && t.stride() == 16);
    EXPECT(t.f32() == t.data() && t.bf16() == nullptr && t.norm2() != nullptr);
    t.f32()[10 * 16 + 255] = 1.0f;  // (ASan: the block really has the slack)
    t.norm2()[9] = 1.0f;
    int seen = 0;
    t.with_row_type([&](auto row) { seen = (int)sizeof(row); });
    EXPECT(seen == 4);

    // move-construct and move-assign: the source is empty, nothing is freed or copied
    float* block = t.f32();
    RowTable m(std::move(t));
    EXPECT(empty(t) && m.f32() == block && m.n() == 10 && m.d() == 13 && m.stride() == 16 && live == 2 && frees == 0);
    RowTable a;
    EXPECT(a.allocate(ISL_DTYPE_BF16, 3, 5) == ISL_OK && live == 4);
    a = std::move(m);  // the destination's blocks go
    EXPECT(empty(m) && a.f32() == block && !a.is_bf16() && a.n() == 10 && live == 2 && frees == 2);
    RowTable& self = a;
    a = std::move(self);  // (self-assignment keeps the table)
    EXPECT(a.f32() == block && a.n() == 10 && live == 2);

    // reset frees every block exactly once
    a.reset();
    EXPECT(empty(a) && live == 0 && frees == 4);
    a.reset();  // (idempotent)
    EXPECT(frees == 4);
  }
  EXPECT(live == 0 && frees == 4);

  {  // a dtype set on a table without a block
    RowTable t;
    t.set_dtype(ISL_DTYPE_BF16);
    EXPECT(t.is_bf16() && !t.resident() && t.data() == nullptr && t.bf16() == nullptr && t.n() == 0);
    int seen = 0;
    t.with_row_type([&](auto row) { seen = (int)sizeof(row); });
    EXPECT(seen == 2 && live == 0);
    const int before = allocs;
    t.reset();
    EXPECT(empty(t) && allocs == before && frees == 4);
  }
  EXPECT(live == 0 && frees == 4);

  {  // re-allocating with the other dtype: the first table is freed before the second is asked for
    RowTable t;
    EXPECT(t.allocate(ISL_DTYPE_F32, 4, 8) == ISL_OK);
    order.clear();
    EXPECT(t.allocate(ISL_DTYPE_BF16, 7, 13) == ISL_OK);
    EXPECT(order == "ffaa" && live == 2);
    EXPECT(last_bytes[0] == (7 * 16 + 512) * 2 && last_bytes[1] == 7 * 4);
    EXPECT(t.is_bf16() && t.bf16() == t.data() && t.f32() == nullptr && t.n() == 7 && t.d() == 13 && t.stride() == 16);
    t.bf16()[7 * 16 + 511] = 1;

    // a failing allocation (the block, then the norms) leaves an empty table and no block behind
    for (int which : {1, 2}) {
      fail_at = allocs + which;
      EXPECT(t.allocate(ISL_DTYPE_F32, 4, 8) == ISL_ERR_DEVICE);
      EXPECT(empty(t) && live == 0);
      fail_at = 0;
      EXPECT(t.allocate(ISL_DTYPE_F32, 4, 8) == ISL_OK && live == 2);
    }
  }
  EXPECT(live == 0);

  {  // entry seeds: moved into place, dropped by assignment, reset after a move
    EntrySeeds s;
    EXPECT(s.count() == 0);
    EXPECT(s.d_ids.reserve(3) == ISL_OK && s.rows.allocate(ISL_DTYPE_BF16, 3, 5) == ISL_OK && live == 3);
    s.ids = {0, 7, 19};
    EXPECT(s.count() == 3);
    EntrySeeds held;
    held = std::move(s);
    EXPECT(held.count() == 3 && held.ids.size() == 3 && held.rows.is_bf16() && live == 3);
    EXPECT(s.count() == 0 && s.ids.empty() && s.d_ids.get() == nullptr && empty(s.rows));
    const int before = frees;
    s = {};  // the moved-from group owns nothing
    s.rows.reset();
    EXPECT(frees == before && live == 3);
    held = {};
    EXPECT(held.count() == 0 && held.ids.empty() && held.d_ids.get() == nullptr && empty(held.rows));
    EXPECT(frees == before + 3 && live == 0);
  }
  EXPECT(live == 0);

  if (failures) { std::printf("row table host: %d failures\n", failures); return 1; }
  std::printf("row table host: ok (%d allocations, %d frees)\n", allocs, frees);
  return 0;
}
