// islands_amd/csrc/row_table.hpp on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: a row table
// with a capacity and the view a construction graph reads it through, over fake hipMalloc / hipFree as in
// row_table_host.cpp (malloc underneath, a count of live blocks).  A view frees nothing -- not when it is reset, moved,
// assigned over or destroyed -- and the table it was taken from frees its blocks exactly once (ASan reports a second
// free or a leak).  Built by `make -C islands_amd/csrc ../lib/asan/row_capacity_host`; stand-alone, no device is touched.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "../../islands_amd/csrc/row_table.hpp"

static int live = 0, frees = 0, failures = 0;
static size_t last_bytes[2] = {0, 0};

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
  last_bytes[0] = last_bytes[1];
  last_bytes[1] = bytes;
  *p = std::malloc(bytes);
  ++live;
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  if (p) { --live; ++frees; }
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

using isl::RowTable;

int main() {
  {  // a table nobody reserved: capacity == n
    RowTable t;
    EXPECT(t.capacity() == 0 && !t.reserved() && !t.borrowed());
    EXPECT(t.allocate(ISL_DTYPE_F32, 10, 13) == ISL_OK && t.capacity() == 10 && !t.reserved());
    EXPECT(t.block_bytes() == (10 * 16 + 256) * 4 && last_bytes[0] == t.block_bytes());
  }
  EXPECT(live == 0 && frees == 2);

  {  // block and norms for the capacity; the count moves inside it
    RowTable t;
    EXPECT(t.allocate(ISL_DTYPE_BF16, 300, 100, 512, true) == ISL_OK && live == 2);
    EXPECT(last_bytes[0] == (512 * 104 + 512) * 2 && last_bytes[1] == 512 * 4);
    EXPECT(t.n() == 300 && t.capacity() == 512 && t.reserved() && t.stride() == 104 && t.block_bytes() == last_bytes[0]);
    t.bf16()[512 * 104 + 511] = 1;  // (ASan: the block really has the capacity and the slack)
    t.norm2()[511] = 1.0f;
    t.set_n(512);
    EXPECT(t.n() == 512 && t.capacity() == 512);
    t.set_n(7);
    EXPECT(t.n() == 7 && t.capacity() == 512 && t.reserved());

    // a view: the same blocks, another count, nothing owned
    {
      RowTable v = RowTable::view_of(t, 400);
      EXPECT(v.borrowed() && v.data() == t.data() && v.norm2() == t.norm2() && v.n() == 400 && v.capacity() == 512);
      EXPECT(v.is_bf16() && v.d() == 100 && v.stride() == 104 && v.reserved() && live == 2);
      RowTable w(std::move(v));  // moved: still a view, the source empty
      EXPECT(w.borrowed() && w.data() == t.data() && !v.resident() && !v.borrowed() && v.capacity() == 0);
      RowTable x;
      EXPECT(x.allocate(ISL_DTYPE_F32, 2, 4) == ISL_OK && live == 4);
      x = std::move(w);  // assigned over an owning table: that one's blocks go, the view's do not
      EXPECT(x.borrowed() && x.data() == t.data() && live == 2 && frees == 4);
      RowTable y = RowTable::view_of(t, 8);
      x = std::move(y);  // assigned over a view: nothing is freed
      EXPECT(x.n() == 8 && live == 2 && frees == 4);
      x.reset();
      EXPECT(!x.resident() && !x.borrowed() && live == 2 && frees == 4);
      RowTable z = RowTable::view_of(t, 9);  // destroyed at the end of the scope
      EXPECT(z.borrowed());
    }
    EXPECT(live == 2 && frees == 4 && t.resident());
    t.bf16()[0] = 2;  // (ASan: the owner's block is still there)

    // a view that an owning table is assigned over lets go and then owns
    RowTable v = RowTable::view_of(t, 1);
    RowTable own;
    EXPECT(own.allocate(ISL_DTYPE_F32, 2, 4, 6, false) == ISL_OK && live == 4);
    v = std::move(own);
    EXPECT(!v.borrowed() && v.capacity() == 6 && v.n() == 2 && !v.reserved() && live == 4 && frees == 4);
  }
  EXPECT(live == 0 && frees == 8);

  if (failures) { std::printf("row capacity host: %d failures\n", failures); return 1; }
  std::printf("row capacity host: ok (%d frees)\n", frees);
  return 0;
}
