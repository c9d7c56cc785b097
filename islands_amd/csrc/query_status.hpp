// Per-query status words written by the search kernels and read back by the host.  Plain C++ without a
// device header: the kernels (search_kernels.hip.h) and the host-only round planner of the recompute
// provider (recompute_plan.hpp) share it.
#pragma once

#include <cstdint>

enum : uint32_t {
  QS_OK = 0,
  QS_NODE_NOT_FOUND = 5,
  QS_REDO = 0x100,     // fast kernel gave up -> exact kernel
  QS_SCRATCH = 0x101,  // exact kernel ran out of candidate scratch
  QS_REPLAY = 0x102,   // result-heap order needed: replay kernel re-orders from the push log
  QS_BLOCKED = 0x103,  // recompute provider: a needed row is not materialised yet (ids reported)
  QS_BLOCKED_X = 0x104 // ... and the query is parked in the heap-exact kernel (it keeps its pool slot)
};
