// Host-only arithmetic of the entry-seed table (entry_seeds.hip): the ISL_ENTRY_SEEDS variable, the check
// of a caller's seed list, how one pick launch is cut into workgroups.  Plain C++ without a device header,
// so that tests/cpp/entry_seeds_host.cpp drives it under AddressSanitizer without a device.
#pragma once

#include <cstdint>

#include "../../include/islands_amd.h"

namespace isl_seeds {

// tile of the pick kernel: PQT queries x PST seeds per workgroup step, PDC elements of d per LDS chunk
constexpr uint32_t PQT = 32, PST = 32, PDC = 32;
constexpr uint32_t PLD = PDC + 4;  // LDS row pitch in floats: rows stay 16-byte aligned and the 16 rows a
                                   // wave reads with ds_read_b128 start 36 r (mod 64) banks apart -- 0, 36, 8,
                                   // 44, ... are the 16 multiples of 4, every bank once

// ISL_ENTRY_SEEDS: a decimal count.  NULL, "" and "0" mean none (*count = 0).  Anything that is not a
// decimal number is ISL_ERR_INVALID_ARGUMENT, a count above ISL_MAX_ENTRY_SEEDS is ISL_ERR_UNSUPPORTED
// (the statuses isl_index_select_entry_seeds gives); *count is 0 then.
inline isl_status parse_seed_env(const char* text, uint64_t* count) {
  *count = 0;
  if (!text || !*text) return ISL_OK;
  uint64_t v = 0;
  for (const char* c = text; *c; ++c) {
    if (*c < '0' || *c > '9') return ISL_ERR_INVALID_ARGUMENT;
    v = v * 10 + (uint64_t)(*c - '0');
    if (v > ISL_MAX_ENTRY_SEEDS) return ISL_ERR_UNSUPPORTED;  // (before v can wrap)
  }
  *count = v;
  return ISL_OK;
}

// A caller's seed list against an index of `len` nodes with `nvec` rows: ISL_OK, ISL_ERR_UNSUPPORTED for a
// list above the cap, ISL_ERR_INVALID_ARGUMENT for a NULL list with count > 0, ISL_ERR_NODE_NOT_FOUND with
// *bad = the first id that names no row.  Repeated ids are accepted.
inline isl_status check_seed_ids(const uint64_t* ids, uint64_t count, uint64_t len, uint64_t nvec, uint64_t* bad) {
  *bad = 0;
  if (count > ISL_MAX_ENTRY_SEEDS) return ISL_ERR_UNSUPPORTED;
  if (count && !ids) return ISL_ERR_INVALID_ARGUMENT;
  const uint64_t lim = len < nvec ? len : nvec;
  for (uint64_t i = 0; i < count; ++i)
    if (ids[i] >= lim) {
      *bad = ids[i];
      return ISL_ERR_NODE_NOT_FOUND;
    }
  return ISL_OK;
}

// One pick launch: grid.x = query tiles, grid.y = `splits` ranges of `tiles_per_split` seed tiles each.
// A query tile alone would leave most of the card idle at the batch sizes a search call has (1024 queries
// = 32 tiles on 256 CUs), so the seed table is cut until there are about two workgroups per CU; the
// ranges of one query meet in a packed 64-bit minimum.
struct PickGrid {
  uint32_t qtiles = 0, splits = 0, tiles_per_split = 0;
};
inline PickGrid pick_grid(uint64_t nq, uint64_t seeds, uint32_t cus) {
  PickGrid g;
  g.qtiles = (uint32_t)((nq + PQT - 1) / PQT);
  const uint32_t stiles = (uint32_t)((seeds + PST - 1) / PST);
  const uint32_t want = 2u * (cus ? cus : 1u);
  uint32_t splits = g.qtiles ? (want + g.qtiles - 1) / g.qtiles : 1u;
  if (splits > stiles) splits = stiles;
  if (splits < 1) splits = 1;
  g.tiles_per_split = (stiles + splits - 1) / splits;
  if (g.tiles_per_split < 1) g.tiles_per_split = 1;
  g.splits = (stiles + g.tiles_per_split - 1) / g.tiles_per_split;  // no empty range
  if (g.splits < 1) g.splits = 1;
  return g;
}

}  // namespace isl_seeds
