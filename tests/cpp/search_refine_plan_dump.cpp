// Prints the host-only arithmetic of islands_amd/csrc/search_refine_plan.hpp for the cases read from stdin, one
// command per line (tests/test_refine_cpu.py compares with a Python restatement; g++ alone, no device header):
//   geo d pitch nq c
//     -> geo <padded d> <lds bytes> <grid> <passes> <rank compares per lane> <scratch ids> <dist> <count> <bytes>
//   set null_idx is_hnsw on_device has_dimension len dimension rows_null n d dtype mem placement
//     -> set <status> <why> <drops>
//   ref null_idx is_hnsw recompute table_rows table_d buffers_null nq d k candidates ef
//     -> ref <status> <why>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../islands_amd/csrc/search_refine_plan.hpp"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    std::vector<long long> v;
    for (long long x; in >> x;) v.push_back(x);
    if (cmd == "geo" && v.size() == 4) {
      const uint64_t d = v[0], pitch = v[1], nq = v[2], c = v[3];
      const isl_refine::Scratch s = isl_refine::scratch_elems(nq, pitch);
      printf("geo %u %llu %u %u %llu %llu %llu %llu %llu\n", isl_refine::padded_dim(d),
             (unsigned long long)isl_refine::lds_bytes(d, pitch), isl_refine::grid(nq), isl_refine::passes(c),
             (unsigned long long)isl_refine::rank_compares_per_lane(c), (unsigned long long)s.ids,
             (unsigned long long)s.dist, (unsigned long long)s.count,
             (unsigned long long)isl_refine::scratch_bytes(nq, pitch));
    } else if (cmd == "set" && v.size() == 12) {
      isl_refine::Handle h{};
      h.null_idx = v[0]; h.is_hnsw = v[1]; h.on_device = v[2]; h.has_dimension = v[3];
      h.len = v[4]; h.dimension = v[5];
      bool drops = false;
      const isl_refine::Verdict r = isl_refine::check_set_rows(h, v[6] != 0, v[7], v[8], (int32_t)v[9], (int32_t)v[10],
                                                                (int32_t)v[11], &drops);
      printf("set %d %d %d\n", (int)r.status, (int)r.why, (int)drops);
    } else if (cmd == "ref" && v.size() == 11) {
      isl_refine::Handle h{};
      h.null_idx = v[0]; h.is_hnsw = v[1]; h.recompute = v[2]; h.table_rows = v[3]; h.table_d = v[4];
      h.on_device = true;
      const isl_refine::Verdict r = isl_refine::check_refined(h, v[5] != 0, v[6], v[7], v[8], v[9], v[10]);
      printf("ref %d %d\n", (int)r.status, (int)r.why);
    } else {
      fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
