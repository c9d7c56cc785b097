// The LDS arithmetic of the graph builders' bf16 instantiations (islands_amd/csrc/build_plan.hpp) without a
// device or the library:
//   g++ -std=c++17 tests/cpp/build_lds_dump.cpp -o build_lds_dump
// stdin: triples "d nmax M".  stdout, per triple: "d nmax M query_floats_bf16 link_lds_bf16 select_lds_bf16".
// tests/test_build_bf16_cpu.py compares them with a restatement of the formula.
#include <cstdio>

#include "../../islands_amd/csrc/build_plan.hpp"

// the figures are constexpr: what the host reserves is what the kernels lay their lists out by
static_assert(isl_plan::query_floats_bf16(1) == 48 && isl_plan::query_floats_bf16(32) == 48 &&
              isl_plan::query_floats_bf16(33) == 80, "whole steps of 32 elements plus 16 of slack");
static_assert(isl_plan::select_lds_bf16(768, 129, 128) == isl_plan::link_lds_bf16(768) + 129 * 16 + 128 * 4,
              "four lists and a row behind the query");

int main() {
  unsigned d = 0, nmax = 0, M = 0;
  while (std::scanf("%u %u %u", &d, &nmax, &M) == 3)
    std::printf("%u %u %u %u %zu %zu\n", d, nmax, M, isl_plan::query_floats_bf16(d), isl_plan::link_lds_bf16(d),
                isl_plan::select_lds_bf16(d, nmax, M));
  return 0;
}
