// The host definition of the row conversions (islands_amd/csrc/row_convert_plan.hpp) over arrays of f32 bit
// patterns, for tests/test_convert_rows_cpu.py: plain C++, no device.
//   row_convert_dump e4m3 <e> <in> <out>   u32 bit patterns -> u8 codes under exponent e
//   row_convert_dump bf16 <in> <out>       u32 bit patterns -> u16 bf16 bit patterns
//   row_convert_dump scale <in> <out>      u32 bit patterns of max|x| -> i32 automatic exponents
//   row_convert_dump plan                  chunks_per_row / grid_for over a few shapes, as text
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../islands_amd/csrc/row_convert_plan.hpp"

static std::vector<uint32_t> read_all(const char* path) {
  std::vector<uint32_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  v.resize((size_t)bytes / 4);
  if (!v.empty() && fread(v.data(), 4, v.size(), f) != v.size()) { fprintf(stderr, "short read\n"); exit(2); }
  fclose(f);
  return v;
}

template <typename T>
static void write_all(const char* path, const std::vector<T>& v) {
  FILE* f = fopen(path, "wb");
  if (!f) { perror(path); exit(2); }
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "short write\n"); exit(2); }
  fclose(f);
}

int main(int argc, char** argv) {
  using namespace isl_convert;
  if (argc == 5 && !strcmp(argv[1], "e4m3")) {
    const int32_t e = atoi(argv[2]);
    const std::vector<uint32_t> in = read_all(argv[3]);
    std::vector<uint8_t> out(in.size());
    for (size_t i = 0; i < in.size(); ++i) out[i] = narrow_e4m3(in[i], e);
    write_all(argv[4], out);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "bf16")) {
    const std::vector<uint32_t> in = read_all(argv[2]);
    std::vector<uint16_t> out(in.size());
    for (size_t i = 0; i < in.size(); ++i) out[i] = narrow_bf16(in[i]);
    write_all(argv[3], out);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "scale")) {
    const std::vector<uint32_t> in = read_all(argv[2]);
    std::vector<int32_t> out(in.size());
    for (size_t i = 0; i < in.size(); ++i) out[i] = scale_exp_for(in[i]);
    write_all(argv[3], out);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "plan")) {
    for (uint64_t d : {1ull, 15ull, 16ull, 17ull, 300ull, 768ull, 7680000000ull})
      printf("chunks %llu -> %llu\n", (unsigned long long)d, (unsigned long long)chunks_per_row(d));
    for (uint64_t items : {0ull, 1ull, 256ull, 257ull, 524288ull, 524289ull, 480000000ull})
      printf("grid %llu -> %u\n", (unsigned long long)items, grid_for(items, 256, 2048));
    printf("lane %u top %08x %08x %08x\n", kElemsPerLane, top_bits(-32), top_bits(0), top_bits(32));
    return 0;
  }
  fprintf(stderr, "usage: row_convert_dump e4m3 <e> <in> <out> | bf16 <in> <out> | scale <in> <out> | plan\n");
  return 2;
}
