// Prints the NTT pass plans of csrc/fft_plan.hpp (test infrastructure, host
// code only): a first line "tile_log=T elems_log=E", then for every m = 0..28
// and every stage cap S = 1..T one line
//   m=<m> S=<S> passes=<a>:<log_ns>:<log_c> ...
// and, for the knob parser, one line "knob <value>=<cap>" per argument.
// Compiled and read by tests/test_fft_cpu.py.
#include <cstdio>
#include <cstdlib>

#include "fft_plan.hpp"

int main(int argc, char** argv) {
  printf("tile_log=%u elems_log=%u max_log=%u\n", zkh::kFftTileLog, zkh::kFftTileElemsLog, zkh::kFftMaxLog);
  for (int i = 1; i < argc; ++i) printf("knob %s=%u\n", argv[i], zkh::fft_stage_cap(strtol(argv[i], nullptr, 0)));
  for (uint32_t m = 0; m <= zkh::kFftMaxLog; ++m)
    for (uint32_t S = 1; S <= zkh::kFftTileLog; ++S) {
      printf("m=%u S=%u passes=", m, S);
      for (const auto& q : zkh::fft_plan(m, S)) printf(" %u:%u:%u", q.a, q.log_ns, q.log_c);
      printf("\n");
    }
  return 0;
}
