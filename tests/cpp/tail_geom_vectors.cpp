// CPU test (tests/test_accref_cpu.py): the geometry of the MSM's fix-up and bucket reduction
// (csrc/msm_plan.hpp) on cases read from a file, one line of decimal numbers out per line in.  No
// arithmetic of its own.
//   consts        -> RED_L FIX_FAN FIX_LEVELS FIX_WAVE_SPAN
//   tail half     -> L0 L1 g1 g nbits specs CH nch tree lg0 weight sum_n, then sum_sets' 8-way passes over sum_n
//   fix nchunks   -> n total len[1] .. len[n]
#include <cstdio>
#include <cstring>

#include "msm_plan.hpp"
using namespace tns;

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char op[16];
  while (std::fscanf(f, "%15s", op) == 1) {
    unsigned long long x;
    if (!std::strcmp(op, "consts")) {
      std::printf("%d %d %d %zu", RED_L, FIX_FAN, FIX_LEVELS, FIX_WAVE_SPAN);
    } else if (!std::strcmp(op, "tail") && std::fscanf(f, "%llu", &x) == 1) {
      const TailGeom t = tail_geom((size_t)x);
      int passes = 0;
      for (size_t n = t.sum_n; sum_sets_splits(n); n /= 8) passes++;
      std::printf("%d %d %zu %zu %d %d %d %zu %d %d %d %zu %d", t.L0, t.L1, t.g1, t.g, t.nbits, t.specs, t.CH, t.nch,
                  (int)t.tree, t.lg0, t.weight, t.sum_n, passes);
    } else if (!std::strcmp(op, "fix") && std::fscanf(f, "%llu", &x) == 1) {
      const FixLevelSizes s = fix_level_sizes((size_t)x);
      std::printf("%d %zu", s.n, s.total);
      for (int l = 1; l <= s.n; l++) std::printf(" %zu", s.len[l]);
    } else {
      std::fprintf(stderr, "bad line: %s\n", op);
      return 1;
    }
    std::putchar('\n');
  }
  std::fclose(f);
  return 0;
}
