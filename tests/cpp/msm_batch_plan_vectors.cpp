// msm_batch_plan_vectors.cpp -- csrc/msm_batch_plan.hpp (and the batch members of msm_plan.hpp)
// from the headers alone, for tests/test_msm_batch_plan_cpu.py: one line of numbers per case read
// from the file named on the command line.
//   consts                                   -> entry limit, key bits, workspace cap, max scalars, crossover
//   plan n rows bits basis entries ws crossover force
//       (entries / ws / crossover 0: the default; force -1: the rule)
//                                            -> route c W rows n_row Wr bucket_bits nb group_rows groups ws_bytes
//   group n g bits                           -> c W rows n_row Wr bucket_bits nb half shared stride
//   one n bits                               -> the same of plan_msm without a table
//   fits n g c W entries ws                  -> 0 / 1
//   geom n_row rows c W                      -> E keybits npass ibits ct spb T1 pk vo
#include <cstdio>
#include <cstring>

#include "msm_batch_plan.hpp"

using namespace tns;

static void print_plan(const MsmPlan &P) {
  std::printf("%d %d %u %zu %d %d %zu %zu %d %u\n", P.c, P.W, P.rows, P.n_row, P.Wr, P.bucket_bits, P.nb, P.half,
              P.shared ? 1 : 0, P.stride);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char op[32];
  while (std::fscanf(f, "%31s", op) == 1) {
    if (!std::strcmp(op, "consts")) {
      std::printf("%zu %d %zu %zu %zu\n", BATCH_ENTRY_LIMIT, BATCH_KEY_BITS, BATCH_WS_CAP, BATCH_MAX_SCALARS,
                  BATCH_CROSSOVER);
    } else if (!std::strcmp(op, "plan")) {
      size_t n, rows, entries, ws, crossover;
      int bits, basis, force;
      if (std::fscanf(f, "%zu %zu %d %d %zu %zu %zu %d", &n, &rows, &bits, &basis, &entries, &ws, &crossover, &force) != 8)
        return 3;
      BatchLimits lim;
      if (entries) lim.entries = entries;
      if (ws) lim.ws_bytes = ws;
      if (crossover) lim.crossover = crossover;
      lim.force_route = force;
      // (all defaults: the call as the entry points make it)
      const BatchPlan B = entries || ws || crossover || force >= 0 ? plan_batch(n, rows, bits, basis != 0, lim)
                                                                   : plan_batch(n, rows, bits, basis != 0);
      std::printf("%d %d %d %u %zu %d %d %zu %zu %zu %zu\n", B.route, B.P.c, B.P.W, B.P.rows, B.P.n_row, B.P.Wr,
                  B.P.bucket_bits, B.P.nb, B.group_rows, B.groups, B.ws_bytes);
    } else if (!std::strcmp(op, "group")) {
      size_t n, g;
      int bits;
      if (std::fscanf(f, "%zu %zu %d", &n, &g, &bits) != 3) return 3;
      print_plan(plan_batch_group(n, g, bits));
    } else if (!std::strcmp(op, "one")) {
      size_t n;
      int bits;
      if (std::fscanf(f, "%zu %d", &n, &bits) != 2) return 3;
      print_plan(plan_msm(n, bits, TableShape(), 0, false));
    } else if (!std::strcmp(op, "fits")) {
      size_t n, g, entries, ws;
      int c, W;
      if (std::fscanf(f, "%zu %zu %d %d %zu %zu", &n, &g, &c, &W, &entries, &ws) != 6) return 3;
      BatchLimits lim;
      lim.entries = entries;
      lim.ws_bytes = ws;
      std::printf("%d\n", batch_group_fits(n, g, c, W, lim) ? 1 : 0);
    } else if (!std::strcmp(op, "geom")) {
      size_t n_row, rows;
      int c, W;
      if (std::fscanf(f, "%zu %zu %d %d", &n_row, &rows, &c, &W) != 4) return 3;
      WindowPlan P;
      P.c = c;
      P.W = W;
      P.rows = (uint32_t)rows;
      P.n_row = rows > 1 ? n_row : 0;
      P.bucket_bits = ceil_log2_sz(rows * (size_t)W) + c - 1;
      const SortGeom g = sort_geom(rows * n_row, P);
      std::printf("%zu %d %d %d %d %zu %zu %d %d\n", g.E, g.keybits, g.npass, g.ibits, g.ct, g.spb, g.T1, g.pk ? 1 : 0,
                  g.vo ? 1 : 0);
    } else {
      return 4;
    }
  }
  std::fclose(f);
  return 0;
}
