// prove_batch_plan_vectors.cpp -- csrc/prove_batch_plan.hpp from the headers alone, for
// tests/test_prove_batch_plan_cpu.py: one line of numbers per case read from the file named on the
// command line.
//   plan batch n_wide n_narrow whole basis_wide basis_narrow entries ws crossover force
//       (entries / ws / crossover 0: the default; force -1: the rule)
//     -> route group_rows groups open_calls rows_per_point open_rows open_group_rows open_groups
#include <cstdio>
#include <cstring>

#include "prove_batch_plan.hpp"

using namespace tns;

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char op[32];
  while (std::fscanf(f, "%31s", op) == 1) {
    if (std::strcmp(op, "plan")) return 4;
    ProveBatchShape s;
    size_t entries, ws, crossover;
    int whole, bw, bn, force;
    if (std::fscanf(f, "%zu %zu %zu %d %d %d %zu %zu %zu %d", &s.batch, &s.n_wide, &s.n_narrow, &whole, &bw, &bn,
                    &entries, &ws, &crossover, &force) != 10)
      return 3;
    s.whole_srs = whole != 0;
    s.basis_wide = bw != 0;
    s.basis_narrow = bn != 0;
    BatchLimits lim;
    if (entries) lim.entries = entries;
    if (ws) lim.ws_bytes = ws;
    if (crossover) lim.crossover = crossover;
    lim.force_route = force;
    // (all defaults: the call as the entry points make it)
    const ProveBatchPlan P = entries || ws || crossover || force >= 0 ? plan_prove_batch(s, lim) : plan_prove_batch(s);
    std::printf("%d %zu %zu %d %d %zu %zu %zu\n", P.route, P.group_rows, P.groups, P.open_calls, P.rows_per_point,
                P.open_rows, P.open_group_rows, P.open_groups);
  }
  std::fclose(f);
  return 0;
}
