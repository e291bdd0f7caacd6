// sumcheck_batch_plan_vectors.cpp -- csrc/sumcheck_batch_plan.hpp from the headers alone, for
// tests/test_sumcheck_batch_plan_cpu.py: one line of numbers per case read from the file named on
// the command line.
//   plan batch nv n_tables table_terms ws crossover force
//       (ws / crossover 0: the default; force -1: the rule)
//     -> route group_rows groups
#include <cstdio>
#include <cstring>

#include "sumcheck_batch_plan.hpp"

using namespace tns;

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char op[32];
  while (std::fscanf(f, "%31s", op) == 1) {
    if (std::strcmp(op, "plan")) return 4;
    ScBatchShape s;
    size_t ws, crossover;
    int tt, force;
    if (std::fscanf(f, "%zu %u %d %d %zu %zu %d", &s.batch, &s.nv, &s.n_tables, &tt, &ws, &crossover, &force) != 7)
      return 3;
    s.table_terms = tt != 0;
    ScBatchLimits lim;
    if (ws) lim.ws_bytes = ws;
    if (crossover) lim.crossover = crossover;
    lim.force_route = force;
    // (all defaults: the call as the entry points make it)
    const ScBatchPlan P = ws || crossover || force >= 0 ? plan_sumcheck_batch(s, lim) : plan_sumcheck_batch(s);
    std::printf("%d %zu %zu\n", P.route, P.group_rows, P.groups);
  }
  std::fclose(f);
  return 0;
}
