// sumcheck_batch_plan.hpp -- how a batch of generic sum-checks of one shape runs (sumcheck_batch.hip:
// tns_sumcheck_prove_batch and its _device form): the batched route -- every instance's round in
// one launch, nv + 1 launches a group whatever the batch -- or the single prover in a loop over the
// rows.
// Host arithmetic alone (plain C++17, no HIP), like prove_batch_plan.hpp:
// tests/test_sumcheck_batch_plan_cpu.py.
#pragma once
#include "msm_batch_plan.hpp"

namespace tns {

// Instances of at least this many entries (2^nv) take the row route.  Measured
// (profiles/sumcheck_batch_bench.json), 3-table Twist-shaped composition on
// resident tables, 16 instances, nv = 8, 10, .. 22: batched was faster than the loop at every one
// of them -- 4.2x at 2^8, 5.8x at 2^16, 2.4x at 2^20, 1.36x at 2^22 -- so the measured grid holds no
// size at which batched is not faster.  2^24, the next size of the grid, was not measured (16
// instances of 3 tables are 24 GiB of input, and one such instance's scratch is already above
// BATCH_WS_CAP, so it could only run row by row): the rule keeps the loop from there on, the
// smallest size for which no measurement says otherwise.
#ifndef TNS_SC_BATCH_CROSSOVER
#define TNS_SC_BATCH_CROSSOVER ((size_t)1 << 24)
#endif
constexpr size_t SC_BATCH_CROSSOVER = TNS_SC_BATCH_CROSSOVER;

// One call's shape: `batch` instances of n_tables tables of 2^nv entries under one composition.
struct ScBatchShape {
  size_t batch = 0;
  unsigned nv = 0;
  int n_tables = 0;
  bool table_terms = false;  // some term has a table factor (else the transcript alone proves it)
};

// the limits as arguments (defaults: the real ones) so that tests and the probe can force a route
// or a split with small numbers.  The workspace cap is BATCH_WS_CAP: the fold scratch lives in the
// context's sum-check workspaces, which keep their high-water mark for the context's life exactly
// as the batched MSM's do, so the same bound on what one call may leave behind applies.
struct ScBatchLimits {
  size_t crossover = SC_BATCH_CROSSOVER;  // entries an instance
  size_t ws_bytes = BATCH_WS_CAP;
  int force_route = -1;  // BATCH_ROUTE_*: taken whenever it is possible at all
};

struct ScBatchPlan {
  int route = BATCH_ROUTE_ROWS;
  size_t group_rows = 1;  // instances of every group but the last; on the rows route 1
  size_t groups = 0;      // the groups cover the instances in order; on the rows route batch
};

// Fold scratch of `rows` instances: every table folded once (2^(nv-1) entries, ping) and twice
// (2^(nv-2), pong), 32 bytes an entry.  nv >= 1.
inline size_t sc_batch_ws_bytes(int n_tables, size_t rows, unsigned nv) {
  const size_t n = (size_t)1 << nv;
  return (size_t)32 * (size_t)n_tables * rows * (n / 2 + n / 4);
}

// Batched when batch >= 2 (a forced route: >= 1), nv >= 1, some term has a table factor, 2^nv is
// below the crossover (a forced route: any) and one instance's scratch fits the cap; the groups are
// the largest row counts whose scratch stays under the cap and run one after another.  Otherwise:
// the single prover, row by row.
inline ScBatchPlan plan_sumcheck_batch(const ScBatchShape &s, const ScBatchLimits &lim = ScBatchLimits()) {
  ScBatchPlan P;
  P.groups = s.batch;
  if (s.batch == 0 || s.nv == 0 || s.nv >= 8 * sizeof(size_t) - 8 || s.n_tables < 1 || !s.table_terms) return P;
  bool batched = s.batch >= 2 && ((size_t)1 << s.nv) < lim.crossover;
  if (lim.force_route >= 0) batched = lim.force_route == BATCH_ROUTE_BATCHED;
  if (!batched) return P;
  const size_t one = sc_batch_ws_bytes(s.n_tables, 1, s.nv);
  if (one > lim.ws_bytes) return P;
  const size_t g = lim.ws_bytes / one;  // (the scratch is linear in the rows)
  P.route = BATCH_ROUTE_BATCHED;
  P.group_rows = g < s.batch ? g : s.batch;
  P.groups = (s.batch + P.group_rows - 1) / P.group_rows;
  return P;
}

}  // namespace tns
