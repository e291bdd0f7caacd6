// prove_batch_plan.hpp -- how a batch of Twist or Shout proofs over one SRS runs (prove_batch.hip:
// tns_twist_prove_batch, tns_shout_prove_batch and their _device forms): the batched route -- every
// proof's tables, commitments, folds and openings in passes whose launch count does not depend on
// the batch -- or the single prover in a loop over the rows.
// Host arithmetic alone (plain C++17, no HIP), like msm_batch_plan.hpp: tests/test_prove_batch_plan_cpu.py.
#pragma once
#include "msm_batch_plan.hpp"

namespace tns {

// One call's shape.  Twist: n_wide = n_narrow = N = next_pow2(n_ops) (values and addresses).
// Shout: n_wide = T = next_pow2(n_entries) (the table), n_narrow = M = next_pow2(n_lookups) (the
// indices).  The sum-check has log2(n_narrow) rounds.
struct ProveBatchShape {
  size_t batch = 0;
  size_t n_wide = 0, n_narrow = 0;
  bool whole_srs = true;                         // not a shard
  bool basis_wide = true, basis_narrow = true;   // a Lagrange basis of that many nodes exists or can be built
};

struct ProveBatchPlan {
  int route = BATCH_ROUTE_ROWS;
  // the commitment of the `batch` full-width rows (plan_batch at 254 bits): rows of every group but
  // the last, and the groups; on the rows route 1 and batch
  size_t group_rows = 1, groups = 0;
  // the openings: Twist, and Shout with T == M, open 2 batch rows of n_wide nodes in one call with
  // two rows a point (open_calls = 1, rows_per_point = 2); Shout with T != M opens the batch table
  // rows and the batch index rows in a call each (open_calls = 2, rows_per_point = 1).  The groups
  // are those of the (first) call's full-width quotient rows.
  int open_calls = 0, rows_per_point = 0;
  size_t open_rows = 0, open_group_rows = 1, open_groups = 0;
};

// The batched route is taken when batch >= 2 (a forced route: batch >= 1), there are openings
// (n_narrow >= 2: at least one sum-check round), the SRS is whole, both node counts have a basis,
// and plan_batch takes the batched route for the full-width rows of the commitment and of every
// opening call.  Otherwise: the single prover, row by row.
inline ProveBatchPlan plan_prove_batch(const ProveBatchShape &s, const BatchLimits &lim = BatchLimits()) {
  ProveBatchPlan P;
  P.groups = s.batch;
  P.open_groups = 0;
  if (s.batch == 0 || s.n_wide == 0 || s.n_narrow < 2 || !s.whole_srs || !s.basis_wide || !s.basis_narrow) return P;
  if (lim.force_route == BATCH_ROUTE_ROWS || (lim.force_route < 0 && s.batch < 2)) return P;
  const BatchPlan C = plan_batch(s.n_wide, s.batch, 254, true, lim);
  if (C.route != BATCH_ROUTE_BATCHED) return P;
  const bool one_call = s.n_wide == s.n_narrow;
  const size_t open_rows = one_call ? 2 * s.batch : s.batch;
  const BatchPlan O = plan_batch(s.n_wide, open_rows, 254, true, lim);
  if (O.route != BATCH_ROUTE_BATCHED) return P;
  if (!one_call && plan_batch(s.n_narrow, s.batch, 254, true, lim).route != BATCH_ROUTE_BATCHED) return P;
  P.route = BATCH_ROUTE_BATCHED;
  P.group_rows = C.group_rows;
  P.groups = C.groups;
  P.open_calls = one_call ? 1 : 2;
  P.rows_per_point = one_call ? 2 : 1;
  P.open_rows = open_rows;
  P.open_group_rows = O.group_rows;
  P.open_groups = O.groups;
  return P;
}

}  // namespace tns
