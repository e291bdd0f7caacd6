// scbatchprobe.hip -- the batched sum-check's internal entry point (csrc/sumcheck_batch.hip:
// sumcheck_prove_batch) with forced limits, for tests/test_gpu_sumcheck_batch.py and
// tools/sumcheck_batch_bench.py: the C entry point calls the shipped function with the ScBatchLimits it
// is given and returns the results with what the call reports -- the route, the group rows, the
// groups and the round launches it queued.  Like provebatchprobe.hip nothing is re-implemented on the
// device: this file has no kernel, and libtns_scbatchprobe.so links libtns.so for every symbol it calls.
#include <hip/hip_runtime.h>

#include "abi.hpp"
#include "sumcheck.hpp"

namespace {
using namespace tns;
enum { I_ROUTE, I_GROUP_ROWS, I_GROUPS, I_LAUNCHES, I_COUNT };
}  // namespace

extern "C" {

int scbatchprobe_info_words() { return I_COUNT; }

// force_route: -1 the rule, 0 rows, 1 batched; ws_limit, crossover: 0 = the shipped default.
// resident: tables[j] are device pointers.  info: route, group rows, groups, launches.  Returns the
// call's status.
int scbatchprobe_prove(tns_ctx *ctx, const uint64_t *const *tables, int n_tables, unsigned nv, uint64_t batch,
                       const uint64_t *claimed_sums, const tns_term *terms, int n_terms,
                       tns_transcript *const *transcripts, int resident, int force_route, uint64_t ws_limit,
                       uint64_t crossover, uint64_t *rounds_out, uint64_t *finals_out, uint64_t *challenges_out,
                       int64_t *info) {
  if (!info || force_route < -1 || force_route > 1) return -1;
  ScBatchLimits lim;
  lim.force_route = force_route;
  if (ws_limit) lim.ws_bytes = (size_t)ws_limit;
  if (crossover) lim.crossover = (size_t)crossover;
  ScBatchReport r;
  const int st = sumcheck_prove_batch(ctx, tables, n_tables, nv, (size_t)batch, claimed_sums, terms, n_terms, transcripts,
                                      rounds_out, finals_out, challenges_out, resident != 0, lim, &r);
  info[I_ROUTE] = r.route;
  info[I_GROUP_ROWS] = (int64_t)r.group_rows;
  info[I_GROUPS] = (int64_t)r.groups;
  info[I_LAUNCHES] = (int64_t)r.launches;
  return st;
}

}  // extern "C"
