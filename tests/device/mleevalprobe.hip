// mleevalprobe.hip -- the one-pass MLE evaluation's internal entry points (csrc/mle_eval.hip:
// mle_evaluate_batch; csrc/sumcheck_verify.hip: sumcheck_verify_batch) with forced launch limits, for
// tests/test_gpu_mle_evaluate_batch.py, tests/test_gpu_sumcheck_verify_batch.py and
// tools/mle_eval_bench.py: the C entry points call the shipped functions with the MleEvalLimits they
// are given and return the results with what the call reports -- the regime, the launches, the
// blocks of the dot-product launch and the rows a thread took.  mleevalprobe_fold_chain runs the
// earlier route, mle_evaluate_dev's fold chain (csrc/mle.hip), once per (instance, table) on
// resident tables: the benchmark's baseline, nothing else calls it.  Like scbatchprobe.hip nothing
// is re-implemented on the device: this file has no kernel, and libtns_mleevalprobe.so links
// libtns.so for every symbol it calls.
#include <hip/hip_runtime.h>

#include "abi.hpp"
#include "sumcheck.hpp"

namespace {
using namespace tns;
enum { I_REGIME, I_LAUNCHES, I_BLOCKS, I_ROWS, I_COUNT };

MleEvalLimits limits(uint64_t min_blocks, int max_log_rows) {
  MleEvalLimits lim;
  if (min_blocks) lim.min_blocks = (size_t)min_blocks;
  if (max_log_rows >= 0) lim.max_log_rows = (unsigned)max_log_rows;
  return lim;
}
void fill(const MleEvalReport &r, int64_t *info) {
  info[I_REGIME] = r.regime;
  info[I_LAUNCHES] = (int64_t)r.launches;
  info[I_BLOCKS] = (int64_t)r.blocks;
  info[I_ROWS] = (int64_t)r.rows_per_thread;
}
}  // namespace

extern "C" {

int mleevalprobe_info_words() { return I_COUNT; }

// min_blocks: 0 = the shipped default; max_log_rows: -1 = the shipped default.  resident: tables[j]
// are device pointers.  info: regime, launches, blocks, rows a thread.  Returns the call's status.
int mleevalprobe_evaluate(tns_ctx *ctx, const uint64_t *const *tables, int n_tables, unsigned nv, uint64_t batch,
                          const uint64_t *points, int resident, uint64_t min_blocks, int max_log_rows,
                          uint64_t *values_out, int64_t *info) {
  if (!info) return -1;
  MleEvalReport r;
  const int st = mle_evaluate_batch(ctx, tables, n_tables, nv, (size_t)batch, points, values_out, resident != 0,
                                    limits(min_blocks, max_log_rows), &r);
  fill(r, info);
  return st;
}

int mleevalprobe_verify(tns_ctx *ctx, const uint64_t *const *tables, int n_tables, unsigned nv, uint64_t batch,
                        const uint64_t *claimed_sums, const tns_term *terms, int n_terms,
                        tns_transcript *const *transcripts, const uint64_t *rounds, const uint64_t *finals, int resident,
                        uint64_t *challenges_out, uint32_t *n_challenges_out, int *verdicts_out, uint64_t *values_out,
                        int64_t *info) {
  if (!info) return -1;
  MleEvalReport r;
  const int st = sumcheck_verify_batch(ctx, tables, n_tables, nv, (size_t)batch, claimed_sums, terms, n_terms, transcripts,
                                       rounds, finals, challenges_out, n_challenges_out, verdicts_out, values_out,
                                       resident != 0, MleEvalLimits(), &r);
  fill(r, info);
  return st;
}

// The baseline: mle_evaluate_dev (nv fold launches through ping-pong scratch, one synchronise) for
// every (instance, table) of resident tables, values_out[b n_tables + j].
int mleevalprobe_fold_chain(tns_ctx *ctx, const uint64_t *const *d_tables, int n_tables, unsigned nv, uint64_t batch,
                            const uint64_t *points, uint64_t *values_out) {
  return guarded([&]() {
    if (!ctx || !d_tables || !values_out || n_tables < 0 || n_tables > 4 || nv > 30)
      throw Error(TNS_ERR_INVALID_PARAMETERS, "bad probe call");
    CtxScope scope(&ctx->c);
    const size_t n = (size_t)1 << nv;
    std::vector<Fr> pt(nv ? nv : 1);
    for (size_t b = 0; b < batch; b++) {
      if (nv) std::memcpy((void *)pt.data(), points + 4 * (size_t)nv * b, sizeof(Fr) * nv);
      for (int j = 0; j < n_tables; j++) {
        const Fr v = mle_evaluate_dev(&ctx->c, (const Fr *)d_tables[j] + b * n, nv, pt.data());
        std::memcpy(values_out + 4 * (b * n_tables + j), &v, sizeof v);
      }
    }
    return (int)TNS_OK;
  });
}

}  // extern "C"
