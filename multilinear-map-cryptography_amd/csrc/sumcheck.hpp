// sumcheck.hpp -- the generic sum-check family's internal declarations: the engine (sumcheck.hip),
// the batched prover (sumcheck_batch.hip), the batched verifier (sumcheck_verify.hip), the one-pass
// MLE evaluation (mle_eval.hip), and the front door their C entry points share
// (sumcheck_front.hip).  The host's turn of a round is host.hpp's (sumcheck_host.cpp), what the
// round kernels share sc_poly.hpp's.
#pragma once
#include <vector>

#include "ctx.hpp"
#include "host.hpp"
#include "sc_tables.hpp"
#include "sumcheck_batch_plan.hpp"

namespace tns {

// ---- sumcheck.hip
struct SumcheckTerm {
  Fr coeff;
  int tab[3];
};
Fr composition_sum_dev(Ctx *c, Fr *const *tables, int k, unsigned nv, const SumcheckTerm *terms, int n_terms);
// Runs every round of SumCheck::prove over k device tables of 2^nv entries (only read: they are
// folded into workspace) on the host's transcript.  Returns status; fills rounds (nv x 4), the
// challenges and the final evaluation.
int sumcheck_prove_dev(Ctx *c, Fr *const *tables, int k, unsigned nv, const Fr &claimed,
                       const SumcheckTerm *terms, int n_terms, HostTranscript &tr, Fr *rounds,
                       Fr *challenges, Fr *final_eval);

// ---- sumcheck_front.hip: what the C entry points do before they reach a device, each check in the
// order and with the message include/tns.h documents
// tns_term[] as the engine reads it; *table_terms (optional): some term has a table factor
std::vector<SumcheckTerm> sc_terms(const tns_term *terms, int n_terms, bool *table_terms = nullptr);
void sc_check_shape(unsigned nv, int n_tables, int n_terms);
// `have`: every array the call needs is there; then every tables[j] (tables == NULL: none to check)
// and batch * 2^nv <= 2^32 entries
void sc_check_arrays(bool have, const uint64_t *const *tables, int n_tables, size_t batch, unsigned nv);
// no NULL handle, no handle twice
void sc_check_transcripts(tns_transcript *const *transcripts, size_t batch);
// A call's k <= MAX_SC_TABLES tables of `bytes` each on the device: resident input as it is, host
// input uploaded on c->stream into buffers that live as long as this object.  On every exit the
// stream is drained and only then are the buffers freed: members die in reverse order, and
// `drain` is the last of them.
class StagedTables {
 public:
  StagedTables(Ctx *c, const uint64_t *const *tables, int k, size_t bytes, bool resident);
  Fr *tab[MAX_SC_TABLES] = {nullptr, nullptr, nullptr, nullptr};  // only read

 private:
  DevBuf up_[MAX_SC_TABLES];
  struct Drain {
    Ctx *c;
    ~Drain() { (void)hipStreamSynchronize(c->stream); }
  } drain_;
};

// ---- sumcheck_batch.hip: tns_sumcheck_prove_batch(_device) with the limits as an argument (the
// entry points pass the defaults, the probe of tests/device/scbatchprobe.hip forces routes and
// splits); rep (optional): what the call took -- the plan's route and groups, and the launches the
// batched route queued (nv + 1 a group; 0 on the rows route)
struct ScBatchReport {
  int route = BATCH_ROUTE_ROWS;
  size_t group_rows = 1, groups = 0, launches = 0;
};
int sumcheck_prove_batch(tns_ctx *ctx, const uint64_t *const *tables, int n_tables, unsigned nv, size_t batch,
                         const uint64_t *claimed_sums, const tns_term *terms, int n_terms,
                         tns_transcript *const *transcripts, uint64_t *rounds_out, uint64_t *finals_out,
                         uint64_t *challenges_out, bool resident, const ScBatchLimits &lim, ScBatchReport *rep);

// ---- mle_eval.hip
// values_host[b k + j] = MLE(tables[j] + b 2^nv)(points_host + b nv) for every instance b and table
// j < k <= 4 in one pass: every entry read once, at most two launches whatever nv and batch, one
// synchronise.  lim: the launch geometry's limits (the entry points pass the defaults, the probe
// of tests/device/mleevalprobe.hip forces them); rep (optional): what ran.
enum : int { MLE_EVAL_NONE = 0, MLE_EVAL_WAVE = 1, MLE_EVAL_BLOCK = 2, MLE_EVAL_BLOCKS = 3 };
struct MleEvalLimits {
  // a thread takes more rows only while the launch keeps this many blocks, and at most
  // 2^max_log_rows.  Measured (profiles/mle_eval_bench.json rows_sweep): a block's
  // fixed cost -- the eq_lo products, the block sum and, across blocks, the fence before its
  // counter increment -- outweighs what more blocks a CU hide, so one block a CU (256 CUs) is the
  // floor; beyond 64 rows a thread the time is flat
  size_t min_blocks = 256;
  unsigned max_log_rows = 6;
};
struct MleEvalReport {
  int regime = MLE_EVAL_NONE;     // how an instance's sum is formed: part of a wave, one block, several blocks
  size_t launches = 0, blocks = 0, rows_per_thread = 0;  // blocks: of the dot-product launch
};
void mle_evaluate_batch_dev(Ctx *c, const Fr *const *tables, int k, unsigned nv, size_t batch, const Fr *points_host,
                            Fr *values_host, const MleEvalLimits &lim = MleEvalLimits(), MleEvalReport *rep = nullptr);
// tns_mle_evaluate_batch(_device) with the limits as an argument
int mle_evaluate_batch(tns_ctx *ctx, const uint64_t *const *tables, int n_tables, unsigned nv, size_t batch,
                       const uint64_t *points, uint64_t *values_out, bool resident, const MleEvalLimits &lim,
                       MleEvalReport *rep);

// ---- sumcheck_verify.hip: tns_sumcheck_verify_batch(_device) likewise; rep: the one evaluation pass
int sumcheck_verify_batch(tns_ctx *ctx, const uint64_t *const *tables, int n_tables, unsigned nv, size_t batch,
                          const uint64_t *claimed_sums, const tns_term *terms, int n_terms,
                          tns_transcript *const *transcripts, const uint64_t *rounds, const uint64_t *finals,
                          uint64_t *challenges_out, uint32_t *n_challenges_out, int *verdicts_out, uint64_t *values_out,
                          bool resident, const MleEvalLimits &lim, MleEvalReport *rep);

}  // namespace tns
