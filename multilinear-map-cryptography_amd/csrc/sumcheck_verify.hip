// sumcheck_verify.hip -- SumCheck::verify for a batch of generic sum-check proofs of one shape,
// checked against their tables.
//
// SumCheck::verify (src/sumcheck.rs:113-153) replays the transcript and ends with
// current_sum == proof.final_evaluation: two numbers the prover supplied.  A proof is checked once
// final_evaluation is compared with the composition at the challenge point, one
// MultilinearExtension::evaluate (src/polynomials.rs:85-122) a table an instance.  Here:
//   1. the host replays every instance on its own transcript (sumcheck_replay_host, sumcheck_host.cpp);
//   2. ONE mle_evaluate_batch_dev pass (mle_eval.hip) evaluates every table of every instance at
//      the instance's challenges -- at most two launches whatever nv and batch; instances whose
//      replay failed ride along at the zero point;
//   3. the host evaluates the composition per instance (eval_composition_host, the prover's).
// Without tables (tables == NULL) it is the reference's verify, batched, and touches no device.
#include "abi.hpp"
#include "sc_poly.hpp"

namespace tns {

int sumcheck_verify_batch(tns_ctx *ctx, const uint64_t *const *tables, int n_tables, unsigned nv, size_t batch,
                          const uint64_t *claimed_sums, const tns_term *terms, int n_terms,
                          tns_transcript *const *transcripts, const uint64_t *rounds, const uint64_t *finals,
                          uint64_t *challenges_out, uint32_t *n_challenges_out, int *verdicts_out, uint64_t *values_out,
                          bool resident, const MleEvalLimits &lim, MleEvalReport *rep_out) {
  MleEvalReport rep;
  int status = guarded([&]() {
    // ---- the checks, before anything touches a transcript or a device
    if (!ctx) throw Error(TNS_ERR_INVALID_PARAMETERS, "null context");
    if (batch == 0) return (int)TNS_OK;
    sc_check_shape(nv, n_tables, n_terms);
    sc_check_arrays(claimed_sums && transcripts && finals && verdicts_out && (nv == 0 || rounds) && (n_terms == 0 || terms),
                    tables, n_tables, batch, nv);
    sc_check_transcripts(transcripts, batch);
    const std::vector<SumcheckTerm> st = sc_terms(terms, n_terms);
    sc_check_terms(st.data(), n_terms, n_tables);

    // ---- 1. the replay, per instance (src/sumcheck.rs:124-152)
    std::vector<Fr> rd(4 * (size_t)nv * batch + 1), fin(batch), cl(batch), chal((size_t)nv * batch + 1, Fr::zero());
    if (nv) std::memcpy((void *)rd.data(), rounds, sizeof(Fr) * 4 * (size_t)nv * batch);
    std::memcpy((void *)fin.data(), finals, sizeof(Fr) * batch);
    std::memcpy((void *)cl.data(), claimed_sums, sizeof(Fr) * batch);
    std::vector<int> verdict(batch);
    std::vector<uint32_t> nchal(batch);
    for (size_t b = 0; b < batch; b++) {
      unsigned nc = 0;
      verdict[b] = sumcheck_replay_host(transcripts[b]->t, cl[b], rd.data() + 4 * (size_t)nv * b, nv, fin[b],
                                        chal.data() + (size_t)nv * b, &nc);
      nchal[b] = nc;
    }

    // ---- 2. and 3. the final evaluations against the tables
    std::vector<Fr> vals((size_t)batch * std::max(n_tables, 0) + 1, Fr::zero());
    if (tables) {
      if (n_tables > 0) {
        const size_t n = (size_t)1 << nv;
        std::vector<Fr> pts((size_t)nv * batch + 1, Fr::zero());  // (a failed instance: the zero point)
        for (size_t b = 0; b < batch; b++)
          if (verdict[b] == 0) std::copy(chal.begin() + (size_t)nv * b, chal.begin() + (size_t)nv * (b + 1), pts.begin() + (size_t)nv * b);
        CtxScope scope(&ctx->c);
        Ctx *c = &ctx->c;
        StagedTables staged(c, tables, n_tables, sizeof(Fr) * batch * n, resident);
        mle_evaluate_batch_dev(c, staged.tab, n_tables, nv, batch, pts.data(), vals.data(), lim, &rep);
      }
      for (size_t b = 0; b < batch; b++) {
        Fr *v = vals.data() + (size_t)n_tables * b;
        if (verdict[b] != 0) {
          std::fill(v, v + n_tables, Fr::zero());
          continue;
        }
        if (eval_composition_host(v, st.data(), n_terms) != fin[b]) verdict[b] = 3;  // polynomial(&challenges)
      }
      if (values_out) std::memcpy(values_out, vals.data(), sizeof(Fr) * (size_t)n_tables * batch);
    }
    std::copy(verdict.begin(), verdict.end(), verdicts_out);
    if (n_challenges_out) std::copy(nchal.begin(), nchal.end(), n_challenges_out);
    if (challenges_out) std::memcpy(challenges_out, chal.data(), sizeof(Fr) * (size_t)nv * batch);
    return (int)TNS_OK;
  });
  if (rep_out) *rep_out = rep;
  return status;
}

}  // namespace tns

using namespace tns;

extern "C" {

int tns_sumcheck_verify_batch(tns_ctx *ctx, const uint64_t *const *tables, int n_tables, unsigned nv, size_t batch,
                              const uint64_t *claimed_sums, const tns_term *terms, int n_terms,
                              tns_transcript *const *transcripts, const uint64_t *rounds, const uint64_t *finals,
                              uint64_t *challenges_out, uint32_t *n_challenges_out, int *verdicts_out,
                              uint64_t *values_out) {
  return sumcheck_verify_batch(ctx, tables, n_tables, nv, batch, claimed_sums, terms, n_terms, transcripts, rounds, finals,
                               challenges_out, n_challenges_out, verdicts_out, values_out, false, MleEvalLimits(), nullptr);
}
int tns_sumcheck_verify_batch_device(tns_ctx *ctx, const uint64_t *const *d_tables, int n_tables, unsigned nv,
                                     size_t batch, const uint64_t *claimed_sums, const tns_term *terms, int n_terms,
                                     tns_transcript *const *transcripts, const uint64_t *rounds,
                                     const uint64_t *finals, uint64_t *challenges_out, uint32_t *n_challenges_out,
                                     int *verdicts_out, uint64_t *values_out) {
  return sumcheck_verify_batch(ctx, d_tables, n_tables, nv, batch, claimed_sums, terms, n_terms, transcripts, rounds,
                               finals, challenges_out, n_challenges_out, verdicts_out, values_out, true, MleEvalLimits(),
                               nullptr);
}

}  // extern "C"
