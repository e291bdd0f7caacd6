// sumcheck_front.hip -- the front door of the generic sum-check family's C entry points
// (sumcheck.hpp): the term conversion, the argument checks and the call-scoped device copies of
// host tables that the single, batched and verifying entries share, and the single prover's
// entry points themselves.
#include <algorithm>

#include "abi.hpp"
#include "sumcheck.hpp"

namespace tns {

std::vector<SumcheckTerm> sc_terms(const tns_term *terms, int n_terms, bool *table_terms) {
  std::vector<SumcheckTerm> st(n_terms);
  bool any = false;
  for (int t = 0; t < n_terms; t++) {
    std::memcpy(&st[t].coeff, terms[t].coeff, 32);
    for (int j = 0; j < 3; j++) {
      st[t].tab[j] = terms[t].tables[j];
      any = any || st[t].tab[j] >= 0;
    }
  }
  if (table_terms) *table_terms = any;
  return st;
}

void sc_check_shape(unsigned nv, int n_tables, int n_terms) {
  if (nv > 30 || n_tables < 0 || n_tables > MAX_SC_TABLES || n_terms < 0)
    throw Error(TNS_ERR_INVALID_PARAMETERS, "unsupported sum-check shape (<= 4 tables)");
}

void sc_check_arrays(bool have, const uint64_t *const *tables, int n_tables, size_t batch, unsigned nv) {
  for (int j = 0; have && tables && j < n_tables; j++) have = tables[j] != nullptr;
  if (!have) throw Error(TNS_ERR_INVALID_PARAMETERS, "null input or output array");
  if (batch > (BATCH_MAX_SCALARS >> nv)) throw Error(TNS_ERR_INVALID_PARAMETERS, "batch * 2^nv exceeds 2^32 entries");
}

void sc_check_transcripts(tns_transcript *const *transcripts, size_t batch) {
  std::vector<const tns_transcript *> seen(transcripts, transcripts + batch);
  for (const tns_transcript *t : seen)
    if (!t) throw Error(TNS_ERR_INVALID_PARAMETERS, "null transcript handle");
  std::sort(seen.begin(), seen.end());
  if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
    throw Error(TNS_ERR_INVALID_PARAMETERS, "the same transcript handle twice in one batch");
}

StagedTables::StagedTables(Ctx *c, const uint64_t *const *tables, int k, size_t bytes, bool resident) : drain_{c} {
  for (int j = 0; j < k; j++) tab[j] = (Fr *)on_device(c, tables[j], bytes, resident, up_[j]);
}

namespace {

// tns_sumcheck_prove(_device) once the tables are on the device
int prove_single(tns_ctx *ctx, Fr *const *tabs, int n_tables, unsigned nv, const uint64_t claimed[4],
                 const tns_term *terms, int n_terms, tns_transcript *tr, uint64_t *rounds_out, uint64_t final_out[4],
                 uint64_t *challenges_out) {
  const std::vector<SumcheckTerm> st = sc_terms(terms, n_terms);
  Fr cl;
  std::memcpy(&cl, claimed, 32);
  std::vector<Fr> rounds(4 * (size_t)(nv ? nv : 1)), chal(nv ? nv : 1);
  Fr fe;
  int rc = sumcheck_prove_dev(&ctx->c, tabs, n_tables, nv, cl, st.data(), n_terms, tr->t, rounds.data(), chal.data(), &fe);
  std::memcpy(rounds_out, rounds.data(), 128 * (size_t)nv);
  if (challenges_out) std::memcpy(challenges_out, chal.data(), 32 * (size_t)nv);
  std::memcpy(final_out, &fe, 32);
  return rc;
}

}  // namespace
}  // namespace tns

using namespace tns;

extern "C" {

int tns_sumcheck_prove(tns_ctx *ctx, const uint64_t *const *tables, int n_tables, unsigned nv,
                       const uint64_t claimed[4], const tns_term *terms, int n_terms, tns_transcript *tr,
                       uint64_t *rounds_out, uint64_t final_out[4], uint64_t *challenges_out) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    sc_check_shape(nv, n_tables, n_terms);
    StagedTables staged(&ctx->c, tables, n_tables, sizeof(Fr) << nv, false);
    return prove_single(ctx, staged.tab, n_tables, nv, claimed, terms, n_terms, tr, rounds_out, final_out, challenges_out);
  });
}

int tns_sumcheck_prove_device(tns_ctx *ctx, const uint64_t *const *d_tables, int n_tables, unsigned nv,
                              const uint64_t claimed[4], const tns_term *terms, int n_terms, tns_transcript *tr,
                              uint64_t *rounds_out, uint64_t final_out[4], uint64_t *challenges_out) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    sc_check_shape(nv, n_tables, n_terms);
    Fr *tab[MAX_SC_TABLES] = {};  // resident: used as they are (only read), nothing staged, nothing to drain
    for (int j = 0; j < n_tables; j++) tab[j] = (Fr *)d_tables[j];
    return prove_single(ctx, tab, n_tables, nv, claimed, terms, n_terms, tr, rounds_out, final_out, challenges_out);
  });
}

int tns_composition_sum_device(tns_ctx *ctx, const uint64_t *const *d_tables, int n_tables, unsigned nv,
                               const tns_term *terms, int n_terms, uint64_t out[4]) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    sc_check_shape(nv, n_tables, n_terms);
    Fr *tab[MAX_SC_TABLES] = {};  // resident: used as they are (only read), nothing staged, nothing to drain
    for (int j = 0; j < n_tables; j++) tab[j] = (Fr *)d_tables[j];
    const std::vector<SumcheckTerm> st = sc_terms(terms, n_terms);
    const Fr s = composition_sum_dev(&ctx->c, tab, n_tables, nv, st.data(), n_terms);
    std::memcpy(out, &s, 32);
    return (int)TNS_OK;
  });
}

}  // extern "C"
