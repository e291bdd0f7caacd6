// sumcheck_host.cpp -- the host's turn of a sum-check round (SumCheck::prove, src/sumcheck.rs:77-100;
// SumCheck::verify, :113-152), the one place that names the round's transcript labels.  The single
// prover (sumcheck.hip), the batched prover (sumcheck_batch.hip), the constant rounds and the
// replay below compose the same pieces, so a prover and a verifier cannot differ by an append.
#include <cstdio>

#include "host.hpp"

namespace tns {

SumcheckLabels::SumcheckLabels(unsigned rnd) {
  const int n1 = snprintf(round, sizeof round, "sumcheck_round_%u", rnd);
  const int n2 = snprintf(challenge, sizeof challenge, "sumcheck_challenge_%u", rnd);
  added = (size_t)n1 + 4 * 32 + (size_t)n2;
}

void sumcheck_prehash(HostTranscript &tr, const SumcheckLabels &lab) { tr.prehash(tr.state.size() + lab.added); }

bool sumcheck_round_holds(const Fr coeffs[4], const Fr &claim) {
  return add(horner_host(coeffs, 4, Fr::zero()), horner_host(coeffs, 4, Fr::one())) == claim;
}

bool sumcheck_round_coeffs(const Fr e[4], const Fr &claim, bool g1_from_claim, Fr coeffs[4]) {
  const Fr p[4] = {e[0], g1_from_claim ? sub(claim, e[0]) : e[1], e[2], e[3]};
  interpolate4_host(p, coeffs);
  return sumcheck_round_holds(coeffs, claim);
}

Fr sumcheck_absorb_round(HostTranscript &tr, const SumcheckLabels &lab, const Fr coeffs[4]) {
  tr.append_label(lab.round);
  for (int x = 0; x < 4; x++) tr.append_fr(coeffs[x]);
  return tr.challenge(lab.challenge);
}

// Round rnd's polynomial is the constant c 2^(nv-1-rnd) -- [that, 0, 0, 0] as coefficients -- so
// the transcript alone yields the challenges (prove.hip zero_closure_transcript: c = 0)
void sumcheck_constant_rounds(HostTranscript &tr, unsigned nv, const Fr &c, Fr *rounds, Fr *chal) {
  std::vector<Fr> g(nv);  // g[rnd] = c 2^(nv-1-rnd)
  for (unsigned rnd = nv; rnd-- > 0;) g[rnd] = rnd + 1 == nv ? c : add(g[rnd + 1], g[rnd + 1]);
  for (unsigned rnd = 0; rnd < nv; rnd++) {
    const Fr coeffs[4] = {g[rnd], Fr::zero(), Fr::zero(), Fr::zero()};
    for (int x = 0; rounds && x < 4; x++) rounds[4 * rnd + x] = coeffs[x];
    const Fr ch = sumcheck_absorb_round(tr, SumcheckLabels(rnd), coeffs);
    if (chal) chal[rnd] = ch;
  }
}

// round polynomials are 4 coefficients (evaluate_round_polynomial = Horner, :209-212)
int sumcheck_replay_host(HostTranscript &tr, const Fr &claimed, const Fr *rounds, unsigned nv, const Fr &final_eval,
                         Fr *chal, unsigned *n_chal) {
  Fr cur = claimed;
  if (n_chal) *n_chal = 0;
  for (unsigned r = 0; r < nv; r++) {
    const Fr *c = rounds + 4 * (size_t)r;
    if (!sumcheck_round_holds(c, cur)) return 1;  // :132-134, before the round is appended
    const Fr ch = sumcheck_absorb_round(tr, SumcheckLabels(r), c);
    if (chal) chal[r] = ch;
    if (n_chal) *n_chal = r + 1;
    cur = sumcheck_next_claim(c, ch);
  }
  return cur == final_eval ? 0 : 2;
}

bool sumcheck_verify_host(HostTranscript &tr, const Fr *rounds, unsigned nv, const Fr &final_eval) {
  return sumcheck_replay_host(tr, Fr::zero(), rounds, nv, final_eval, nullptr, nullptr) == 0;
}

}  // namespace tns
