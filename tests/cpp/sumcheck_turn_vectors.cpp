// CPU test (tests/test_sumcheck_turn_cpu.py): the host's turn of a sum-check round
// (csrc/sumcheck_host.cpp) without tables.  Usage: sumcheck_turn_vectors <nv>.  A prover made of the
// library's own pieces runs nv rounds on a transcript with a prefix; round polynomials come from
// chosen sums: seeded e0, e2, e3 a round, e1 the claim minus e0, round 0's claim e0 + e1.  Prints
// what the prover, the replays (honest and tampered), the constant rounds and a run without
// prehash saw -- coefficients, challenges and transcript states, canonical values as 64 hex
// digits -- and judges nothing: every comparison is the Python side's.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host.hpp"
using namespace tns;

static void put(const Fr &a) {
  const Fr c = from_mont(a);
  putchar(' ');
  for (int i = 7; i >= 0; i--) printf("%08x", c.v[i]);
}
static void put_state(const HostTranscript &tr) {
  putchar(' ');
  for (uint8_t b : tr.state) printf("%02x", b);
  if (tr.state.empty()) putchar('-');
}
static HostTranscript fresh() {
  HostTranscript tr;
  tr.append_label("instance");
  tr.append_fr(from_u64<FrCfg>(1000003));
  return tr;
}

struct Run {
  std::vector<Fr> coeffs, chal;
  Fr last;  // the claim after the last round
  HostTranscript tr = fresh();
  bool held = true;
};

// the single prover's turns (sumcheck.hip: sumcheck_prove_terms) on sums[4 rnd + x]; round 0 reads
// all four sums, later rounds take g(1) from the claim.  tag: print the rounds under it.
static Run prove(unsigned nv, const Fr &claim, const std::vector<Fr> &sums, bool prehash, const char *tag) {
  Run R;
  Fr cur = claim;
  SumcheckLabels lab(0);
  if (prehash && nv > 0) sumcheck_prehash(R.tr, lab);
  for (unsigned rnd = 0; rnd < nv; rnd++) {
    if (tag) printf("%s_state %u", tag, rnd), put_state(R.tr), putchar('\n');
    if (tag) {
      printf("%s_sums %u", tag, rnd);
      for (int x = 0; x < 4; x++) put(sums[4 * rnd + x]);
      putchar('\n');
    }
    Fr c[4];
    if (!sumcheck_round_coeffs(&sums[4 * rnd], cur, rnd > 0, c)) {
      R.held = false;
      break;
    }
    const Fr ch = sumcheck_absorb_round(R.tr, lab, c);
    cur = sumcheck_next_claim(c, ch);
    R.coeffs.insert(R.coeffs.end(), c, c + 4);
    R.chal.push_back(ch);
    if (tag) {
      printf("%s_round %u", tag, rnd);
      for (int x = 0; x < 4; x++) put(c[x]);
      put(ch), putchar('\n');
    }
    if (rnd + 1 < nv) {
      lab = SumcheckLabels(rnd + 1);
      if (prehash) sumcheck_prehash(R.tr, lab);
    }
  }
  R.last = cur;
  if (tag) printf("%s_state %u", tag, nv), put_state(R.tr), putchar('\n');
  if (tag) printf("%s_end %d", tag, (int)R.held), put(cur), putchar('\n');
  return R;
}

static void replay(const char *tag, const Fr &claim, const std::vector<Fr> &coeffs, unsigned nv, const Fr &final_eval) {
  HostTranscript tr = fresh();
  std::vector<Fr> chal(nv + 1, Fr::zero());
  unsigned n_chal = 77;
  const int verdict = sumcheck_replay_host(tr, claim, coeffs.data(), nv, final_eval, chal.data(), &n_chal);
  printf("%s %d %u", tag, verdict, n_chal);
  put_state(tr);
  for (unsigned i = 0; i < n_chal; i++) put(chal[i]);
  putchar('\n');
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  const unsigned nv = (unsigned)atoi(argv[1]);
  uint8_t seed[32];
  for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(16 * nv + i);
  std::vector<Fr> sums(4 * (size_t)nv + 4);
  host_fr_rand_stream(seed, sums.size(), sums.data());
  const Fr claim = add(sums[0], sums[1]);
  printf("claim"), put(claim), putchar('\n');

  // (a) the honest run and its replay; (d) the same run without prehash
  const Run H = prove(nv, claim, sums, true, "honest");
  prove(nv, claim, sums, false, "noprehash");
  replay("replay", claim, H.coeffs, nv, H.last);
  // (b) one coefficient of round r changed (c0 moves g(0) + g(1) by 2, c3 by 1); the final changed
  for (unsigned r = 0; r < nv; r++)
    for (int x = 0; x < 4; x += 3) {
      std::vector<Fr> bad = H.coeffs;
      bad[4 * r + x] = add(bad[4 * r + x], Fr::one());
      char tag[32];
      snprintf(tag, sizeof tag, "tamper_%u_%d", r, x);
      replay(tag, claim, bad, nv, H.last);
    }
  replay("tamper_final", claim, H.coeffs, nv, add(H.last, Fr::one()));
  // a wrong claim stops the prover's own round 0 before it appends anything
  prove(nv, add(claim, Fr::one()), sums, true, "wrongclaim");

  // (c) the constant closure c: sumcheck_constant_rounds against turns fed c 2^(nv-1-rnd)
  for (unsigned cv = 0; cv <= 5; cv += 5) {
    const Fr c = from_u64<FrCfg>(cv);
    std::vector<Fr> cs(4 * (size_t)nv + 4, Fr::zero());
    Fr total = c;  // c 2^nv
    for (unsigned j = 0; j < nv; j++) total = add(total, total);
    for (unsigned rnd = 0; rnd < nv; rnd++) {
      Fr g = c;
      for (unsigned j = rnd + 1; j < nv; j++) g = add(g, g);
      for (int x = 0; x < 4; x++) cs[4 * rnd + x] = g;
    }
    char tag[32];
    snprintf(tag, sizeof tag, "turns_%u", cv);
    prove(nv, total, cs, true, tag);
    HostTranscript tr = fresh();
    std::vector<Fr> rounds(4 * (size_t)nv + 4), chal(nv + 1);
    sumcheck_constant_rounds(tr, nv, c, rounds.data(), chal.data());
    for (unsigned rnd = 0; rnd < nv; rnd++) {
      printf("constant_%u_round %u", cv, rnd);
      for (int x = 0; x < 4; x++) put(rounds[4 * rnd + x]);
      put(chal[rnd]), putchar('\n');
    }
    printf("constant_%u_state %u", cv, nv), put_state(tr), putchar('\n');
    // sumcheck_verify_host is the replay with claimed sum 0: it accepts the rounds of c = 0 alone
    HostTranscript tv = fresh();
    printf("constant_%u_verify %d\n", cv, (int)sumcheck_verify_host(tv, rounds.data(), nv, c));
  }
  return 0;
}
