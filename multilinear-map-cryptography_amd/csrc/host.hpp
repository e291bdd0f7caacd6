// host.hpp -- what libtns computes on the host alone: G2 and the pairing (pairing.cpp), the
// reference verifiers (verify.cpp), the ark-serialize encodings (serialize.cpp), the Fiat-Shamir
// transcript with its hash and sampling helpers (transcript.cpp), and the host's turn of a
// sum-check round with the replay built from it (sumcheck_host.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "bn254.hpp"

namespace tns {

// pairing.cpp: BN254 G2 (D-type twist, affine over Fq2 = Fq[u]/(u^2+1)) and the pairing
struct G2Affine {
  Fq x0, x1, y0, y1;  // x = x0 + x1 u, y = y0 + y1 u
  bool inf = false;
};
G2Affine g2_generator();
G2Affine g2_add(const G2Affine &a, const G2Affine &b);
G2Affine g2_neg(const G2Affine &a);
G2Affine g2_mul(const G2Affine &a, const uint64_t k_canonical[4]);
bool g2_on_curve(const G2Affine &a);
bool pairing_eq(const G1Affine &P1, const G2Affine &Q1, const G1Affine &P2, const G2Affine &Q2);
void pairing_value(const G1Affine &P, const G2Affine &Q, Fq out[12]);

// verify.cpp: the reference verifiers (host)
G1Xyzz g1_mul_host(const G1Affine &P, const Fr &k);
G1Affine g1_generator_host();
void verifier_key(const Fr &tau, G1Affine *g1, G2Affine *g2, G2Affine *g2_tau);
bool kzg_verify_host(const G1Affine &g1, const G2Affine &g2, const G2Affine &g2_tau, const G1Affine &C,
                     const Fr &z, const Fr &v, const G1Affine &pi);
bool kzg_batch_verify_host(const G1Affine &g1, const G2Affine &g2, const G2Affine &g2_tau, size_t n,
                           const G1Affine *C, const Fr *z, const Fr *v, const G1Affine *pi);
// the batched check's challenges [first, first + count) of `seed`, canonical 4 x u64 each
void verify_challenges_host(const uint8_t seed[32], uint64_t first, size_t count, uint64_t *out);
bool protocol_verify_host(const G1Affine &g1, const G2Affine &g2, const G2Affine &g2_tau, const char *label0,
                          const char *label1, const G1Affine C[2], const Fr *rounds, unsigned nv,
                          const Fr &final_eval, unsigned n_openings, const G1Affine pi[2], const Fr vals[2]);

// serialize.cpp: ark-serialize 0.4 canonical encodings (host)
void g1_serialize(const G1Affine &P, bool compressed, uint8_t *out);
G1Affine g1_deserialize(const uint8_t *in, bool compressed, bool validate);
void fr_serialize(const Fr &x, uint8_t out[32]);
Fr fr_deserialize(const uint8_t in[32]);

// host-side helpers (transcript.cpp)
struct HostTranscript {
  std::vector<uint8_t> state;
  void append_label(const char *s);
  void append_bytes(const uint8_t *p, size_t n);
  void append_fr(const Fr &x);
  Fr challenge(const char *label);
  Fr challenge_bytes(const uint8_t *label, size_t n);
  // The next challenge's hash, started early: DefaultHasher writes the state's length FIRST, so no
  // hash state carries over between challenges -- but once the length the state will have at the
  // next challenge is known (a sum-check round appends fixed-size data), the SipHash blocks of the
  // bytes already in the state can run while the device computes the round; challenge() then
  // hashes only the round's own ~170 bytes.  Same hash, same challenge.
  void prehash(size_t final_len);
  struct Pre {
    bool valid = false;
    size_t final_len = 0, done = 0;  // bytes of the state absorbed (a multiple of 8)
    uint64_t v[4];
  } pre;
};
Fr commitment_hash(const G1Affine &a);
Fr host_fr_rand_chacha(const uint8_t seed[32], uint8_t *fs_seed_out /* nullable: next 32 bytes */);
uint64_t siphash13_keys00(const uint8_t *msg, size_t n);
void host_fr_rand_stream(const uint8_t seed[32], size_t n, Fr *out);
void chacha20_block_host(const uint32_t key[8], uint64_t counter, uint32_t out[16]);
// Lagrange interpolation of 4 points (0..3) for sum-check round polys (host, exact).
void interpolate4_host(const Fr e[4], Fr out[4]);
Fr horner_host(const Fr *c, int n, const Fr &z);

// sumcheck_host.cpp: the host's turn of a sum-check round (src/sumcheck.rs:77-100), in the pieces
// every prover and the replay compose.  The two transcript labels of round rnd, and the bytes a
// round adds to the state: both labels and four coefficients.
struct SumcheckLabels {
  char round[32], challenge[32];
  size_t added;
  explicit SumcheckLabels(unsigned rnd);
};
// HostTranscript::prehash for the round's challenge, on a state that holds the earlier rounds
void sumcheck_prehash(HostTranscript &tr, const SumcheckLabels &lab);
// g(0) + g(1) == claim (:80-84)
bool sumcheck_round_holds(const Fr coeffs[4], const Fr &claim);
// The round polynomial's coefficients from its sums e at X = 0..3 (lagrange_interpolate, :201-206);
// g1_from_claim: e[1] is not read, g(1) is the claim minus g(0).  Returns sumcheck_round_holds.
bool sumcheck_round_coeffs(const Fr e[4], const Fr &claim, bool g1_from_claim, Fr coeffs[4]);
// Appends the round's label and coefficients and draws its challenge (:90-96)
Fr sumcheck_absorb_round(HostTranscript &tr, const SumcheckLabels &lab, const Fr coeffs[4]);
inline Fr sumcheck_next_claim(const Fr coeffs[4], const Fr &ch) { return horner_host(coeffs, 4, ch); }
// The nv rounds of a closure that is the constant c everywhere (c = 0: the zero closure of Twist /
// Shout), on the transcript alone; rounds (nv x 4) and chal (nv) are optional.
void sumcheck_constant_rounds(HostTranscript &tr, unsigned nv, const Fr &c, Fr *rounds, Fr *chal);
// SumCheck::verify's replay (src/sumcheck.rs:124-152) for any claimed sum.  Returns 0: every round
// check held and the last claim equals final_eval; 1: round *n_chal failed g(0) + g(1) == claim --
// the replay stopped before appending it, the transcript holds the earlier rounds only; 2: the
// rounds held, the last claim differs.  chal (optional, nv entries): the challenges drawn,
// *n_chal (optional) of them.
int sumcheck_replay_host(HostTranscript &tr, const Fr &claimed, const Fr *rounds, unsigned nv, const Fr &final_eval,
                         Fr *chal, unsigned *n_chal);
// ... with claimed sum 0, as Twist::verify / Shout::verify call it
bool sumcheck_verify_host(HostTranscript &tr, const Fr *rounds, unsigned nv, const Fr &final_eval);

}  // namespace tns
