// abi.hpp -- what the translation units of the C ABI share: the opaque handle types of
// include/tns.h, the error guard of every entry point, the KZG routes of kzg.hip and kzg_batch.hip,
// and the batched provers' and verifiers' internal entry points.  (The generic sum-check family
// declares its own in sumcheck.hpp.)
#pragma once
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "comm.hpp"
#include "ctx.hpp"
#include "host.hpp"
#include "srs.hpp"

struct tns_ctx {
  tns::Ctx c;
  double timing[6] = {0, 0, 0, 0, 0, 0};
};
struct tns_srs {
  tns::Srs s;
};
struct tns_transcript {
  tns::HostTranscript t;
};
struct tns_comm {
  tns::Comm *c = nullptr;
  ~tns_comm() { delete c; }
};
struct tns_buffer {
  tns::DevBuf buf;
  size_t bytes = 0;
  int device = 0;
};

namespace tns {

template <class F>
static int guarded(F &&f) {
  try {
    return f();
  } catch (const Error &e) {
    set_last_error(e.what());
    return e.code;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return TNS_ERR_DEVICE;
  }
}

static void store_proj(const G1Affine &a, uint64_t out[12]) {
  G1Jac j = affine_to_jac(a);
  std::memcpy(out, &j, sizeof j);
}
static G1Affine proj_to_affine_host(const uint64_t in[12]) {
  G1Jac j;
  std::memcpy(&j, in, sizeof j);
  G1Affine a;
  if (j.z.is_zero()) {
    a.x = Fq::zero();
    a.y = Fq::zero();
    return a;
  }
  Fq zi = inv(j.z), zi2 = sqr(zi);
  a.x = mul(j.x, zi2);
  a.y = mul(j.y, mul(zi2, zi));
  return a;
}

struct Timer {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double ms() const {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
};

// One committed vector of Twist/Shout::prove: evaluations y on the nodes 0..N-1
// (vector_to_polynomial input, src/polynomials.rs:248-262), of which this rank holds the
// slice [first, first + cnt).  Committed and opened via the Lagrange basis when the SRS
// provides it (partial MSMs summed over the ranks), else via interpolated coefficients.
struct EvalPoly {
  const Fr *y = nullptr;       // device, cnt (must stay intact until opened)
  Fr *coeffs = nullptr;        // device scratch, N (coefficient path, unsharded only)
  size_t N = 0, first = 0, cnt = 0;
  const LagrangeBasis *basis = nullptr;
  bool have_coeffs = false;
};

// What rides along with an exchange of MSM partials (the exchanges of a sharded proof are few and
// latency-bound, so independent payloads share one): `bytes` of this rank's data, every rank's
// copy landing rank-major in `all` (size * bytes).
struct ExtraPayload {
  const void *data = nullptr;
  size_t bytes = 0;  // a multiple of 4
  std::vector<uint8_t> all;
};

// kzg.hip
G1Affine commit_dev(Ctx *c, const Srs &srs, const Fr *coeffs, size_t n);
void open_dev(Ctx *c, const Srs &srs, const Fr *coeffs, size_t n, const Fr &z, Fr *value, G1Affine *proof,
              DevBuf &sbuf);
G1Affine commit_evals(Ctx *c, const Srs &srs, EvalPoly &p, Comm &m);
void open_evals(Ctx *c, const Srs &srs, EvalPoly &p, const Fr &z, Fr *value, G1Affine *proof, DevBuf &sbuf, Comm &m);
void commit_evals_pair(Ctx *c, const Srs &srs, EvalPoly &p0, EvalPoly &p1, Comm &m, G1Affine out[2],
                       const ScalarSource *src0 = nullptr, const ScalarSource *src1 = nullptr,
                       ExtraPayload *extra = nullptr);
void open_evals_pair(Ctx *c, const Srs &srs, EvalPoly &p0, EvalPoly &p1, const Fr &z, Fr value[2], G1Affine proof[2],
                     DevBuf &sbuf0, DevBuf &sbuf1, Comm &m, ExtraPayload *extra = nullptr,
                     const std::function<void()> &extra_ready = nullptr,
                     const std::function<void()> &side_work = nullptr);
// kzg_batch.hip: `rows` vectors of n entries (rows x n Montgomery forms on the device) over one SRS,
// results in host arrays of `rows` elements; lim: msm_batch_plan.hpp's limits (the entry points pass
// the defaults, the probe of tests/device/batchprobe.hip forces routes and splits); rep (optional):
// the route taken.  msm_batch_srs: out[b] = sum_i d_s[b n + i] g1_powers[i]; commit_evals_batch /
// open_evals_batch: commit_evals / open_evals of every row (every row at the same z).
void msm_batch_srs(Ctx *c, const Srs &srs, const Fr *d_s, size_t n, size_t rows, const BatchLimits &lim,
                   G1Affine *out_host, BatchReport *rep);
void commit_evals_batch(Ctx *c, const Srs &srs, const Fr *d_y, size_t n, size_t rows, const BatchLimits &lim,
                        G1Affine *out_host, BatchReport *rep);
void open_evals_batch(Ctx *c, const Srs &srs, const Fr *d_y, size_t n, size_t rows, const Fr &z, const BatchLimits &lim,
                      Fr *values_host, G1Affine *proofs_host, BatchReport *rep);
// open_evals_batch with one point per g consecutive rows (row r at points_host[r / g], ceil(rows / g)
// Montgomery points on the host; nodes and other points may be mixed): the public calls pass g = 1,
// the batched provers g = 2 so that a proof's two vectors share their inverses
void open_evals_batch_points(Ctx *c, const Srs &srs, const Fr *d_y, size_t n, size_t rows, const Fr *points_host,
                             size_t g, const BatchLimits &lim, Fr *values_host, G1Affine *proofs_host,
                             BatchReport *rep);
// prove_batch.hip: what the batched provers' stages took (tests/device/provebatchprobe.hip)
struct ProveBatchReport {
  int route = 0;
  BatchReport commit[2], open[2];  // commitments 0 and 1; opening calls (one call: open[0] alone)
  int open_calls = 0, rows_per_point = 0;
};
int twist_prove_batch(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, const uint64_t *addr,
                      const uint64_t *value, const uint8_t *is_write, size_t n_ops, size_t batch, tns_proof *out,
                      bool resident, const BatchLimits &lim, ProveBatchReport *rep);
int shout_prove_batch(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, const uint64_t *entries,
                      size_t n_entries, const uint64_t *indices, size_t n_lookups, size_t batch, tns_proof *out,
                      bool resident, const BatchLimits &lim, ProveBatchReport *rep);
// abi_host.cpp: a tns_vk's three points, each checked against its curve
struct Vk {
  G1Affine g1;
  G2Affine g2, g2_tau;
};
Vk vk_load(const tns_vk *vk);
// kzg_verify.hip: k openings (C_i, z_i, v_i, pi_i) on the device, checked in one weighted pairing
// equation.  commitments == nullptr: `shared` is every opening's commitment; z == nullptr: z_i = i
// (a vector commitment's openings); v and z in Montgomery form.
struct VerifyBatch {
  const G1Affine *proofs = nullptr;
  const G1Affine *commitments = nullptr;
  G1Affine shared{};
  const Fr *z = nullptr, *v = nullptr;
  size_t k = 0;
};
// false: *bad = the lowest malformed position, or with `locate` the lowest failing opening's
// (bisected with the same challenges); seed == nullptr: 32 bytes from the OS
bool kzg_verify_many_dev(Ctx *c, const Vk &vk, const VerifyBatch &in, const uint8_t seed[32], bool locate,
                         uint64_t *bad);
// prove.hip
void check_shard(const Comm &m, size_t N, const char *what);
size_t slice_count(uint64_t n_total, size_t first, size_t L);
// What the transcript alone decides of a Twist / Shout proof, for the single and the batched
// provers: the two commitments appended under their labels, the nv all-zero sum-check rounds
// (sumcheck_constant_rounds) and, when nv >= 1, the opening point opening_challenges_0, which is
// returned.  Stores the commitments, num_rounds, the zero round polynomials, the challenges, the
// zero final evaluation and the opening point into *out, and the challenges into chal[0 .. nv) as
// well (the caller's memory: the single prover's fold chain copies them from pinned memory).
Fr zero_closure_transcript(const char *label0, const char *label1, const G1Affine cm[2], unsigned nv, Fr *chal,
                           tns_proof *out);
// LookupTable::lookup bounds (src/shout.rs:44-50): whether some idx[i] >= bound (n device values).
// Zeroes the device word `bad`, runs the check on st, copies the word back and waits for st.
bool index_out_of_bounds(hipStream_t st, const uint64_t *idx, size_t n, uint64_t bound, unsigned *bad);

}  // namespace tns
