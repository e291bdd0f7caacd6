// abi_host.cpp -- the entry points of include/tns.h that never touch the device: the last error,
// transcripts, verifiers, pairing and G2, the wire format, communicators, host conversions and
// the benchmark trace.
#include <thread>

#include "abi.hpp"

namespace tns {

static thread_local std::string g_last_error;
void set_last_error(const std::string &m) { g_last_error = m; }

// multi-threaded element-wise host conversion
template <class C, class F>
static void par_convert(const uint64_t *in, size_t n, uint64_t *out, F f) {
  unsigned nt = std::thread::hardware_concurrency();
  if (nt < 1) nt = 1;
  if (nt > 16) nt = 16;
  if (n < 4096) nt = 1;
  std::vector<std::thread> th;
  size_t per = (n + nt - 1) / nt;
  for (unsigned t = 0; t < nt; t++) {
    size_t a = t * per, b = std::min(n, a + per);
    if (a >= b) break;
    th.emplace_back([=]() {
      for (size_t i = a; i < b; i++) f(in, out, i);
    });
  }
  for (auto &x : th) x.join();
}

static G2Affine g2_from_limbs(const uint64_t in[16]) {
  G2Affine g;
  std::memcpy(&g.x0, in, 32);
  std::memcpy(&g.x1, in + 4, 32);
  std::memcpy(&g.y0, in + 8, 32);
  std::memcpy(&g.y1, in + 12, 32);
  g.inf = g.x0.is_zero() && g.x1.is_zero() && g.y0.is_zero() && g.y1.is_zero();
  if (!g.inf && !g2_on_curve(g)) throw Error(TNS_ERR_INVALID_PARAMETERS, "G2 point not on the twist");
  return g;
}
static G1Affine g1_from_limbs(const uint64_t in[8]) {
  G1Affine a;
  std::memcpy(&a.x, in, 32);
  std::memcpy(&a.y, in + 4, 32);
  if (!a.is_inf() && !g1_on_curve(a)) throw Error(TNS_ERR_INVALID_PARAMETERS, "G1 point not on the curve");
  return a;
}
Vk vk_load(const tns_vk *vk) { return Vk{g1_from_limbs(vk->g1), g2_from_limbs(vk->g2), g2_from_limbs(vk->g2_tau)}; }

}  // namespace tns

using namespace tns;

extern "C" {

const char *tns_last_error(void) { return g_last_error.c_str(); }

int tns_commitment_hash(const uint64_t proj[12], uint64_t out[4]) {
  return guarded([&]() {
    Fr h = commitment_hash(proj_to_affine_host(proj));
    std::memcpy(out, &h, 32);
    return TNS_OK;
  });
}

tns_transcript *tns_transcript_new(const uint8_t seed[32]) {
  (void)seed;  // src/utils.rs:141-147: the seeded rng is replaced before first use
  return new tns_transcript();
}
void tns_transcript_free(tns_transcript *t) { delete t; }
void tns_transcript_append_field_element(tns_transcript *t, const uint8_t *label, size_t len, const uint64_t x[4]) {
  t->t.append_bytes(label, len);
  Fr f;
  std::memcpy(&f, x, 32);
  t->t.append_fr(f);
}
void tns_transcript_append_field_elements(tns_transcript *t, const uint8_t *label, size_t len,
                                          const uint64_t *xs, size_t n) {
  t->t.append_bytes(label, len);
  for (size_t i = 0; i < n; i++) {
    Fr f;
    std::memcpy(&f, xs + 4 * i, 32);
    t->t.append_fr(f);
  }
}
void tns_transcript_challenge_field_element(tns_transcript *t, const uint8_t *label, size_t len, uint64_t out[4]) {
  Fr r = t->t.challenge_bytes(label, len);
  std::memcpy(out, &r, 32);
}

// ---------------------------------------------------------------- verifiers (host)
static void g2_to_limbs(const G2Affine &g, uint64_t out[16]) {
  if (g.inf) {
    std::memset(out, 0, 128);
    return;
  }
  std::memcpy(out, &g.x0, 32);
  std::memcpy(out + 4, &g.x1, 32);
  std::memcpy(out + 8, &g.y0, 32);
  std::memcpy(out + 12, &g.y1, 32);
}
static Fr fr_load(const uint64_t x[4]) {
  Fr r;
  std::memcpy(&r, x, 32);
  return r;
}

static int verify_proof(const tns_vk *vk, const tns_proof *p, const char *l0, const char *l1, int *ok) {
  return guarded([&]() {
    const Vk k = vk_load(vk);
    if (p->num_rounds > TNS_MAX_ROUNDS || p->num_openings > 2) throw Error(TNS_ERR_INVALID_PARAMETERS, "malformed proof");
    G1Affine C[2] = {proj_to_affine_host(p->commitments[0]), proj_to_affine_host(p->commitments[1])};
    G1Affine pi[2] = {proj_to_affine_host(p->opening_proofs[0]), proj_to_affine_host(p->opening_proofs[1])};
    Fr vals[2] = {fr_load(p->final_evaluations[0]), fr_load(p->final_evaluations[1])};
    std::vector<Fr> rounds(4 * (size_t)(p->num_rounds ? p->num_rounds : 1));
    std::memcpy(rounds.data(), p->round_polynomials, 128 * (size_t)p->num_rounds);
    *ok = protocol_verify_host(k.g1, k.g2, k.g2_tau, l0, l1, C, rounds.data(), p->num_rounds,
                               fr_load(p->final_evaluation), p->num_openings, pi, vals)
              ? 1 : 0;
    return TNS_OK;
  });
}

int tns_verifier_key(const tns_params *params, tns_vk *out) {
  return guarded([&]() {
    G1Affine g1;
    G2Affine g2, g2t;
    verifier_key(fr_load(params->tau), &g1, &g2, &g2t);
    std::memcpy(out->g1, &g1, 64);
    g2_to_limbs(g2, out->g2);
    g2_to_limbs(g2t, out->g2_tau);
    return TNS_OK;
  });
}

int tns_kzg_verify(const tns_vk *vk, const uint64_t commitment_proj[12], const uint64_t z[4], const uint64_t value[4],
                   const uint64_t proof_proj[12], int *ok) {
  return guarded([&]() {
    const Vk k = vk_load(vk);
    *ok = kzg_verify_host(k.g1, k.g2, k.g2_tau, proj_to_affine_host(commitment_proj), fr_load(z), fr_load(value),
                          proj_to_affine_host(proof_proj))
              ? 1 : 0;
    return TNS_OK;
  });
}

int tns_kzg_batch_verify(const tns_vk *vk, size_t n, const uint64_t *commitments_proj, const uint64_t *points,
                         const uint64_t *values, const uint64_t *proofs_proj, int *ok) {
  return guarded([&]() {
    const Vk k = vk_load(vk);
    std::vector<G1Affine> C(n), pi(n);
    std::vector<Fr> z(n), v(n);
    for (size_t i = 0; i < n; i++) {
      C[i] = proj_to_affine_host(commitments_proj + 12 * i);
      pi[i] = proj_to_affine_host(proofs_proj + 12 * i);
      z[i] = fr_load(points + 4 * i);
      v[i] = fr_load(values + 4 * i);
    }
    *ok = kzg_batch_verify_host(k.g1, k.g2, k.g2_tau, n, C.data(), z.data(), v.data(), pi.data()) ? 1 : 0;
    return TNS_OK;
  });
}

int tns_twist_verify(const tns_vk *vk, const tns_proof *proof, int *ok) {
  return verify_proof(vk, proof, "address_commitment", "value_commitment", ok);
}

int tns_shout_verify(const tns_vk *vk, const tns_proof *proof, int *ok) {
  return verify_proof(vk, proof, "table_commitment", "index_commitment", ok);
}

// SumCheck::verify (src/sumcheck.rs:113-153)
int tns_sumcheck_verify(unsigned nv, const uint64_t claimed_sum[4], const uint64_t *rounds, size_t n_rounds,
                        const uint64_t final_eval[4], tns_transcript *transcript, uint64_t *challenges_out,
                        size_t *n_challenges_out, int *ok) {
  return guarded([&]() {
    if (!claimed_sum || !final_eval || !transcript || !ok || (n_rounds > 0 && !rounds))
      throw Error(TNS_ERR_INVALID_PARAMETERS, "null input or output array");
    if (n_rounds != nv) throw Error(TNS_ERR_SUMCHECK, "Proof has wrong number of rounds");  // :118-122
    std::vector<Fr> rd(4 * (size_t)nv + 1), chal((size_t)nv + 1);
    if (nv) std::memcpy((void *)rd.data(), rounds, sizeof(Fr) * 4 * (size_t)nv);
    unsigned nc = 0;
    const int v = sumcheck_replay_host(transcript->t, fr_load(claimed_sum), rd.data(), nv, fr_load(final_eval),
                                       chal.data(), &nc);
    if (challenges_out && nc) std::memcpy(challenges_out, chal.data(), sizeof(Fr) * nc);
    if (n_challenges_out) *n_challenges_out = nc;
    *ok = v == 0 ? 1 : 0;
    return TNS_OK;
  });
}

int tns_pairing(const uint64_t g1_affine[8], const uint64_t g2_affine[16], uint64_t out[48]) {
  return guarded([&]() {
    Fq e[12];
    pairing_value(g1_from_limbs(g1_affine), g2_from_limbs(g2_affine), e);
    std::memcpy(out, e, sizeof e);
    return TNS_OK;
  });
}

int tns_g2_mul(const uint64_t g2_affine[16], const uint64_t k[4], uint64_t out[16]) {
  return guarded([&]() {
    g2_to_limbs(g2_mul(g2_from_limbs(g2_affine), k), out);
    return TNS_OK;
  });
}

// ---------------------------------------------------------------- wire format (host)
int tns_g1_serialize(const uint64_t proj[12], int compressed, uint8_t *out) {
  return guarded([&]() {
    g1_serialize(proj_to_affine_host(proj), compressed != 0, out);
    return TNS_OK;
  });
}

int tns_g1_deserialize(const uint8_t *in, int compressed, uint64_t proj_out[12]) {
  return guarded([&]() {
    store_proj(g1_deserialize(in, compressed != 0, true), proj_out);
    return TNS_OK;
  });
}

namespace {
struct Writer {
  uint8_t *out;
  size_t cap, n = 0;
  void bytes(const uint8_t *p, size_t k) {
    if (out && n + k <= cap) std::memcpy(out + n, p, k);
    n += k;
  }
  void u64(uint64_t v) {
    uint8_t b[8];
    for (int i = 0; i < 8; i++) b[i] = (uint8_t)(v >> (8 * i));
    bytes(b, 8);
  }
};
struct Reader {
  const uint8_t *in;
  size_t len, n = 0;
  const uint8_t *take(size_t k) {
    if (n + k > len) throw Error(TNS_ERR_INVALID_PARAMETERS, "truncated proof bytes");
    const uint8_t *p = in + n;
    n += k;
    return p;
  }
  uint64_t u64() {
    const uint8_t *b = take(8);
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) v |= (uint64_t)b[i] << (8 * i);
    return v;
  }
};
}  // namespace

int tns_proof_serialize(const tns_proof *p, int compressed, uint8_t *out, size_t cap, size_t *len) {
  return guarded([&]() {
    const size_t gs = compressed ? 32 : 64;
    Writer w{out, cap};
    uint8_t g[64], f[32];
    for (int i = 0; i < 2; i++) {
      g1_serialize(proj_to_affine_host(p->commitments[i]), compressed != 0, g);
      w.bytes(g, gs);
    }
    w.u64(p->num_rounds);
    for (uint32_t r = 0; r < p->num_rounds; r++) {
      w.u64(4);
      for (int x = 0; x < 4; x++) {
        fr_serialize(fr_load(p->round_polynomials[r][x]), f);
        w.bytes(f, 32);
      }
    }
    fr_serialize(fr_load(p->final_evaluation), f);
    w.bytes(f, 32);
    w.u64(p->num_openings);
    for (uint32_t i = 0; i < p->num_openings; i++) {
      g1_serialize(proj_to_affine_host(p->opening_proofs[i]), compressed != 0, g);
      w.bytes(g, gs);
    }
    w.u64(p->num_openings);  // final_evaluations has one value per opening
    for (uint32_t i = 0; i < p->num_openings; i++) {
      fr_serialize(fr_load(p->final_evaluations[i]), f);
      w.bytes(f, 32);
    }
    *len = w.n;
    if (out && w.n > cap) throw Error(TNS_ERR_INVALID_PARAMETERS, "output buffer too small");
    return TNS_OK;
  });
}

int tns_proof_deserialize(const uint8_t *in, size_t len, int compressed, tns_proof *p) {
  return guarded([&]() {
    std::memset(p, 0, sizeof *p);
    const size_t gs = compressed ? 32 : 64;
    Reader r{in, len};
    for (int i = 0; i < 2; i++) store_proj(g1_deserialize(r.take(gs), compressed != 0, true), p->commitments[i]);
    const uint64_t nr = r.u64();
    if (nr > TNS_MAX_ROUNDS) throw Error(TNS_ERR_INVALID_PARAMETERS, "too many sum-check rounds");
    p->num_rounds = (uint32_t)nr;
    for (uint64_t k = 0; k < nr; k++) {
      if (r.u64() != 4) throw Error(TNS_ERR_INVALID_PARAMETERS, "round polynomial must have 4 coefficients");
      for (int x = 0; x < 4; x++) {
        const Fr v = fr_deserialize(r.take(32));
        std::memcpy(p->round_polynomials[k][x], &v, 32);
      }
    }
    const Fr fe = fr_deserialize(r.take(32));
    std::memcpy(p->final_evaluation, &fe, 32);
    const uint64_t no = r.u64();
    if (no > 2) throw Error(TNS_ERR_INVALID_PARAMETERS, "more than two opening proofs");
    p->num_openings = (uint32_t)no;
    for (uint64_t i = 0; i < no; i++) store_proj(g1_deserialize(r.take(gs), compressed != 0, true), p->opening_proofs[i]);
    const uint64_t nf = r.u64();
    if (nf != no) throw Error(TNS_ERR_INVALID_PARAMETERS, "final evaluations do not match the openings");
    for (uint64_t i = 0; i < nf; i++) {
      const Fr v = fr_deserialize(r.take(32));
      std::memcpy(p->final_evaluations[i], &v, 32);
    }
    if (r.n != len) throw Error(TNS_ERR_INVALID_PARAMETERS, "trailing bytes after the proof");
    return TNS_OK;
  });
}

// ---------------------------------------------------------------- communicators
int tns_comm_unique_id(uint8_t uid[128]) {
  return guarded([&]() {
    comm_unique_id(uid);
    return TNS_OK;
  });
}

int tns_comm_create(tns_ctx *ctx, int rank, int size, const uint8_t uid[128], tns_comm **out) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    tns_comm *cm = new tns_comm();
    try {
      cm->c = comm_rccl_new(&ctx->c, rank, size, uid);
    } catch (...) {
      delete cm;
      throw;
    }
    *out = cm;
    return TNS_OK;
  });
}

int tns_comm_create_callback(int rank, int size, tns_allgather_fn fn, void *user, tns_comm **out) {
  return guarded([&]() {
    tns_comm *cm = new tns_comm();
    try {
      cm->c = comm_callback_new(rank, size, fn, user);
    } catch (...) {
      delete cm;
      throw;
    }
    *out = cm;
    return TNS_OK;
  });
}

void tns_comm_destroy(tns_comm *comm) { delete comm; }

int tns_comm_info(const tns_comm *comm, int *rank, int *size, int *seen_size, int *kind) {
  return guarded([&]() {
    if (!comm || !comm->c) throw Error(TNS_ERR_INVALID_PARAMETERS, "null communicator");
    if (rank) *rank = comm->c->rank;
    if (size) *size = comm->c->size;
    if (seen_size) *seen_size = comm->c->seen_size();
    if (kind) *kind = comm->c->kind();
    return TNS_OK;
  });
}

int tns_comm_allgather(tns_ctx *ctx, tns_comm *comm, const void *send, size_t bytes, void *recv) {
  return guarded([&]() {
    if (!comm || !comm->c) throw Error(TNS_ERR_INVALID_PARAMETERS, "null communicator");
    if (bytes && (!send || !recv)) throw Error(TNS_ERR_INVALID_PARAMETERS, "null exchange buffer");
    comm->c->exchange(ctx ? &ctx->c : nullptr, send, bytes, recv, "tns_comm_allgather");
    return TNS_OK;
  });
}

int tns_comm_set_timeout(tns_comm *comm, double seconds) {
  return guarded([&]() {
    if (!comm || !comm->c) throw Error(TNS_ERR_INVALID_PARAMETERS, "null communicator");
    if (!(seconds > 0.0)) throw Error(TNS_ERR_INVALID_PARAMETERS, "timeout must be positive");
    comm->c->timeout_s = seconds;
    return TNS_OK;
  });
}

int tns_comm_stats_ex(const tns_comm *comm, double out[6]) {
  return guarded([&]() {
    if (!comm || !comm->c || !out) throw Error(TNS_ERR_INVALID_PARAMETERS, "null communicator or output");
    out[0] = (double)comm->c->seq;
    out[1] = comm->c->total_s;
    out[2] = comm->c->max_s;
    out[3] = comm->c->timeout_s;
    out[4] = comm->c->bytes_total;
    out[5] = comm->c->bytes_max;
    return TNS_OK;
  });
}

int tns_comm_stats(const tns_comm *comm, double out[4]) {
  return guarded([&]() {
    if (!comm || !comm->c || !out) throw Error(TNS_ERR_INVALID_PARAMETERS, "null communicator or output");
    out[0] = (double)comm->c->seq;
    out[1] = comm->c->total_s;
    out[2] = comm->c->max_s;
    out[3] = comm->c->timeout_s;
    return TNS_OK;
  });
}

// n draws of ark-ff UniformRand for Fr from one ChaCha20Rng::from_seed(seed) stream (host)
void tns_fr_rand_batch(const uint8_t seed[32], size_t n, uint64_t *out_mont) {
  host_fr_rand_stream(seed, n, (Fr *)out_mont);
}

// the challenges of tns_kzg_verify_many / tns_vc_verify_all (kzg_verify.hip), on the host
void tns_verify_challenges(const uint8_t seed[32], uint64_t first, size_t count, uint64_t *out_canonical) {
  verify_challenges_host(seed, first, count, out_canonical);
}

// ---------------------------------------------------------------- host utilities
void tns_fr_from_u64(const uint64_t *in, size_t n, uint64_t *out) {
  par_convert<FrCfg>(in, n, out, [](const uint64_t *i, uint64_t *o, size_t k) {
    Fr r = from_u64<FrCfg>(i[k]);
    std::memcpy(o + 4 * k, &r, 32);
  });
}
void tns_fr_from_canonical(const uint64_t *in, size_t n, uint64_t *out) {
  par_convert<FrCfg>(in, n, out, [](const uint64_t *i, uint64_t *o, size_t k) {
    Fr x;
    std::memcpy(&x, i + 4 * k, 32);
    reduce_once(x);
    Fr r = to_mont(x);
    std::memcpy(o + 4 * k, &r, 32);
  });
}
void tns_fr_to_canonical(const uint64_t *in, size_t n, uint64_t *out) {
  par_convert<FrCfg>(in, n, out, [](const uint64_t *i, uint64_t *o, size_t k) {
    Fr x;
    std::memcpy(&x, i + 4 * k, 32);
    Fr r = from_mont(x);
    std::memcpy(o + 4 * k, &r, 32);
  });
}
void tns_fq_to_canonical(const uint64_t *in, size_t n, uint64_t *out) {
  par_convert<FqCfg>(in, n, out, [](const uint64_t *i, uint64_t *o, size_t k) {
    Fq x;
    std::memcpy(&x, i + 4 * k, 32);
    Fq r = from_mont(x);
    std::memcpy(o + 4 * k, &r, 32);
  });
}

// ProtocolBenchmarks trace (src/benchmarks.rs:88-99), operations [first, first + count) of
// an n_total-operation run (the memory state is replayed from operation 0)
static void bench_trace_core(size_t memory_size, uint64_t n_total, uint64_t first, size_t count, uint64_t *addr,
                             uint64_t *value, uint8_t *is_write) {
  if (memory_size == 0 || (memory_size & (memory_size - 1)))
    throw Error(TNS_ERR_INVALID_PARAMETERS, "Memory size must be power of 2");
  if (first + count > n_total) throw Error(TNS_ERR_INVALID_PARAMETERS, "slice beyond the trace");
  std::vector<uint64_t> mem(memory_size, 0);
  for (uint64_t i = 0; i < first + count; i++) {
    const bool out = i >= first;
    if (i % 3 == 0) {
      const size_t a = i % memory_size;
      mem[a] = i * 42;
      if (out) {
        addr[i - first] = a;
        value[i - first] = mem[a];
        is_write[i - first] = 1;
      }
    } else if (out) {
      const size_t a = (i / 2) % memory_size;
      addr[i - first] = a;
      value[i - first] = mem[a];
      is_write[i - first] = 0;
    }
  }
}

int tns_bench_trace(size_t memory_size, size_t n_ops, uint64_t *addr, uint64_t *value, uint8_t *is_write) {
  return guarded([&]() {
    bench_trace_core(memory_size, n_ops, 0, n_ops, addr, value, is_write);
    return TNS_OK;
  });
}

int tns_bench_trace_slice(size_t memory_size, uint64_t n_total, uint64_t first, size_t count, uint64_t *addr,
                          uint64_t *value, uint8_t *is_write) {
  return guarded([&]() {
    bench_trace_core(memory_size, n_total, first, count, addr, value, is_write);
    return TNS_OK;
  });
}

}  // extern "C"
