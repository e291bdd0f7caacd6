// api.hip -- the device-side C ABI of include/tns.h: device info, contexts, setup, SRS and SRS files, the KZG /
// MSM / interpolation / MLE entry points, device buffers, the clock probe and the profiler
// read-out.  (The provers are in prove.hip, the host-only entry points in abi_host.cpp.)
#include "abi.hpp"

namespace tns {

Ctx::~Ctx() {
  if (lanes[1].stream) (void)hipStreamDestroy(lanes[1].stream);
  if (side) (void)hipStreamDestroy(side);
  if (copy) (void)hipStreamDestroy(copy);
  if (acc) (void)hipStreamDestroy(acc);
  for (hipEvent_t e : stage_ev)
    if (e) (void)hipEventDestroy(e);
  if (stream) (void)hipStreamDestroy(stream);
}

}  // namespace tns

using namespace tns;

extern "C" {

int tns_version(void) { return 100; }
int tns_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int tns_device_info_get(int device, tns_device_info *out) {
  return guarded([&]() {
    if (!out) throw Error(TNS_ERR_INVALID_PARAMETERS, "null output");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
      throw Error(TNS_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) throw Error(TNS_ERR_INVALID_PARAMETERS, "device index out of range");
    hipDeviceProp_t p;
    TNS_HIP(hipGetDeviceProperties(&p, device));
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->name, sizeof(out->name), "%s", p.name);
    std::snprintf(out->arch, sizeof(out->arch), "%s", p.gcnArchName);
    std::snprintf(out->pci_bus_id, sizeof(out->pci_bus_id), "%04x:%02x:%02x.0", p.pciDomainID, p.pciBusID,
                  p.pciDeviceID);
    out->clock_khz = p.clockRate;
    out->mem_clock_khz = p.memoryClockRate;
    out->cu_count = p.multiProcessorCount;
    out->total_mem = p.totalGlobalMem;
    return TNS_OK;
  });
}

// The context's five streams.  Created in this order: with GPU_MAX_HW_QUEUES = 4 (HIP's default)
// the fifth stream shares the first one's hardware queue, and the copy stream (drop-in uploads,
// during the commitments) and the accumulation stream (only in the openings of a drop-in proof)
// are never busy together -- the copy stream on the context stream's queue serialised the upload
// behind the commitments (+1.4 ms per drop-in C4 step, profiles/r06_ab_stream_priority.txt).
// prio: the accumulations at the least priority and the context stream (lane 0) at the greatest,
// lane 1 / side / copy normal -- lane 1's last sort passes then wait for the first accumulation's
// tail-off instead of running beside it (-0.3-0.45 ms per C4 step); off for processes sharing a
// GPU, whose least-priority queues starve behind the other processes' (TNS_CTX_NO_STREAM_PRIORITIES;
// chosen at creation: streams recreated without priorities in the same process kept the pathology).
static void create_streams(Ctx &c, bool prio) {
  int lo = 0, hi = 0;
  TNS_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
  if (!prio) lo = hi = 0;
  auto mk = [](hipStream_t *s, int p) {
    TNS_HIP(p ? hipStreamCreateWithPriority(s, hipStreamNonBlocking, p) : hipStreamCreateWithFlags(s, hipStreamNonBlocking));
  };
  mk(&c.acc, lo);
  mk(&c.stream, hi);
  c.lanes[0].stream = c.stream;
  mk(&c.lanes[1].stream, 0);
  mk(&c.side, 0);
  mk(&c.copy, 0);
}

int tns_ctx_create(int device, tns_ctx **out) { return tns_ctx_create_ex(device, 0, out); }

int tns_ctx_create_ex(int device, unsigned flags, tns_ctx **out) {
  return guarded([&]() {
    if (flags & ~TNS_CTX_NO_STREAM_PRIORITIES) throw Error(TNS_ERR_INVALID_PARAMETERS, "unknown context flags");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
      throw Error(TNS_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) throw Error(TNS_ERR_INVALID_PARAMETERS, "device index out of range");
    TNS_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    TNS_HIP(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
      throw Error(TNS_ERR_NO_DEVICE, std::string("libtns is built for gfx950, device is ") + prop.gcnArchName);
    tns_ctx *x = new tns_ctx();
    x->c.device = device;
    x->c.num_cu = prop.multiProcessorCount;
    try {
      create_streams(x->c, !(flags & TNS_CTX_NO_STREAM_PRIORITIES));
    } catch (...) {
      delete x;
      throw;
    }
    *out = x;
    return TNS_OK;
  });
}

void tns_ctx_destroy(tns_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->c.device);
  (void)hipStreamSynchronize(ctx->c.stream);
  if (ctx->c.side) (void)hipStreamSynchronize(ctx->c.side);
  if (ctx->c.acc) (void)hipStreamSynchronize(ctx->c.acc);
  delete ctx;
}

int tns_ctx_synchronize(tns_ctx *ctx) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    for (hipStream_t s : {ctx->c.stream, ctx->c.lanes[1].stream, ctx->c.side, ctx->c.acc, ctx->c.copy})
      TNS_HIP(hipStreamSynchronize(s));
    return TNS_OK;
  });
}

// setup_params (src/utils.rs:79-131) for ranks [rank] of [size]: the SRS holds the
// contiguous share [first, first + held) of the num_powers g1_powers (all of them for size 1)
static void setup_core(tns_ctx *ctx, unsigned log_size, int rank, int size, tns_params *out, tns_srs **srs_out) {
  if (log_size > 26) throw Error(TNS_ERR_INVALID_PARAMETERS, "log_size too large");
  if (size < 1 || rank < 0 || rank >= size) throw Error(TNS_ERR_INVALID_PARAMETERS, "bad shard");
  std::memset(out, 0, sizeof *out);
  out->log_size = log_size;
  out->max_operations = (uint64_t)1 << (log_size + 2);  // src/utils.rs:80
  out->num_powers = next_pow2(out->max_operations) + 1;  // src/utils.rs:89
  uint8_t seed42[32];
  std::memset(seed42, 42, 32);
  Fr tau = host_fr_rand_chacha(seed42, out->fiat_shamir_seed);  // src/utils.rs:81-84, 101-102
  std::memcpy(out->tau, &tau, 32);
  if (!srs_out) return;
  *srs_out = nullptr;
  CtxScope g(&ctx->c);
  tns_srs *s = new tns_srs();
  s->s.device = ctx->c.device;
  s->s.n = out->num_powers;
  // shares of the 2^k + 1 powers: [r 2^k/size, (r + 1) 2^k/size), the last rank also holding
  // g1_powers[2^k] -- so rank r's share covers the coefficient slice of tns_shard_slice
  // (tns_msm_sharded); any other count splits as evenly as possible
  const size_t m = s->s.n - 1;
  if (m % (size_t)size == 0 && m >= (size_t)size) {
    s->s.first = (size_t)rank * (m / size);
    s->s.held = m / size + (rank == size - 1 ? 1 : 0);
  } else {
    const size_t base = s->s.n / size, rem = s->s.n % size;
    s->s.first = (size_t)rank * base + std::min<size_t>(rank, rem);
    s->s.held = base + ((size_t)rank < rem ? 1 : 0);
  }
  s->s.has_tau = true;
  s->s.tau = tau;
  try {
    G1Affine *pts = (G1Affine *)s->s.points.ensure(sizeof(G1Affine) * (s->s.held ? s->s.held : 1));
    srs_generate_dev(&ctx->c, tau, s->s.first, s->s.held, pts);
  } catch (...) {
    delete s;
    throw;
  }
  *srs_out = s;
}

int tns_setup_params(tns_ctx *ctx, unsigned log_size, tns_params *out, tns_srs **srs_out) {
  return guarded([&]() {
    setup_core(ctx, log_size, 0, 1, out, srs_out);
    return TNS_OK;
  });
}

int tns_setup_params_shard(tns_ctx *ctx, unsigned log_size, int rank, int size, tns_params *out,
                           tns_srs **srs_out) {
  return guarded([&]() {
    setup_core(ctx, log_size, rank, size, out, srs_out);
    return TNS_OK;
  });
}

int tns_srs_upload(tns_ctx *ctx, const uint64_t *g1, size_t n, tns_srs **out) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    tns_srs *s = new tns_srs();
    s->s.device = ctx->c.device;
    s->s.n = n;
    s->s.held = n;
    try {
      void *p = s->s.points.ensure(sizeof(G1Affine) * (n ? n : 1));
      if (n) TNS_HIP(hipMemcpy(p, g1, sizeof(G1Affine) * n, hipMemcpyHostToDevice));
    } catch (...) {
      delete s;
      throw;
    }
    *out = s;
    return TNS_OK;
  });
}

int tns_srs_download(tns_ctx *ctx, const tns_srs *srs, uint64_t *g1_out, size_t n) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    if (srs->s.first != 0 || n > srs->s.held) throw Error(TNS_ERR_INVALID_PARAMETERS, "download beyond SRS length");
    if (n) TNS_HIP(hipMemcpy(g1_out, srs->s.points.p, sizeof(G1Affine) * n, hipMemcpyDeviceToHost));
    return TNS_OK;
  });
}

int tns_srs_download_indices(tns_ctx *ctx, const tns_srs *srs, const uint64_t *idx, size_t k,
                             uint64_t *g1_out) {
  return guarded([&]() {
    if (!ctx || !srs) throw Error(TNS_ERR_INVALID_PARAMETERS, "null context or SRS");
    if (k > 0 && (!idx || !g1_out)) throw Error(TNS_ERR_INVALID_PARAMETERS, "null index or output buffer");
    CtxScope g(&ctx->c);
    for (size_t t = 0; t < k; t++)
      if (idx[t] < srs->s.first || idx[t] >= srs->s.first + srs->s.held)
        throw Error(TNS_ERR_INVALID_PARAMETERS, "SRS index outside this SRS's share");
    const G1Affine *pts = srs->s.points.as<G1Affine>();
    for (size_t t = 0; t < k; t++)
      TNS_HIP(hipMemcpyAsync(g1_out + 8 * t, pts + (idx[t] - srs->s.first), sizeof(G1Affine), hipMemcpyDeviceToHost,
                             ctx->c.stream));
    TNS_HIP(hipStreamSynchronize(ctx->c.stream));
    return TNS_OK;
  });
}

int tns_srs_share(const tns_srs *srs, uint64_t *first, uint64_t *held) {
  return guarded([&]() {
    if (!srs || !first || !held) throw Error(TNS_ERR_INVALID_PARAMETERS, "null SRS or output");
    *first = srs->s.first;
    *held = srs->s.held;
    return TNS_OK;
  });
}

size_t tns_srs_len(const tns_srs *srs) { return srs ? srs->s.n : 0; }

int tns_srs_set_tau(tns_srs *srs, const uint64_t tau[4]) {
  return guarded([&]() {
    if (!srs) throw Error(TNS_ERR_INVALID_PARAMETERS, "null SRS");
    Fr t;
    std::memcpy(&t, tau, 32);
    // The Lagrange basis (every commitment and opening of the Lagrange route) is derived from
    // tau, so tau must be the trapdoor of the uploaded powers: one held point g1_powers[e]
    // (e = 1, or the shard's first index) is checked against tau^e * G1 on the host.  An SRS
    // holding no such point (only g1_powers[0] = G1) cannot contradict tau.
    const size_t e = srs->s.first ? srs->s.first : 1;
    if (e >= srs->s.first && e < srs->s.first + srs->s.held) {
      TNS_HIP(hipSetDevice(srs->s.device));
      G1Affine held;
      TNS_HIP(hipMemcpy(&held, srs->s.points.as<G1Affine>() + (e - srs->s.first), sizeof(G1Affine),
                        hipMemcpyDeviceToHost));
      const G1Affine want = xyzz_to_affine(g1_mul_host(g1_generator_host(), pow_u64(t, (u64)e)));
      if (!(held.x == want.x) || !(held.y == want.y))
        throw Error(TNS_ERR_INVALID_PARAMETERS, "tau does not match the SRS (g1_powers[e] != tau^e * G1)");
    }
    srs->s.lagrange.clear();
    srs->s.open_all.clear();  // (correlations of the bases just dropped)
    srs->s.tau = t;
    srs->s.has_tau = true;
    return TNS_OK;
  });
}

int tns_srs_prepare_lagrange(tns_ctx *ctx, tns_srs *srs, size_t n) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    if (!srs->s.has_tau) throw Error(TNS_ERR_INVALID_PARAMETERS, "SRS has no tau");
    if (n == 0 || (n & (n - 1))) throw Error(TNS_ERR_INVALID_PARAMETERS, "Lagrange basis size must be a power of two");
    const bool saved = ctx->c.lagrange_commit;
    ctx->c.lagrange_commit = true;
    const LagrangeBasis *b = lagrange_basis_dev(&ctx->c, srs->s, n, 0, n);
    ctx->c.lagrange_commit = saved;
    (void)b;  // nullptr only when tau is itself a node: the coefficient path is used then
    return TNS_OK;
  });
}

int tns_srs_prepare_lagrange_from_powers(tns_ctx *ctx, tns_srs *srs, size_t n) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    (void)lagrange_basis_from_powers_dev(&ctx->c, srs->s, n);
    return TNS_OK;
  });
}

int tns_srs_lagrange_download(tns_ctx *ctx, tns_srs *srs, size_t n, uint64_t *g1_affine_out) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    if (!srs->s.has_tau && !srs->s.lagrange.count(std::make_tuple(n, (size_t)0, n)))
      throw Error(TNS_ERR_INVALID_PARAMETERS, "SRS has no tau (and no basis prepared from its powers)");
    if (n == 0 || (n & (n - 1))) throw Error(TNS_ERR_INVALID_PARAMETERS, "Lagrange basis size must be a power of two");
    const bool saved = ctx->c.lagrange_commit;
    ctx->c.lagrange_commit = true;
    const LagrangeBasis *b = lagrange_basis_dev(&ctx->c, srs->s, n, 0, n);
    ctx->c.lagrange_commit = saved;
    if (!b) throw Error(TNS_ERR_INVALID_PARAMETERS, "tau is an interpolation node: no Lagrange basis");
    TNS_HIP(hipMemcpy(g1_affine_out, b->points.p, sizeof(G1Affine) * n, hipMemcpyDeviceToHost));
    return TNS_OK;
  });
}

// ---------------------------------------------------------------- SRS files (srs_io.hip)
size_t tns_srs_serialized_size(size_t n, int compressed) { return g1_vec_serialized_size(n, compressed != 0); }

static void check_whole_srs(const tns_ctx *ctx, const tns_srs *srs) {
  if (!ctx || !srs) throw Error(TNS_ERR_INVALID_PARAMETERS, "null context or SRS");
  if (srs->s.first != 0 || srs->s.held < srs->s.n)
    throw Error(TNS_ERR_INVALID_PARAMETERS, "SRS files hold all of g1_powers (this SRS is a shard)");
}

// n device points as a Vec<G1Affine> file, under tns_proof_serialize's buffer contract
static void serialize_points(tns_ctx *ctx, const G1Affine *pts, size_t n, int compressed, uint8_t *out, size_t cap,
                             size_t *len) {
  if (!len) throw Error(TNS_ERR_INVALID_PARAMETERS, "null length output");
  *len = g1_vec_serialized_size(n, compressed != 0);
  if (!out) return;
  if (*len > cap) throw Error(TNS_ERR_INVALID_PARAMETERS, "output buffer too small");
  g1_vec_put_header(n, out);
  g1_encode_dev(&ctx->c, pts, n, compressed != 0, out + 8);
}

int tns_srs_serialize(tns_ctx *ctx, const tns_srs *srs, int compressed, uint8_t *out, size_t cap, size_t *len) {
  return guarded([&]() {
    check_whole_srs(ctx, srs);
    CtxScope g(&ctx->c);
    serialize_points(ctx, srs->s.points.as<G1Affine>(), srs->s.n, compressed, out, cap, len);
    return TNS_OK;
  });
}

int tns_srs_deserialize(tns_ctx *ctx, const uint8_t *in, size_t len, int compressed, tns_srs **out) {
  return guarded([&]() {
    if (!ctx || !out) throw Error(TNS_ERR_INVALID_PARAMETERS, "null context or output");
    const size_t n = g1_vec_header(in, len, compressed != 0);
    CtxScope g(&ctx->c);
    tns_srs *s = new tns_srs();
    s->s.device = ctx->c.device;
    s->s.n = n;
    s->s.held = n;
    try {
      G1Affine *p = (G1Affine *)s->s.points.ensure(sizeof(G1Affine) * (n ? n : 1));
      g1_decode_dev(&ctx->c, in + 8, n, compressed != 0, p);
    } catch (...) {
      delete s;
      throw;
    }
    *out = s;
    return TNS_OK;
  });
}

int tns_srs_lagrange_serialize(tns_ctx *ctx, tns_srs *srs, size_t n, int compressed, uint8_t *out, size_t cap,
                               size_t *len) {
  return guarded([&]() {
    check_whole_srs(ctx, srs);
    CtxScope g(&ctx->c);
    if (!srs->s.has_tau && !srs->s.lagrange.count(std::make_tuple(n, (size_t)0, n)))
      throw Error(TNS_ERR_INVALID_PARAMETERS, "SRS has no tau (and no basis prepared from its powers)");
    if (n == 0 || (n & (n - 1))) throw Error(TNS_ERR_INVALID_PARAMETERS, "Lagrange basis size must be a power of two");
    serialize_points(ctx, nullptr, n, compressed, nullptr, 0, len);  // sizing alone builds nothing
    if (!out) return TNS_OK;
    if (*len > cap) throw Error(TNS_ERR_INVALID_PARAMETERS, "output buffer too small");
    const bool saved = ctx->c.lagrange_commit;
    ctx->c.lagrange_commit = true;
    const LagrangeBasis *b = lagrange_basis_dev(&ctx->c, srs->s, n, 0, n);
    ctx->c.lagrange_commit = saved;
    if (!b) throw Error(TNS_ERR_INVALID_PARAMETERS, "tau is an interpolation node: no Lagrange basis");
    serialize_points(ctx, b->points.as<G1Affine>(), n, compressed, out, cap, len);
    return TNS_OK;
  });
}

int tns_srs_lagrange_deserialize(tns_ctx *ctx, tns_srs *srs, const uint8_t *in, size_t len, int compressed,
                                 const uint8_t seed[32]) {
  return guarded([&]() {
    check_whole_srs(ctx, srs);
    const size_t n = g1_vec_header(in, len, compressed != 0);
    CtxScope g(&ctx->c);
    lagrange_basis_attach_dev(&ctx->c, srs->s, in + 8, n, compressed != 0, seed);
    return TNS_OK;
  });
}

int tns_ctx_set_msm_tables(tns_ctx *ctx, int on) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    ctx->c.msm_tables = on != 0;
    return TNS_OK;
  });
}

int tns_ctx_set_upload_chunks(tns_ctx *ctx, int chunks) {
  return guarded([&]() {
    if (!ctx) throw Error(TNS_ERR_INVALID_PARAMETERS, "null context");
    if (chunks < 1 || chunks > 64) throw Error(TNS_ERR_INVALID_PARAMETERS, "upload chunks must be 1..64");
    CtxScope g(&ctx->c);
    ctx->c.upload_chunks = chunks;
    return TNS_OK;
  });
}

int tns_ctx_set_commit_basis(tns_ctx *ctx, int lagrange) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    ctx->c.lagrange_commit = lagrange != 0;
    return TNS_OK;
  });
}
void tns_srs_destroy(tns_srs *srs) {
  if (!srs) return;
  (void)hipSetDevice(srs->s.device);
  delete srs;
}

int tns_kzg_commit(tns_ctx *ctx, const tns_srs *srs, const uint64_t *coeffs, size_t n, uint64_t out[12]) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    if (n > srs->s.n) throw Error(TNS_ERR_COMMITMENT, "Polynomial degree exceeds setup size");
    DevBuf d;
    Fr *dc = (Fr *)d.ensure(sizeof(Fr) * (n ? n : 1));
    if (n) TNS_HIP(hipMemcpyAsync(dc, coeffs, sizeof(Fr) * n, hipMemcpyHostToDevice, ctx->c.stream));
    store_proj(commit_dev(&ctx->c, srs->s, dc, n), out);
    return TNS_OK;
  });
}

static void upload_evals(tns_ctx *ctx, const uint64_t *evals, size_t n, DevBuf &d, DevBuf &cf, EvalPoly &p) {
  if (n == 0) throw Error(TNS_ERR_POLYNOMIAL, "empty evaluation vector");
  Fr *dy = (Fr *)d.ensure(sizeof(Fr) * n);
  TNS_HIP(hipMemcpyAsync(dy, evals, sizeof(Fr) * n, hipMemcpyHostToDevice, ctx->c.stream));
  p.y = dy;
  p.N = n;
  p.first = 0;
  p.cnt = n;
  p.coeffs = (Fr *)cf.ensure(sizeof(Fr) * n);
}

int tns_kzg_commit_evals(tns_ctx *ctx, const tns_srs *srs, const uint64_t *evals, size_t n, uint64_t out[12]) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    DevBuf d, cf;
    EvalPoly p;
    upload_evals(ctx, evals, n, d, cf, p);
    store_proj(commit_evals(&ctx->c, srs->s, p, comm_self()), out);
    return TNS_OK;
  });
}

int tns_kzg_open_evals(tns_ctx *ctx, const tns_srs *srs, const uint64_t *evals, size_t n, const uint64_t z[4],
                       uint64_t value[4], uint64_t proof[12]) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    DevBuf d, cf, s;
    EvalPoly p;
    upload_evals(ctx, evals, n, d, cf, p);
    if (n > srs->s.n) throw Error(TNS_ERR_COMMITMENT, "Polynomial degree exceeds setup size");
    p.basis = lagrange_basis_dev(&ctx->c, srs->s, n, 0, n);
    Fr zz, v;
    std::memcpy(&zz, z, 32);
    G1Affine pi;
    open_evals(&ctx->c, srs->s, p, zz, &v, &pi, s, comm_self());
    std::memcpy(value, &v, 32);
    store_proj(pi, proof);
    return TNS_OK;
  });
}

// KZGVectorCommitment (src/commitments.rs:408-483): commit = commit(interpolant of v on
// 0..n-1), any n; open at index i = KZG open at the node i (value v_i).
int tns_vc_open(tns_ctx *ctx, const tns_srs *srs, const uint64_t *vec, size_t n, size_t index, uint64_t value[4],
                uint64_t proof[12]) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    if (index >= n) throw Error(TNS_ERR_COMMITMENT, "Index out of bounds");
    DevBuf d, cf, s;
    EvalPoly p;
    upload_evals(ctx, vec, n, d, cf, p);
    if (n > srs->s.n) throw Error(TNS_ERR_COMMITMENT, "Polynomial degree exceeds setup size");
    p.basis = lagrange_basis_dev(&ctx->c, srs->s, n, 0, n);
    const Fr z = from_u64<FrCfg>((uint64_t)index);
    Fr v;
    G1Affine pi;
    open_evals(&ctx->c, srs->s, p, z, &v, &pi, s, comm_self());
    std::memcpy(value, &v, 32);
    store_proj(pi, proof);
    return TNS_OK;
  });
}

int tns_msm(tns_ctx *ctx, const tns_srs *srs, const uint64_t *scalars, size_t n, uint64_t out[12]) {
  return tns_kzg_commit(ctx, srs, scalars, n, out);
}

int tns_kzg_open(tns_ctx *ctx, const tns_srs *srs, const uint64_t *coeffs, size_t n, const uint64_t z[4],
                 uint64_t value[4], uint64_t proof[12]) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    DevBuf d, s;
    Fr *dc = (Fr *)d.ensure(sizeof(Fr) * (n ? n : 1));
    if (n) TNS_HIP(hipMemcpyAsync(dc, coeffs, sizeof(Fr) * n, hipMemcpyHostToDevice, ctx->c.stream));
    Fr zz, v;
    std::memcpy(&zz, z, 32);
    G1Affine pi;
    open_dev(&ctx->c, srs->s, dc, n, zz, &v, &pi, s);
    std::memcpy(value, &v, 32);
    store_proj(pi, proof);
    return TNS_OK;
  });
}

int tns_interpolate_consecutive(tns_ctx *ctx, const uint64_t *y, size_t n, uint64_t *coeffs) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    if (n == 0) return TNS_OK;
    DevBuf dy, dc;
    Fr *py = (Fr *)dy.ensure(sizeof(Fr) * n), *pc = (Fr *)dc.ensure(sizeof(Fr) * n);
    TNS_HIP(hipMemcpyAsync(py, y, sizeof(Fr) * n, hipMemcpyHostToDevice, ctx->c.stream));
    interpolate_consecutive_dev(&ctx->c, py, n, pc);
    TNS_HIP(hipMemcpyAsync(coeffs, pc, sizeof(Fr) * n, hipMemcpyDeviceToHost, ctx->c.stream));
    TNS_HIP(hipStreamSynchronize(ctx->c.stream));
    return TNS_OK;
  });
}

// The 2^nv-entry table of an MLE from the caller's n_evals entries: entries past n_evals are
// zero (the reference's evaluate sums over the entries it holds, src/polynomials.rs:91-102);
// more than 2^nv entries is rejected (callers fold aliases first).
static Fr *upload_mle(tns_ctx *ctx, const uint64_t *evals, size_t n_evals, unsigned nv, DevBuf &d) {
  if (nv > 30) throw Error(TNS_ERR_INVALID_PARAMETERS, "too many variables");
  const size_t n = (size_t)1 << nv;
  if (n_evals > n) throw Error(TNS_ERR_INVALID_PARAMETERS, "more evaluations than 2^num_vars");
  Fr *pe = (Fr *)d.ensure(sizeof(Fr) * n);
  if (n_evals) TNS_HIP(hipMemcpyAsync(pe, evals, sizeof(Fr) * n_evals, hipMemcpyHostToDevice, ctx->c.stream));
  if (n_evals < n) TNS_HIP(hipMemsetAsync(pe + n_evals, 0, sizeof(Fr) * (n - n_evals), ctx->c.stream));
  return pe;
}

int tns_mle_evaluate(tns_ctx *ctx, const uint64_t *evals, size_t n_evals, unsigned nv, const uint64_t *point,
                     uint64_t out[4]) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    DevBuf d;
    Fr *pe = upload_mle(ctx, evals, n_evals, nv, d);
    std::vector<Fr> pt(nv ? nv : 1);
    if (nv) std::memcpy(pt.data(), point, 32 * (size_t)nv);
    Fr r = mle_evaluate_dev(&ctx->c, pe, nv, pt.data());
    std::memcpy(out, &r, 32);
    return TNS_OK;
  });
}

int tns_mle_partial_evaluate(tns_ctx *ctx, const uint64_t *evals, size_t n_evals, unsigned nv,
                             const uint64_t *fixed, unsigned k, uint64_t *out) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    if (k > nv) throw Error(TNS_ERR_INVALID_PARAMETERS, "Cannot fix more variables than available");
    const size_t n = (size_t)1 << nv;
    DevBuf a, b;
    Fr *pa = upload_mle(ctx, evals, n_evals, nv, a);
    Fr *pb = (Fr *)b.ensure(sizeof(Fr) * (n / 2 + 1));
    Fr *src = pa, *dst = pb;
    for (unsigned j = 0; j < k; j++) {
      Fr r;
      std::memcpy(&r, fixed + 4 * (size_t)j, 32);
      mle_fold_dev(&ctx->c, src, dst, n >> (j + 1), r);
      std::swap(src, dst);
    }
    TNS_HIP(hipMemcpyAsync(out, src, sizeof(Fr) * (n >> k), hipMemcpyDeviceToHost, ctx->c.stream));
    TNS_HIP(hipStreamSynchronize(ctx->c.stream));
    return TNS_OK;
  });
}

int tns_last_prove_timing(tns_ctx *ctx, double out_ms[6]) {
  for (int i = 0; i < 6; i++) out_ms[i] = ctx->timing[i];
  return TNS_OK;
}

int tns_srs_prepare_lagrange_shard(tns_ctx *ctx, tns_srs *srs, size_t n, int rank, int size) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    if (!srs->s.has_tau) throw Error(TNS_ERR_INVALID_PARAMETERS, "SRS has no tau");
    if (n == 0 || (n & (n - 1))) throw Error(TNS_ERR_INVALID_PARAMETERS, "Lagrange basis size must be a power of two");
    if (size < 1 || (size & (size - 1)) || rank < 0 || rank >= size || (size_t)size > n)
      throw Error(TNS_ERR_INVALID_PARAMETERS, "bad shard");
    const bool saved = ctx->c.lagrange_commit;
    ctx->c.lagrange_commit = true;
    const size_t L = n / size;
    (void)lagrange_basis_dev(&ctx->c, srs->s, n, (size_t)rank * L, L);
    ctx->c.lagrange_commit = saved;
    return TNS_OK;
  });
}

// ---------------------------------------------------------------- device buffers
int tns_buffer_upload(tns_ctx *ctx, const void *host, size_t bytes, tns_buffer **out) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    tns_buffer *b = new tns_buffer();
    b->device = ctx->c.device;
    b->bytes = bytes;
    try {
      b->buf.ensure(bytes ? bytes : 16);
      if (bytes) TNS_HIP(hipMemcpy(b->buf.p, host, bytes, hipMemcpyHostToDevice));
    } catch (...) {
      delete b;
      throw;
    }
    *out = b;
    return TNS_OK;
  });
}
void *tns_buffer_device_ptr(const tns_buffer *b) { return b ? b->buf.p : nullptr; }
int tns_buffer_download(const tns_buffer *b, void *host, size_t bytes) {
  return guarded([&]() {
    if (!b || bytes > b->bytes) throw Error(TNS_ERR_INVALID_PARAMETERS, "download beyond the buffer");
    TNS_HIP(hipSetDevice(b->device));
    if (bytes) TNS_HIP(hipMemcpy(host, b->buf.p, bytes, hipMemcpyDeviceToHost));
    return TNS_OK;
  });
}
void tns_buffer_free(tns_buffer *b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  delete b;
}

int tns_msm_device(tns_ctx *ctx, const tns_srs *srs, const uint64_t *d_scalars, size_t n, uint64_t out[12]) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    store_proj(commit_dev(&ctx->c, srs->s, (const Fr *)d_scalars, n), out);
    return TNS_OK;
  });
}

int tns_msm_sharded(tns_ctx *ctx, const tns_srs *srs, tns_comm *comm, const uint64_t *d_scalars, size_t n_local,
                    uint64_t n_total, uint64_t out[12]) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    if (!comm || !comm->c) throw Error(TNS_ERR_INVALID_PARAMETERS, "null communicator");
    Comm &m = *comm->c;
    if (n_total > srs->s.n) throw Error(TNS_ERR_COMMITMENT, "Polynomial degree exceeds setup size");
    const size_t N = next_pow2((size_t)n_total);
    check_shard(m, N, "coefficient");
    const size_t L = N / (size_t)m.size, first = (size_t)m.rank * L;
    if (n_local != slice_count(n_total, first, L))
      throw Error(TNS_ERR_INVALID_PARAMETERS, "n_local is not this rank's slice of n_total");
    if (n_local && (first < srs->s.first || first + n_local > srs->s.first + srs->s.held))
      throw Error(TNS_ERR_INVALID_PARAMETERS, "this rank's SRS share does not hold its coefficient slice");
    const size_t off = first - std::min(first, srs->s.first);
    const FixedBase *fb = srs_fixed_base(&ctx->c, srs->s, n_local);
    const G1Xyzz part = n_local ? msm_dev(&ctx->c, srs->s.points.as<G1Affine>() + off, (const Fr *)d_scalars, n_local,
                                          fb, off)
                                : G1Xyzz::inf();
    store_proj(xyzz_to_affine(allgather_sum_g1(&ctx->c, m, part, "sharded MSM partial")), out);
    return TNS_OK;
  });
}

// ---------------------------------------------------------------- clock probe
// Every workgroup: a chain of `iters` Montgomery products per lane (the accumulation's
// instruction mix), bracketed by the shader-clock and constant 100 MHz counters.
__global__ void __launch_bounds__(256) k_clock_probe(uint32_t iters, uint32_t seed, uint64_t *__restrict__ out,
                                                     uint32_t *__restrict__ sink) {
  const uint64_t t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  Fq a, b;
#pragma unroll
  for (int l = 0; l < 8; l++) {
    a.v[l] = (seed + threadIdx.x * 0x9e3779b9u + l * 0x85ebca6bu) & (l == 7 ? 0x0fffffffu : 0xffffffffu);
    b.v[l] = (seed * 31u + blockIdx.x + l * 0xc2b2ae35u) & (l == 7 ? 0x0fffffffu : 0xffffffffu);
  }
  for (uint32_t i = 0; i < iters; i++) {
    a = mul(a, b);
    b = mul(b, a);
  }
  const uint64_t t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  if (a.v[0] == 0x12345678u && b.v[1] == 0x9abcdef0u) sink[0] = a.v[2];  // keep the chain live
  if (threadIdx.x == 0) {
    out[2 * blockIdx.x] = t1 - t0;
    out[2 * blockIdx.x + 1] = r1 - r0;
  }
}

int tns_clock_probe(tns_ctx *ctx, double ms, double out[4]) {
  return guarded([&]() {
    if (!ctx || !out || !(ms > 0.0)) throw Error(TNS_ERR_INVALID_PARAMETERS, "null context/output or ms <= 0");
    CtxScope g(&ctx->c);
    hipStream_t st = ctx->c.stream;
    int cus = 0;
    TNS_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->c.device));
    const unsigned nblk = (unsigned)std::max(1, cus) * 4;  // 4 waves per SIMD
    DevBuf dout, dsink;
    uint64_t *d = (uint64_t *)dout.ensure(sizeof(uint64_t) * 2 * nblk);
    uint32_t *sink = (uint32_t *)dsink.ensure(sizeof(uint32_t));
    Event e0(hipEventDefault), e1(hipEventDefault);
    auto run = [&](uint32_t iters) {
      TNS_HIP(hipEventRecord(e0, st));
      k_clock_probe<<<nblk, 256, 0, st>>>(iters, 0x1234567u, d, sink);
      TNS_LAUNCH_CHECK();
      TNS_HIP(hipEventRecord(e1, st));
      TNS_HIP(hipEventSynchronize(e1));
      float t = 0.f;
      TNS_HIP(hipEventElapsedTime(&t, e0, e1));
      return (double)t;
    };
    uint32_t iters = 256;
    double t = run(iters);
    while (t < ms / 4 && iters < (1u << 26)) {  // calibrate to about `ms`
      iters = (uint32_t)std::min<double>((double)(1u << 26), iters * std::max(2.0, 0.5 * ms / std::max(t, 1e-3)));
      t = run(iters);
    }
    if (t < ms) t = run((uint32_t)std::min<double>((double)(1u << 30), iters * ms / std::max(t, 1e-3)));
    std::vector<uint64_t> h(2 * nblk);
    TNS_HIP(hipMemcpy(h.data(), d, sizeof(uint64_t) * 2 * nblk, hipMemcpyDeviceToHost));
    std::vector<double> mhz;
    for (unsigned b = 0; b < nblk; b++)
      if (h[2 * b + 1]) mhz.push_back(100.0 * (double)h[2 * b] / (double)h[2 * b + 1]);
    if (mhz.empty()) throw Error(TNS_ERR_DEVICE, "clock probe: no workgroup reported");
    std::sort(mhz.begin(), mhz.end());
    out[0] = mhz[mhz.size() / 2];
    out[1] = mhz.front();
    out[2] = mhz.back();
    out[3] = t;
    return TNS_OK;
  });
}

// ---------------------------------------------------------------- kernel timing (HIP events)
int tns_profile_enable(tns_ctx *ctx, int on) {
  ctx->c.prof.enabled = on != 0;
  ctx->c.prof.only.clear();  // a new profile times every stage until tns_profile_only narrows it
  ctx->c.prof.start(ctx->c.stream);
  return TNS_OK;
}

int tns_profile_only(tns_ctx *ctx, const char *stage) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    ctx->c.prof.only = stage ? stage : "";
    return TNS_OK;
  });
}

int tns_profile_read_ex(tns_ctx *ctx, const char *stage, double out[5]) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    ctx->c.prof.collect();
    auto it = ctx->c.prof.totals.find(stage);
    const bool f = it != ctx->c.prof.totals.end();
    out[0] = f ? it->second.ms : 0.0;
    out[1] = f ? (double)it->second.launches : 0.0;
    out[2] = f ? it->second.bytes : 0.0;
    out[3] = f ? it->second.ops : 0.0;
    out[4] = f ? it->second.busy_ms : 0.0;
    return TNS_OK;
  });
}
int tns_profile_read(tns_ctx *ctx, const char *kernel, double *total_ms, uint64_t *launches, double *alg_bytes) {
  return guarded([&]() {
    CtxScope g(&ctx->c);
    ctx->c.prof.collect();
    auto it = ctx->c.prof.totals.find(kernel);
    bool f = it != ctx->c.prof.totals.end();
    *total_ms = f ? it->second.ms : 0.0;
    *launches = f ? it->second.launches : 0;
    *alg_bytes = f ? it->second.bytes : 0.0;
    return TNS_OK;
  });
}

}  // extern "C"
