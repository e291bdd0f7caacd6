// vc_open.hip -- every opening of a KZG vector commitment in one pass.
//
// KZGVectorCommitment::open (src/commitments.rs:435-471) opens one index a call: the quotient
// q_i = (f - v_i) / (x - i) of the vector's interpolant f on the nodes 0..n-1, committed as
// pi_i = [q_i(tau)]G.  n calls are n MSMs of n points.  All n proofs together are three correlations:
// with the Lagrange basis Lambda_j = [L_j(tau)]G, the barycentric weights w_j and t_d = 1 / d
// (t_0 = 0), q_i has degree <= n - 2, so pi_i = sum_j q_i(j) Lambda_j with
// q_i(j) = (v_j - v_i) / (j - i) at j != i and q_i(i) = f'(i):
//
//   pi_i  = B_i - v_i A_i + f'(i) Lambda_i
//   B_i   = sum_j t_{j-i} (v_j Lambda_j)         a group correlation, of the vector
//   A_i   = sum_j t_{j-i} Lambda_j               a group correlation, of (SRS, n) alone: cached
//   f'(i) = (1 / w_i) (sum_j t_{i-j} w_j v_j  -  v_i sum_j t_{i-j} w_j)
//
// All four sums are cyclic convolutions of length M = next_pow2(2 n - 1) with ONE kernel,
// c_d = -1 / d, c_{M-d} = 1 / d (0 < d < n), zero elsewhere: (x * c)_i = sum_j x_j c_{i-j} =
// sum_j t_{j-i} x_j, and i - j never wraps.  The group ones run on tfree.hip's group NTT (forward,
// the spectrum of c as canonical scalars pointwise, inverse), the scalar ones on its radix-2 Fr NTT,
// whose index order is the same.  Per call: n + M + 2 n variable-base scalar multiplications around
// M log M butterfly ones -- O(n log n) for any n, no power of two required.
#include "abi.hpp"
#include "group_ntt.hpp"
#include "ntt.hpp"

namespace tns {

namespace {

// c (see above) on [0, M); 1 / d = (d - 1)! / d! from the factorial tables (entries < n)
__global__ void __launch_bounds__(256) k_vo_kernel(const Fr *__restrict__ fact, const Fr *__restrict__ ifact, size_t n,
                                                   size_t M, Fr *__restrict__ ck) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < M; i += (size_t)gridDim.x * blockDim.x) {
    Fr r = Fr::zero();
    if (i != 0 && i < n) r = neg(mul(fact[i - 1], ifact[i]));
    if (i + n > M) r = mul(fact[M - i - 1], ifact[M - i]);  // i = M - d, 0 < d < n (2 d < M: no overlap)
    ck[i] = r;
  }
}

__global__ void __launch_bounds__(256) k_vo_scale(Fr *__restrict__ S, size_t M, Fr s) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < M; i += (size_t)gridDim.x * blockDim.x)
    S[i] = mul(S[i], s);
}

// u_j = w_j v_j (v == nullptr: w_j) zero-padded to M
__global__ void __launch_bounds__(256) k_vo_weighted(const Fr *__restrict__ w, const Fr *__restrict__ v, size_t n,
                                                     size_t M, Fr *__restrict__ u) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < M; i += (size_t)gridDim.x * blockDim.x)
    u[i] = i < n ? (v ? mul(w[i], v[i]) : w[i]) : Fr::zero();
}

__global__ void __launch_bounds__(256) k_vo_fr_pointwise(Fr *__restrict__ X, const Fr *__restrict__ S, size_t M) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < M; i += (size_t)gridDim.x * blockDim.x)
    X[i] = mul(X[i], S[i]);
}

// iw_i = 1 / w_i = (-1)^(n-1-i) i! (n-1-i)!,  D_i = (1 / w_i) sum_j t_{i-j} w_j = -iw_i (w * c)_i
__global__ void __launch_bounds__(256) k_vo_plan_scalars(const Fr *__restrict__ fact, const Fr *__restrict__ Wc,
                                                         size_t n, Fr *__restrict__ iw, Fr *__restrict__ D) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const Fr x = mul(fact[i], fact[n - 1 - i]);
    const Fr r = ((n - 1 - i) & 1) ? neg(x) : x;
    iw[i] = r;
    D[i] = neg(mul(r, Wc[i]));
  }
}

// X_j = s_j Lambda_j in XYZZ (v == nullptr: Lambda_j itself), j < n
__global__ void __launch_bounds__(256, TF_WAVES) k_vo_points(const G1Affine *__restrict__ L, const Fr *__restrict__ v,
                                                             size_t n, G1Xyzz *__restrict__ X) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const G1Xyzz p = xyzz_from_affine(L[i]);
    X[i] = v ? xyzz_mul_canon(p, from_mont(v[i])) : p;
  }
}
// the zero padding X[n..M)
__global__ void __launch_bounds__(256) k_vo_pad(G1Xyzz *__restrict__ X, size_t n, size_t M) {
  for (size_t i = n + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < M; i += (size_t)gridDim.x * blockDim.x)
    X[i] = G1Xyzz::inf();
}

// X^_k *= c^_k / M (the spectra in the group NTT's bit-reversed order)
__global__ void __launch_bounds__(256, TF_WAVES) k_vo_pointwise(G1Xyzz *__restrict__ X, const Fr *__restrict__ S,
                                                                size_t M) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < M; i += (size_t)gridDim.x * blockDim.x)
    X[i] = xyzz_mul_canon(X[i], from_mont(S[i]));
}

// pi_i = B_i - v_i A_i + f'(i) Lambda_i in place of B_i;  f'(i) = -iw_i U_i - v_i D_i, U = (w v) * c
__global__ void __launch_bounds__(256, TF_WAVES) k_vo_combine(G1Xyzz *__restrict__ X, const G1Affine *__restrict__ A,
                                                              const G1Affine *__restrict__ L, const Fr *__restrict__ v,
                                                              const Fr *__restrict__ U, const Fr *__restrict__ iw,
                                                              const Fr *__restrict__ D, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const Fr vi = v[i];
    const Fr fp = neg(add(mul(iw[i], U[i]), mul(vi, D[i])));
    G1Xyzz acc = xyzz_add(X[i], xyzz_mul_canon(xyzz_from_affine(A[i]), from_mont(neg(vi))));
    acc = xyzz_add(acc, xyzz_mul_canon(xyzz_from_affine(L[i]), from_mont(fp)));
    X[i] = acc;
  }
}

// the twiddles of transforms up to 2^L, plain (returned) and split for the group NTT (*TG)
const Fr *transform_tables(Ctx *c, unsigned L, const GlvScalar **TG) {
  const Fr *TW = ntt_twiddles(c, L);
  if (c->glv_tw_log < L || !c->glv_tw.p) {
    glv_twiddles(c, TW, (size_t)1 << L, c->glv_tw);  // (stage-major: the table of L serves every smaller one)
    c->glv_tw_log = L;
  }
  *TG = c->glv_tw.as<GlvScalar>();
  return TW;
}

// X <- X * c on the group vector X[0..M) (spec: c's scaled spectrum)
void group_correlate(Ctx *c, G1Xyzz *X, size_t M, const Fr *spec, const GlvScalar *TG) {
  g_ntt(c->stream, X, M, M, TG, false);
  k_vo_pointwise<<<grid_for(M, 256, 4096), 256, 0, c->stream>>>(X, spec, M);
  TNS_LAUNCH_CHECK();
  g_ntt(c->stream, X, M, M, TG, true);
}
void fr_correlate(Ctx *c, Fr *X, size_t M, const Fr *spec, const Fr *TW) {
  fr_ntt(c->stream, X, M, M, TW, false);
  k_vo_fr_pointwise<<<grid_for(M, 256, 1u << 20), 256, 0, c->stream>>>(X, spec, M);
  TNS_LAUNCH_CHECK();
  fr_ntt(c->stream, X, M, M, TW, true);
}

// the Lagrange basis of n nodes whatever the context's commit basis says (nullptr: none to be had)
const LagrangeBasis *basis_or_null(Ctx *c, const Srs &srs, size_t n) {
  const bool saved = c->lagrange_commit;
  c->lagrange_commit = true;
  const LagrangeBasis *b = nullptr;
  try {
    b = lagrange_basis_dev(c, srs, n, 0, n);
  } catch (...) {
    c->lagrange_commit = saved;
    throw;
  }
  c->lagrange_commit = saved;
  return b;
}
const LagrangeBasis *basis_for(Ctx *c, const Srs &srs, size_t n) {
  const LagrangeBasis *b = basis_or_null(c, srs, n);
  if (!b)
    throw Error(TNS_ERR_INVALID_PARAMETERS,
                "the SRS provides no Lagrange basis of " + std::to_string(n) +
                    " nodes: attach tau (tns_srs_set_tau), or prepare or attach the basis "
                    "(tns_srs_prepare_lagrange_from_powers, tns_srs_lagrange_deserialize)");
  return b;
}

void check_vector(const Srs &srs, size_t n) {
  if (n == 0) throw Error(TNS_ERR_POLYNOMIAL, "empty evaluation vector");
  if (srs.first != 0 || srs.held < srs.n)
    throw Error(TNS_ERR_INVALID_PARAMETERS, "all-index openings need the whole SRS (this is a shard)");
  if (n > srs.n) throw Error(TNS_ERR_COMMITMENT, "Polynomial degree exceeds setup size");
}

}  // namespace

const OpenAllPlan *open_all_plan_dev(Ctx *c, const Srs &srs, size_t n) {
  auto it = srs.open_all.find(n);
  if (it != srs.open_all.end()) return it->second.get();
  const LagrangeBasis *basis = basis_for(c, srs, n);
  if (n > ((size_t)1 << 26)) throw Error(TNS_ERR_INVALID_PARAMETERS, "all-index openings of more than 2^26 entries");
  auto P = std::make_unique<OpenAllPlan>();
  P->n = n;
  P->M = next_pow2(2 * n - 1);
  if (n > 1) {  // (n == 1: the one proof is the identity)
    const size_t M = P->M;
    hipStream_t st = c->stream;
    const GlvScalar *TG = nullptr;
    const Fr *TW = transform_tables(c, ilog2_exact(M), &TG);
    const Fr *w = bary_weights_dev(c, n, 0, n);
    DevBuf fb, ifb, wb, xb, pre;
    Fr *fact = (Fr *)fb.ensure(sizeof(Fr) * n), *ifact = (Fr *)ifb.ensure(sizeof(Fr) * n);
    factorial_tables_dev(c, n, fact, ifact);
    Fr *spec = (Fr *)P->spec.ensure(sizeof(Fr) * M);
    const unsigned gM = grid_for(M, 256, 1u << 20), gn = grid_for(n, 256, 1u << 20);
    k_vo_kernel<<<gM, 256, 0, st>>>(fact, ifact, n, M, spec);
    TNS_LAUNCH_CHECK();
    fr_ntt(st, spec, M, M, TW, false);
    k_vo_scale<<<gM, 256, 0, st>>>(spec, M, inv(from_u64<FrCfg>((uint64_t)M)));
    TNS_LAUNCH_CHECK();
    // the scalars of f' that do not depend on the vector
    Fr *Wc = (Fr *)wb.ensure(sizeof(Fr) * M);
    k_vo_weighted<<<gM, 256, 0, st>>>(w, nullptr, n, M, Wc);
    TNS_LAUNCH_CHECK();
    fr_correlate(c, Wc, M, spec, TW);
    k_vo_plan_scalars<<<gn, 256, 0, st>>>(fact, Wc, n, (Fr *)P->iw.ensure(sizeof(Fr) * n),
                                          (Fr *)P->D.ensure(sizeof(Fr) * n));
    TNS_LAUNCH_CHECK();
    // A = Lambda * c
    G1Xyzz *X = (G1Xyzz *)xb.ensure(sizeof(G1Xyzz) * M);
    k_vo_points<<<gn, 256, 0, st>>>(basis->points.as<G1Affine>(), nullptr, n, X);
    k_vo_pad<<<grid_for(M - n, 256, 1u << 20), 256, 0, st>>>(X, n, M);
    TNS_LAUNCH_CHECK();
    group_correlate(c, X, M, spec, TG);
    xyzz_to_affine_batch_dev(c, X, n, (G1Affine *)P->A.ensure(sizeof(G1Affine) * n),
                             (Fq *)pre.ensure(sizeof(Fq) * n));
    TNS_HIP(hipStreamSynchronize(st));  // the scratch dies here
  }
  return (srs.open_all[n] = std::move(P)).get();
}

void vc_open_all_dev(Ctx *c, const Srs &srs, const Fr *vec, size_t n, G1Affine *proofs) {
  const OpenAllPlan *P = open_all_plan_dev(c, srs, n);
  hipStream_t st = c->stream;
  if (n == 1) {  // q_0 = 0
    TNS_HIP(hipMemsetAsync(proofs, 0, sizeof(G1Affine), st));
    TNS_HIP(hipStreamSynchronize(st));
    return;
  }
  const LagrangeBasis *basis = basis_for(c, srs, n);
  const size_t M = P->M;
  const GlvScalar *TG = nullptr;
  const Fr *TW = transform_tables(c, ilog2_exact(M), &TG);
  const Fr *w = bary_weights_dev(c, n, 0, n);
  const G1Affine *L = basis->points.as<G1Affine>();
  DevBuf ub, xb, pre;
  Fr *U = (Fr *)ub.ensure(sizeof(Fr) * M);
  G1Xyzz *X = (G1Xyzz *)xb.ensure(sizeof(G1Xyzz) * M);
  Fq *prefix = (Fq *)pre.ensure(sizeof(Fq) * n);
  const unsigned gS = grid_for(n, 256, 4096);  // scalar-multiplication kernels: whole waves of work
  k_vo_weighted<<<grid_for(M, 256, 1u << 20), 256, 0, st>>>(w, vec, n, M, U);
  TNS_LAUNCH_CHECK();
  fr_correlate(c, U, M, P->spec.as<Fr>(), TW);
  k_vo_points<<<gS, 256, 0, st>>>(L, vec, n, X);
  k_vo_pad<<<grid_for(M - n, 256, 1u << 20), 256, 0, st>>>(X, n, M);
  TNS_LAUNCH_CHECK();
  group_correlate(c, X, M, P->spec.as<Fr>(), TG);
  k_vo_combine<<<gS, 256, 0, st>>>(X, P->A.as<G1Affine>(), L, vec, U, P->iw.as<Fr>(), P->D.as<Fr>(), n);
  TNS_LAUNCH_CHECK();
  xyzz_to_affine_batch_dev(c, X, n, proofs, prefix);
  TNS_HIP(hipStreamSynchronize(st));  // the scratch dies here
}

// One per-index opening is an O(n) barycentric pass and an MSM of n points (0.8 ms at 2^12 entries,
// 3.7 ms at 2^20); the all-index pass is ~ M log2 M butterfly scalar multiplications, 2 log2 M
// dependent launches at the least (49 ms at 2^12, 0.95 s at 2^20): measured break-even at 62, 40,
// 110 and 257 indices for n = 2^12, 2^16, 2^18, 2^20, 8 log2 M = 104 .. 168 there.
bool vc_open_many_takes_all(size_t n, size_t k) { return k > 8 * (size_t)ilog2_exact(next_pow2(2 * n - 1)); }

}  // namespace tns

using namespace tns;

extern "C" {

// The batched forms of KZGVectorCommitment::open (src/commitments.rs:435-471).
int tns_srs_prepare_open_all(tns_ctx *ctx, tns_srs *srs, size_t n) {
  return guarded([&]() {
    if (!ctx || !srs) throw Error(TNS_ERR_INVALID_PARAMETERS, "null context or SRS");
    CtxScope g(&ctx->c);
    check_vector(srs->s, n);
    (void)open_all_plan_dev(&ctx->c, srs->s, n);
    return TNS_OK;
  });
}

int tns_vc_open_all_device(tns_ctx *ctx, tns_srs *srs, const uint64_t *d_vec, size_t n, uint64_t *d_proofs_affine_out) {
  return guarded([&]() {
    if (!ctx || !srs || !d_vec || !d_proofs_affine_out)
      throw Error(TNS_ERR_INVALID_PARAMETERS, "null context, SRS, vector or output");
    CtxScope g(&ctx->c);
    check_vector(srs->s, n);
    vc_open_all_dev(&ctx->c, srs->s, (const Fr *)d_vec, n, (G1Affine *)d_proofs_affine_out);
    return TNS_OK;
  });
}

int tns_vc_open_all(tns_ctx *ctx, tns_srs *srs, const uint64_t *vec, size_t n, uint64_t *proofs_affine_out) {
  return guarded([&]() {
    if (!ctx || !srs || !vec || !proofs_affine_out)
      throw Error(TNS_ERR_INVALID_PARAMETERS, "null context, SRS, vector or output");
    CtxScope g(&ctx->c);
    check_vector(srs->s, n);
    DevBuf d, o;
    Fr *dv = (Fr *)d.ensure(sizeof(Fr) * n);
    G1Affine *dp = (G1Affine *)o.ensure(sizeof(G1Affine) * n);
    TNS_HIP(hipMemcpyAsync(dv, vec, sizeof(Fr) * n, hipMemcpyHostToDevice, ctx->c.stream));
    vc_open_all_dev(&ctx->c, srs->s, dv, n, dp);
    TNS_HIP(hipMemcpy(proofs_affine_out, dp, sizeof(G1Affine) * n, hipMemcpyDeviceToHost));
    return TNS_OK;
  });
}

int tns_vc_open_many(tns_ctx *ctx, const tns_srs *srs, const uint64_t *vec, size_t n, const uint64_t *indices, size_t k,
                     uint64_t *values_out, uint64_t *proofs_proj_out) {
  return guarded([&]() {
    if (!ctx || !srs || !vec || (k && (!indices || !values_out || !proofs_proj_out)))
      throw Error(TNS_ERR_INVALID_PARAMETERS, "null context, SRS, vector, indices or output");
    CtxScope g(&ctx->c);
    Ctx *c = &ctx->c;
    check_vector(srs->s, n);
    for (size_t t = 0; t < k; t++)
      if (indices[t] >= n) throw Error(TNS_ERR_COMMITMENT, "Index out of bounds");
    if (k == 0) return TNS_OK;
    DevBuf d, cf, s, o;
    Fr *dv = (Fr *)d.ensure(sizeof(Fr) * n);
    TNS_HIP(hipMemcpyAsync(dv, vec, sizeof(Fr) * n, hipMemcpyHostToDevice, c->stream));
    std::vector<G1Affine> pis(k);
    if (vc_open_many_takes_all(n, k) && basis_or_null(c, srs->s, n)) {
      G1Affine *dp = (G1Affine *)o.ensure(sizeof(G1Affine) * n);
      vc_open_all_dev(c, srs->s, dv, n, dp);
      std::vector<G1Affine> all(n);
      TNS_HIP(hipMemcpy(all.data(), dp, sizeof(G1Affine) * n, hipMemcpyDeviceToHost));
      for (size_t t = 0; t < k; t++) pis[t] = all[indices[t]];
    } else {  // tns_vc_open per index, on the one uploaded copy (and one interpolation, without a basis)
      EvalPoly p;
      p.y = dv;
      p.N = p.cnt = n;
      p.coeffs = (Fr *)cf.ensure(sizeof(Fr) * n);
      p.basis = lagrange_basis_dev(c, srs->s, n, 0, n);
      for (size_t t = 0; t < k; t++) {
        Fr v;
        open_evals(c, srs->s, p, from_u64<FrCfg>(indices[t]), &v, &pis[t], s, comm_self());
      }
    }
    for (size_t t = 0; t < k; t++) {
      std::memcpy(values_out + 4 * t, vec + 4 * indices[t], sizeof(Fr));
      store_proj(pis[t], proofs_proj_out + 12 * t);
    }
    return TNS_OK;
  });
}

}  // extern "C"
