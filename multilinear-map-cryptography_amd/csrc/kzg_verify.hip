// kzg_verify.hip -- many KZG openings checked at once, soundly.
//
// KZGCommitment::verify (src/commitments.rs:201-228) is e(C - v G, G2) == e(pi, tau G2 - z G2), two
// pairings an opening.  Moving z pi to the left gives e(C - v G + z pi, G2) == e(pi, tau G2), whose
// G2 arguments no longer depend on the opening, so k of them add up under weights gamma_i:
//
//   L = sum gamma_i C_i - (sum gamma_i v_i) G + sum (gamma_i z_i) pi_i
//   R = sum gamma_i pi_i
//   accept  iff  e(L, G2) == e(R, tau G2)
//
// Valid openings always pass; if one is invalid the difference of the two sides is a non-zero linear
// form in the gamma_i, which vanishes for about 2^-128 of them -- PROVIDED the gamma_i are not known
// to whoever made the proofs (seed == NULL: 32 bytes from the OS).  gamma_i is the i-th 128-bit
// little-endian integer of ChaCha20Rng::from_seed(seed)'s word stream (block i / 4, words
// 4 (i % 4) .. + 3; 0 -> 1), tied to the absolute position i.
//
// On the device: the point validation, the challenges with the MSM scalars a_i = gamma_i and
// b_i = gamma_i z_i and the two scalar sums, and the MSMs (proofs, a), (proofs, b) on the two lanes
// and (commitments, a) when every opening has its own commitment.  On the host: (sum gamma) C for a
// shared commitment, (sum gamma v) G, and the two pairings.  A failed batch is bisected with the
// same gamma_i -- every step the same MSMs on a sub-range and a range reduction of the two sums --
// down to the lowest failing index: the MSM work of about two full checks, <= ceil(log2 k) + 1
// more pairing checks.
#include <sys/random.h>

#include "abi.hpp"

namespace tns {

namespace {

struct ChaChaKey {
  u32 k[8];
};

// the status word of the validation: the lowest refused index, all ones while none is
constexpr unsigned long long POINTS_OK = ~0ull;

__device__ __forceinline__ bool fq_below_modulus(const Fq &x) {  // x < p as integers
  bool lt = false;
#pragma unroll
  for (int i = 0; i < 8; i++) lt = x.v[i] < FqCfg::M[i] || (x.v[i] == FqCfg::M[i] && lt);
  return lt;
}

__device__ __forceinline__ Fq load_fq(const uint4 *p) {
  const uint4 lo = p[0], hi = p[1];
  Fq r;
  r.v[0] = lo.x, r.v[1] = lo.y, r.v[2] = lo.z, r.v[3] = lo.w;
  r.v[4] = hi.x, r.v[5] = hi.y, r.v[6] = hi.z, r.v[7] = hi.w;
  return r;
}

// Untrusted affine Montgomery limbs: both coordinates below p and the point on the curve (BN254 G1
// has cofactor 1: on the curve is in the group); the all-zero pair is the identity.  The lowest
// refused index wins *status.
__global__ void __launch_bounds__(256) k_verify_points(const G1Affine *__restrict__ pts, size_t n,
                                                       unsigned long long *status) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint4 *p = reinterpret_cast<const uint4 *>(pts + i);
  G1Affine P;
  P.x = load_fq(p);
  P.y = load_fq(p + 2);
  if (P.is_inf()) return;
  if (!fq_below_modulus(P.x) || !fq_below_modulus(P.y) || !g1_on_curve(P)) atomicMin(status, (unsigned long long)i);
}

__device__ __forceinline__ u32 rotl32_dev(u32 v, int c) { return (v << c) | (v >> (32 - c)); }

// gamma_i (canonical): words 4 (i % 4) .. + 3 of ChaCha20 block i / 4 (20 rounds, 64-bit counter,
// stream 0 -- transcript.cpp's chacha20_block_host), 0 replaced by 1
__device__ __forceinline__ Fr challenge_dev(const ChaChaKey &key, u64 i) {
  const u64 ctr = i >> 2;
  u32 s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
#pragma unroll
  for (int t = 0; t < 8; t++) s[4 + t] = key.k[t];
  s[12] = (u32)ctr;
  s[13] = (u32)(ctr >> 32);
  s[14] = s[15] = 0;
  u32 x[16];
#pragma unroll
  for (int t = 0; t < 16; t++) x[t] = s[t];
#define TNS_QR(a, b, c, d)                        \
  x[a] += x[b], x[d] = rotl32_dev(x[d] ^ x[a], 16); \
  x[c] += x[d], x[b] = rotl32_dev(x[b] ^ x[c], 12); \
  x[a] += x[b], x[d] = rotl32_dev(x[d] ^ x[a], 8);  \
  x[c] += x[d], x[b] = rotl32_dev(x[b] ^ x[c], 7)
  for (int r = 0; r < 10; r++) {
    TNS_QR(0, 4, 8, 12);
    TNS_QR(1, 5, 9, 13);
    TNS_QR(2, 6, 10, 14);
    TNS_QR(3, 7, 11, 15);
    TNS_QR(0, 5, 10, 15);
    TNS_QR(1, 6, 11, 12);
    TNS_QR(2, 7, 8, 13);
    TNS_QR(3, 4, 9, 14);
  }
#undef TNS_QR
  const int q = (int)(i & 3);
  Fr g = Fr::zero();
#pragma unroll
  for (int t = 0; t < 4; t++) {  // (selects, not an indexed read: x stays in registers)
    u32 w = x[t] + s[t];
    if (q == 1) w = x[4 + t] + s[4 + t];
    if (q == 2) w = x[8 + t] + s[8 + t];
    if (q == 3) w = x[12 + t] + s[12 + t];
    g.v[t] = w;
  }
  if (g.is_zero()) g.v[0] = 1;
  // The four high limbs are zeros the compiler can see, and the Montgomery product's asm blocks
  // (mont_mul.inc) must not be given such limbs beside non-zero ones: their carry word starts a
  // high column as the constant 0 too and is not early-clobber, so the compiler kept ONE register
  // for it and for these limbs -- a carry in the column then multiplied as a limb of gamma
  // (seen as sum gamma_i v_i off by ~2^64 for a few openings in a thousand).  Behind this barrier
  // every limb is a value of its own.
#pragma unroll
  for (int t = 0; t < 8; t++) asm volatile("" : "+v"(g.v[t]));
  return g;
}

// gamma i as integers: below 2^160 < r, so canonical as it stands (i < 2^32: a batch has < 2^31 openings)
__device__ __forceinline__ Fr challenge_times_index(const Fr &g, u32 i) {
  Fr r = Fr::zero();
  u64 carry = 0;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const u64 p = (u64)g.v[t] * i + carry;
    r.v[t] = (u32)p;
    carry = p >> 32;
  }
  r.v[4] = (u32)carry;
  return r;
}

__device__ __forceinline__ Fr fr_shfl_xor(const Fr &a, int o) {
  Fr r;
#pragma unroll
  for (int l = 0; l < 8; l++) r.v[l] = (u32)__shfl_xor((int)a.v[l], o);
  return r;
}

// (s0, s1) summed over the block into out[0], out[1]: a butterfly in each wave, then the four wave
// sums through LDS (blockDim.x == 256; every thread of the block calls it)
__device__ __forceinline__ void block_sum2(Fr s0, Fr s1, Fr *out) {
  __shared__ Fr wsum[2][4];
  for (int o = 32; o > 0; o >>= 1) {
    s0 = add(s0, fr_shfl_xor(s0, o));
    s1 = add(s1, fr_shfl_xor(s1, o));
  }
  const int w = (int)(threadIdx.x >> 6);
  if ((threadIdx.x & 63) == 0) {
    wsum[0][w] = s0;
    wsum[1][w] = s1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; i++) {
      s0 = add(s0, wsum[0][i]);
      s1 = add(s1, wsum[1][i]);
    }
    out[0] = s0;
    out[1] = s1;
  }
}

// One pass over the openings: a_i = gamma_i and b_i = gamma_i z_i as canonical scalars (what the
// bucket sort reads; z == nullptr: z_i = i) with their largest bit lengths in bits[0], bits[1]
// (zeroed by the caller), a_i in Montgomery form too when am is set (msm_dev's input), and this
// block's share of sum gamma_i and sum gamma_i v_i (canonical) in partials[2 b], [2 b + 1].
// A Montgomery product of the plain integer gamma with a Montgomery z or v is the canonical product.
__global__ void __launch_bounds__(256) k_verify_scalars(ChaChaKey key, const Fr *__restrict__ z,
                                                        const Fr *__restrict__ v, size_t k, Fr *__restrict__ a,
                                                        Fr *__restrict__ b, Fr *__restrict__ am,
                                                        Fr *__restrict__ partials, unsigned *bits) {
  Fr sg = Fr::zero(), sv = Fr::zero();
  unsigned ba = 0, bb = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < k; i += (size_t)gridDim.x * 256) {
    const Fr g = challenge_dev(key, (u64)i);
    const Fr gz = z ? mul(g, z[i]) : challenge_times_index(g, (u32)i);
    a[i] = g;
    b[i] = gz;
    if (am) am[i] = to_mont(g);
    sg = add(sg, g);
    sv = add(sv, mul(g, v[i]));
    ba = max(ba, fr_bit_length(g));
    bb = max(bb, fr_bit_length(gz));
  }
  block_atomic_max2(ba, bb, bits, bits + 1);
  block_sum2(sg, sv, partials + 2 * (size_t)blockIdx.x);
}

// the two sums over [lo, hi) again, from the stored a (the bisection: no gamma is regenerated)
__global__ void __launch_bounds__(256) k_verify_range_sums(const Fr *__restrict__ a, const Fr *__restrict__ v,
                                                           size_t lo, size_t hi, Fr *__restrict__ partials) {
  Fr sg = Fr::zero(), sv = Fr::zero();
  for (size_t i = lo + (size_t)blockIdx.x * 256 + threadIdx.x; i < hi; i += (size_t)gridDim.x * 256) {
    const Fr g = a[i];
    sg = add(sg, g);
    sv = add(sv, mul(g, v[i]));
  }
  block_sum2(sg, sv, partials + 2 * (size_t)blockIdx.x);
}

// the nb blocks' partials -> out[0], out[1] (one block)
__global__ void __launch_bounds__(256) k_verify_sums(const Fr *__restrict__ partials, unsigned nb,
                                                     Fr *__restrict__ out) {
  Fr sg = Fr::zero(), sv = Fr::zero();
  for (unsigned j = threadIdx.x; j < nb; j += 256) {
    sg = add(sg, partials[2 * (size_t)j]);
    sv = add(sv, partials[2 * (size_t)j + 1]);
  }
  block_sum2(sg, sv, out);
}

// a range of at most 64 openings takes the MSM's tiny path, which reads Montgomery scalars:
// m[t] = a_{lo+t}, m[64 + t] = b_{lo+t} in that form
__global__ void __launch_bounds__(64) k_verify_tiny_scalars(const Fr *__restrict__ a, const Fr *__restrict__ b,
                                                            size_t lo, int cnt, Fr *__restrict__ m) {
  const int t = (int)threadIdx.x;
  if (t >= cnt) return;
  m[t] = to_mont(a[lo + t]);
  m[64 + t] = to_mont(b[lo + t]);
}

constexpr unsigned SUM_BLOCKS = 1024;  // the scalar pass's grid bound = the partials' count

// the small device words of one call, in one allocation
struct VerifyWords {
  unsigned long long status;
  unsigned bits[2];
  Fr sums[2];
  Fr tiny[128];
};

bool fq_below_modulus_host(const Fq &x) { return !geq_raw<FqCfg>(x.v, FqCfg::M); }

struct Verifier {
  Ctx *c;
  const Vk &vk;
  const VerifyBatch &in;
  DevBuf ab, amb, pb, wb;
  Fr *a = nullptr, *b = nullptr, *am = nullptr, *partials = nullptr;
  VerifyWords *w = nullptr;

  Verifier(Ctx *ctx, const Vk &k, const VerifyBatch &batch) : c(ctx), vk(k), in(batch) {}

  void read_sums(Fr out[2]) {
    TNS_HIP(hipMemcpyAsync(out, w->sums, 2 * sizeof(Fr), hipMemcpyDeviceToHost, c->stream));
    TNS_HIP(hipStreamSynchronize(c->stream));
  }

  // the lowest malformed position, or POINTS_OK
  unsigned long long validate() {
    hipStream_t st = c->stream;
    const size_t k = in.k;
    TNS_HIP(hipMemsetAsync(&w->status, 0xff, sizeof(unsigned long long), st));
    const unsigned grid = (unsigned)((k + 255) / 256);
    {
      TNS_PROF(c, "verify_points", 64.0 * k);
      k_verify_points<<<grid, 256, 0, st>>>(in.proofs, k, &w->status);
      TNS_LAUNCH_CHECK();
    }
    if (in.commitments) {
      TNS_PROF(c, "verify_points", 64.0 * k);
      k_verify_points<<<grid, 256, 0, st>>>(in.commitments, k, &w->status);
      TNS_LAUNCH_CHECK();
    }
    unsigned long long s = POINTS_OK;
    TNS_HIP(hipMemcpyAsync(&s, &w->status, sizeof s, hipMemcpyDeviceToHost, st));
    TNS_HIP(hipStreamSynchronize(st));
    if (!in.commitments) {  // the one shared commitment stands at every position: the lowest is 0
      const G1Affine &C = in.shared;
      if (!fq_below_modulus_host(C.x) || !fq_below_modulus_host(C.y) || !g1_on_curve(C)) s = 0;
    }
    return s;
  }

  void scalars(const uint8_t seed[32]) {
    hipStream_t st = c->stream;
    const size_t k = in.k;
    ChaChaKey key;
    for (int i = 0; i < 8; i++)
      key.k[i] = (u32)seed[4 * i] | (u32)seed[4 * i + 1] << 8 | (u32)seed[4 * i + 2] << 16 | (u32)seed[4 * i + 3] << 24;
    a = (Fr *)ab.ensure(2 * sizeof(Fr) * k);
    b = a + k;
    if (in.commitments) am = (Fr *)amb.ensure(sizeof(Fr) * k);
    partials = (Fr *)pb.ensure(2 * sizeof(Fr) * SUM_BLOCKS);
    TNS_HIP(hipMemsetAsync(w->bits, 0, sizeof w->bits, st));
    const unsigned nb = grid_for(k, 256, SUM_BLOCKS);
    TNS_PROF(c, "verify_scalars", (32.0 + 64.0 + (am ? 32.0 : 0.0)) * k);
    k_verify_scalars<<<nb, 256, 0, st>>>(key, in.z, in.v, k, a, b, am, partials, w->bits);
    TNS_LAUNCH_CHECK();
    k_verify_sums<<<1, 256, 0, st>>>(partials, nb, w->sums);
    TNS_LAUNCH_CHECK();
  }

  // the weighted equation over the openings [lo, hi)
  bool check(size_t lo, size_t hi) {
    hipStream_t st = c->stream;
    const size_t cnt = hi - lo;
    if (lo != 0 || hi != in.k) {
      const unsigned nb = grid_for(cnt, 256, SUM_BLOCKS);
      TNS_PROF(c, "verify_scalars", 64.0 * cnt);
      k_verify_range_sums<<<nb, 256, 0, st>>>(a, in.v, lo, hi, partials);
      TNS_LAUNCH_CHECK();
      k_verify_sums<<<1, 256, 0, st>>>(partials, nb, w->sums);
      TNS_LAUNCH_CHECK();
    }
    Fr sums[2];  // sum gamma, sum gamma v (canonical)
    read_sums(sums);
    // the proofs' two MSMs side by side on the lanes; one-shot bases: no window table
    MsmArgs A{in.proofs + lo, a + lo, cnt, nullptr}, B{in.proofs + lo, b + lo, cnt, nullptr};
    if (cnt > 64) {
      A.src.canon_bits = &w->bits[0];  // (the whole batch's: an upper bound for a sub-range)
      B.src.canon_bits = &w->bits[1];
    } else {
      k_verify_tiny_scalars<<<1, 64, 0, st>>>(a, b, lo, (int)cnt, w->tiny);
      TNS_LAUNCH_CHECK();
      A.scalars = w->tiny;
      B.scalars = w->tiny + 64;
    }
    G1Xyzz pr[2];
    msm_pair_dev(c, A, B, pr);
    const G1Xyzz Cg = in.commitments ? msm_dev(c, in.commitments + lo, am + lo, cnt)
                                     : g1_mul_host(in.shared, to_mont(sums[0]));
    const G1Xyzz L = xyzz_add(xyzz_add(Cg, g1_mul_host(g1_neg(vk.g1), to_mont(sums[1]))), pr[1]);
    return pairing_eq(xyzz_to_affine(L), vk.g2, xyzz_to_affine(pr[0]), vk.g2_tau);
  }

  bool run(const uint8_t seed_in[32], bool locate, uint64_t *bad) {
    uint8_t seed[32];
    if (seed_in) {
      std::memcpy(seed, seed_in, 32);
    } else if (getrandom(seed, 32, 0) != 32) {
      throw Error(TNS_ERR_DEVICE, "no randomness from the OS for the verification challenges");
    }
    w = (VerifyWords *)wb.ensure(sizeof(VerifyWords));
    const unsigned long long s = validate();
    if (s != POINTS_OK) {  // a malformed point is a failed verification; no MSM has run
      *bad = (uint64_t)s;
      return false;
    }
    scalars(seed);
    if (check(0, in.k)) return true;
    *bad = 0;
    if (!locate) return false;
    // a failing range's left half fails, or else its right half does: the two halves' pairing
    // values multiply to the range's
    size_t lo = 0, hi = in.k;
    bool checked = true;  // [lo, hi) itself was seen to fail (not only inferred from its sibling)
    while (hi - lo > 1) {
      const size_t mid = lo + (hi - lo) / 2;
      checked = !check(lo, mid);
      if (checked) hi = mid;
      else lo = mid;
    }
    if (!checked && check(lo, hi))  // gamma_lo != 0: this last check is the opening's own equation
      throw Error(TNS_ERR_DEVICE, "batched verification: a failing range has no failing opening");
    *bad = (uint64_t)lo;
    return false;
  }
};

}  // namespace

bool kzg_verify_many_dev(Ctx *c, const Vk &vk, const VerifyBatch &in, const uint8_t seed[32], bool locate,
                         uint64_t *bad) {
  if (in.k == 0) return true;
  if (in.k >= ((size_t)1 << 31)) throw Error(TNS_ERR_COMMITMENT, "more than 2^31 openings in one batch");
  Verifier V(c, vk, in);
  try {
    return V.run(seed, locate, bad);
  } catch (...) {
    (void)hipStreamSynchronize(c->stream);  // nothing queued may outlive the buffers freed here
    throw;
  }
}

namespace {

// what the three entry points share: the outputs are written only once the check has run
int verify_entry(tns_ctx *ctx, const Vk &key, const VerifyBatch &in, const uint8_t seed[32], int *ok,
                 uint64_t *bad_index) {
  uint64_t bad = 0;
  const bool good = kzg_verify_many_dev(&ctx->c, key, in, seed, bad_index != nullptr, &bad);
  *ok = good ? 1 : 0;
  if (!good && bad_index) *bad_index = bad;
  return TNS_OK;
}

G1Affine load_affine(const uint64_t in[8]) {
  G1Affine a;
  std::memcpy(&a, in, sizeof a);
  return a;
}

// a projective commitment whose limbs are out of range becomes an affine point that is: the
// validation then refuses it like any other malformed point
G1Affine shared_from_proj(const uint64_t proj[12]) {
  G1Jac j;
  std::memcpy(&j, proj, sizeof j);
  if (!fq_below_modulus_host(j.x) || !fq_below_modulus_host(j.y) || !fq_below_modulus_host(j.z)) {
    G1Affine bad;
    bad.x = Fq::zero();
    bad.y = Fq::one();
    return bad;  // (0, 1) is not on y^2 = x^3 + 3
  }
  return proj_to_affine_host(proj);
}

}  // namespace

}  // namespace tns

using namespace tns;

extern "C" {

int tns_kzg_verify_many(tns_ctx *ctx, const tns_vk *vk, const uint64_t *commitments_affine, size_t n_commitments,
                        const uint64_t *points, const uint64_t *values, const uint64_t *proofs_affine, size_t k,
                        const uint8_t seed[32], int *ok, uint64_t *bad_index) {
  return guarded([&]() {
    if (!ctx || !vk || !ok || (k && (!commitments_affine || !points || !values || !proofs_affine)))
      throw Error(TNS_ERR_INVALID_PARAMETERS, "null context, verifier key, result or input array");
    if (k && n_commitments != 1 && n_commitments != k)
      throw Error(TNS_ERR_COMMITMENT, "Batch verify input lengths must match");
    CtxScope g(&ctx->c);
    const Vk key = vk_load(vk);
    VerifyBatch in;
    in.k = k;
    DevBuf pb, cb, sb;
    if (k) {
      hipStream_t st = ctx->c.stream;
      G1Affine *dp = (G1Affine *)pb.ensure(sizeof(G1Affine) * k);
      Fr *ds = (Fr *)sb.ensure(2 * sizeof(Fr) * k);
      TNS_HIP(hipMemcpyAsync(dp, proofs_affine, sizeof(G1Affine) * k, hipMemcpyHostToDevice, st));
      TNS_HIP(hipMemcpyAsync(ds, points, sizeof(Fr) * k, hipMemcpyHostToDevice, st));
      TNS_HIP(hipMemcpyAsync(ds + k, values, sizeof(Fr) * k, hipMemcpyHostToDevice, st));
      in.proofs = dp;
      in.z = ds;
      in.v = ds + k;
      if (n_commitments == 1) {
        in.shared = load_affine(commitments_affine);
      } else {
        G1Affine *dc = (G1Affine *)cb.ensure(sizeof(G1Affine) * k);
        TNS_HIP(hipMemcpyAsync(dc, commitments_affine, sizeof(G1Affine) * k, hipMemcpyHostToDevice, st));
        in.commitments = dc;
      }
    }
    return verify_entry(ctx, key, in, seed, ok, bad_index);
  });
}

int tns_vc_verify_all_device(tns_ctx *ctx, const tns_vk *vk, const uint64_t commitment_proj[12], const uint64_t *d_vec,
                             size_t n, const uint64_t *d_proofs_affine, const uint8_t seed[32], int *ok,
                             uint64_t *bad_index) {
  return guarded([&]() {
    if (!ctx || !vk || !ok || !commitment_proj || (n && (!d_vec || !d_proofs_affine)))
      throw Error(TNS_ERR_INVALID_PARAMETERS, "null context, verifier key, result, commitment, vector or proofs");
    CtxScope g(&ctx->c);
    const Vk key = vk_load(vk);
    VerifyBatch in;
    in.k = n;
    in.proofs = (const G1Affine *)d_proofs_affine;
    in.v = (const Fr *)d_vec;
    in.shared = shared_from_proj(commitment_proj);
    return verify_entry(ctx, key, in, seed, ok, bad_index);
  });
}

int tns_vc_verify_all(tns_ctx *ctx, const tns_vk *vk, const uint64_t commitment_proj[12], const uint64_t *vec, size_t n,
                      const uint64_t *proofs_affine, const uint8_t seed[32], int *ok, uint64_t *bad_index) {
  return guarded([&]() {
    if (!ctx || !vk || !ok || !commitment_proj || (n && (!vec || !proofs_affine)))
      throw Error(TNS_ERR_INVALID_PARAMETERS, "null context, verifier key, result, commitment, vector or proofs");
    CtxScope g(&ctx->c);
    const Vk key = vk_load(vk);
    VerifyBatch in;
    in.k = n;
    DevBuf pb, vb;
    if (n) {
      G1Affine *dp = (G1Affine *)pb.ensure(sizeof(G1Affine) * n);
      Fr *dv = (Fr *)vb.ensure(sizeof(Fr) * n);
      TNS_HIP(hipMemcpyAsync(dp, proofs_affine, sizeof(G1Affine) * n, hipMemcpyHostToDevice, ctx->c.stream));
      TNS_HIP(hipMemcpyAsync(dv, vec, sizeof(Fr) * n, hipMemcpyHostToDevice, ctx->c.stream));
      in.proofs = dp;
      in.v = dv;
    }
    in.shared = shared_from_proj(commitment_proj);
    return verify_entry(ctx, key, in, seed, ok, bad_index);
  });
}

}  // extern "C"
