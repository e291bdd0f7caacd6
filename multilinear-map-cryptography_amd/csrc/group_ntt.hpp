// group_ntt.hpp -- the radix-2 transform over G1 that tfree.hip defines and vc_open.hip shares: the
// GLV-split twiddles, the transform's entry points beside its scalar twin, the occupancy bounds of
// the kernels that multiply points by scalars, and the point arithmetic those kernels share.
#pragma once
#include "bn254.hpp"
#include "hip_util.hpp"

namespace tns {

struct Ctx;

// X holds N / M transforms of size M, each in place: forward DIF (natural in, bit-reversed out) or
// inverse DIT (bit-reversed in, natural out, unscaled), a butterfly's twiddle multiplication split
// by the GLV endomorphism.  TG = glv_twiddles of the ntt_twiddles table TW[0..M) (downloaded,
// split on host threads, uploaded: synchronises); fr_ntt is the same radix-2 transform on scalars,
// so spectra of both line up index by index.
struct GlvScalar {
  uint32_t k1[4], k2[4];  // magnitudes
  uint32_t neg;           // bit 0: k1 < 0, bit 1: k2 < 0
};
void glv_twiddles(Ctx *c, const Fr *TW, size_t N, DevBuf &out);
void g_ntt(hipStream_t st, G1Xyzz *X, size_t N, size_t M, const GlvScalar *TG, bool inverse);
void fr_ntt(hipStream_t st, Fr *X, size_t N, size_t M, const Fr *TW, bool inverse);
// the kernels that multiply points by scalars: 3 waves per SIMD (168 VGPRs; the default bound let
// the compiler take 258 registers, one wave per SIMD)
#define TF_WAVES 3
// the group NTT's butterflies (GLV joint multiplication: P, phi(P), their sum and the accumulator)
#ifndef TF_NTT_WAVES
#define TF_NTT_WAVES 2
#endif

__device__ __forceinline__ G1Xyzz xyzz_negate(const G1Xyzz &p) {
  G1Xyzz r = p;
  r.y = neg(p.y);
  return r;
}

// dbl-2008-s-1 in the lazy domain (coordinates in [0, 2M), as xyzz_add_lazy): no final
// subtractions in the products, Y3 as one reduction of M (S - X3) + Y (2M - W)
__device__ __forceinline__ G1Xyzz xyzz_dbl_lazy(const G1Xyzz &p) {
  if (fq_zero_lazy(p.zz) || fq_zero_lazy(p.y)) return G1Xyzz::inf();
  const Fq U = add2_dev(p.y, p.y);
  const Fq V = sqr_lazy_dev(U);
  const Fq W = mul_lazy_dev(U, V);
  const Fq S = mul_lazy_dev(p.x, V);
  const Fq X2 = sqr_lazy_dev(p.x);
  const Fq M = add2_dev(add2_dev(X2, X2), X2);
  G1Xyzz r;
  r.x = sub2_dev(sqr_lazy_dev(M), add2_dev(S, S));
  r.y = mul2_lazy_dev(M, sub2_dev(S, r.x), p.y, const_minus_dev<FqCfg, true>(W));
  r.zz = mul_lazy_dev(V, p.zz);
  r.zzz = mul_lazy_dev(W, p.zzz);
  return r;
}

// k P for a canonical scalar k (the plain integer, not its Montgomery form, below r) and P with
// coordinates in [0, 2M); the result is canonical.  Left to right from k's top bit.  Where the lanes of a wave share
// k (the group NTT maps equal twiddles to one wave), the branches are uniform.
static __device__ G1Xyzz xyzz_mul_canon(const G1Xyzz &P, const Fr &k) {
  G1Xyzz acc = G1Xyzz::inf();
  bool started = false;
#pragma unroll 1
  for (int l = 7; l >= 0; l--) {
    uint32_t w = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) w = q == l ? k.v[q] : w;  // (a dynamic index would use scratch)
    if (!started && w == 0) continue;
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      if (started) acc = xyzz_dbl_lazy(acc);
      if ((w >> b) & 1u) {
        acc = started ? xyzz_add_lazy(acc, P) : P;
        started = true;
      }
    }
  }
  return xyzz_canon(acc);
}

}  // namespace tns
