// fq_sqrt.hpp -- the Fq square root candidate of the SRS decoder (srs_io.hip), in a header so that
// the device tests (tests/device/fieldprobe.hip) call the function the library compiles.
#pragma once
#include "bn254.hpp"
#include "sqrt_chain.inc"

namespace tns {

// a^((p+1)/4), the square root of a square (p = 3 mod 4), along the fixed sliding-window chain of
// sqrt_chain.inc: 251 squarings + 58 products a point, table {a, a^3, a^5, a^7} included, against
// the 256 squarings + 109 products of pow_limbs over the same exponent.  Lazy [0, 2M) domain with
// the dedicated lazy square until the one conditional subtraction at the end (as inv_window_dev),
// so the result is the canonical representative: bit-equal to the host's pow_limbs.  The chain is
// read from constant memory with a uniform index: uniform control flow.
__device__ __forceinline__ Fq fq_sqrt_candidate_dev(const Fq &a) {
  const Fq a2 = sqr_lazy_dev(a);
  const Fq t1 = a, t3 = mul_lazy_dev(a, a2), t5 = mul_lazy_dev(t3, a2), t7 = mul_lazy_dev(t5, a2);
  auto entry = [&](unsigned idx) -> const Fq & { return idx == 0 ? t1 : idx == 1 ? t3 : idx == 2 ? t5 : t7; };
  Fq acc = entry(kSqrtChainFq[0] & 3);
  for (int k = 1; k < (int)sizeof(kSqrtChainFq); k++) {
    const unsigned st = kSqrtChainFq[k];
    for (unsigned q = 0; q < (st >> 2); q++) acc = sqr_lazy_dev(acc);
    acc = mul_lazy_dev(acc, entry(st & 3));
  }
  for (int q = 0; q < kSqrtTailFq; q++) acc = sqr_lazy_dev(acc);
  reduce_once(acc);
  return acc;
}

}  // namespace tns
