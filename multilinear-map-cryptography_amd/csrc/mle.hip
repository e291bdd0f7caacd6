// mle.hip -- multilinear-extension fold and evaluate.
//
// Reference semantics: MultilinearExtension::evaluate / partial_evaluate
// (src/polynomials.rs:85-161) with variable j <-> index bit j (LSB first).  An MLE is kept as a
// table and one variable is bound per fold:  T'[s] = T[2s] + r (T[2s+1] - T[2s]).  The sum-check
// engine (sumcheck.hip) and the zero-closure fold chains (zero_folds.hip) fuse this fold into
// their own kernels.
#include <hip/hip_runtime.h>

#include "ctx.hpp"
#include "host.hpp"

namespace tns {

__global__ void __launch_bounds__(256) k_mle_fold(const Fr *__restrict__ in, Fr *__restrict__ out,
                                                  size_t half, Fr r) {
  for (size_t s = blockIdx.x * (size_t)blockDim.x + threadIdx.x; s < half;
       s += (size_t)gridDim.x * blockDim.x) {
    Fr a = in[2 * s], b = in[2 * s + 1];
    out[s] = add(a, mul(r, sub(b, a)));
  }
}

void mle_fold_dev(Ctx *c, const Fr *in, Fr *out, size_t half, const Fr &r) {
  k_mle_fold<<<grid_for(half, 256), 256, 0, c->stream>>>(in, out, half, r);
  TNS_LAUNCH_CHECK();
}

// Evaluate by nv successive folds (ping-pong in scratch).  point_host: nv Fr.
Fr mle_evaluate_dev(Ctx *c, const Fr *evals, unsigned nv, const Fr *point_host) {
  if (nv == 0) {
    Fr r;
    TNS_HIP(hipMemcpyAsync(&r, evals, sizeof(Fr), hipMemcpyDeviceToHost, c->stream));
    TNS_HIP(hipStreamSynchronize(c->stream));
    return r;
  }
  size_t n = (size_t)1 << nv;
  Fr *a = (Fr *)c->scratch.mle_ping().ensure(sizeof(Fr) * (n / 2));
  Fr *b = (Fr *)c->scratch.mle_pong().ensure(sizeof(Fr) * (n / 4 > 0 ? n / 4 : 1));
  const Fr *src = evals;
  Fr *dst = a;
  for (unsigned j = 0; j < nv; j++) {
    size_t half = n >> (j + 1);
    mle_fold_dev(c, src, dst, half, point_host[j]);
    src = dst;
    dst = (dst == a) ? b : a;
  }
  Fr r;
  TNS_HIP(hipMemcpyAsync(&r, src, sizeof(Fr), hipMemcpyDeviceToHost, c->stream));
  TNS_HIP(hipStreamSynchronize(c->stream));
  return r;
}

}  // namespace tns
