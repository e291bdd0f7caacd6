// fieldprobe.hip -- the device field and point primitives of csrc/ behind thin kernels, for
// tests/test_gpu_field_primitives.py.  One thread a case: load the operands, call ONE primitive
// (or one usage pattern of it), store the result.  No arithmetic lives here: every function under
// test is the one the library compiles (bn254.hpp with mont_mul.inc and field_asm.inc, or
// field_bi.inc under -DTNS_FIELD_BI; group_ntt.hpp; fq_sqrt.hpp).  Built stand-alone as
// libtns_fieldprobe.so / libtns_fieldprobe_bi.so (Makefile); does not link libtns.so.
//
// A field element is 8 u32 words, a G1Xyzz 32, a G1Affine 16.  fieldprobe_run(op, field, ...)
// takes n cases of in_words(op, iters) words each and returns n * out_words(op, iters) words; the
// op numbers are mirrored in the Python test.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bn254.hpp"
#include "fq_sqrt.hpp"
#include "group_ntt.hpp"

using namespace tns;

namespace {

enum Op : int {
  // canonical field functions
  F_MUL = 0, F_SQR, F_ADD, F_SUB, F_NEG, F_REDUCE_ONCE, F_TO_MONT, F_FROM_MONT, F_INV, F_INV_WINDOW, F_INV_BINARY,
  // lazy-domain field functions
  F_MUL_LAZY, F_SQR_LAZY, F_MUL2_LAZY, F_ADD2, F_SUB2, F_CMINUS_2M, F_CMINUS_M, F_REDUCE_2M, F_CANON2,
  F_ZERO_LAZY, F_SQRT,  // Fq only
  // usage patterns: `iters` loop-carried steps, every iterate stored
  P_MUL_AB, P_MUL_BA, P_SQR, P_MUL_LAZY_AB, P_MUL_LAZY_BA, P_SQR_LAZY, P_ADD2_SELF, P_SUB_BA, P_CHAIN_GLOBAL,
  P_FINISH2, P_ALIAS,
  // G1 (Fq only)
  G_MADD_LAZY, G_ADD_LAZY, G_DBL_LAZY, G_CANON, G_MUL_CANON, G_ADD, G_MADD, G_DBL, G_MDBL, G_MADD_CHAIN,
  OP_COUNT
};

constexpr int W = 8, WX = 32, WA = 16;
constexpr int ALIAS_OUT = 7;

constexpr int in_words(int op, int it) {
  switch (op) {
    case F_MUL: case F_ADD: case F_SUB: case F_MUL_LAZY: case F_ADD2: case F_SUB2: return 2 * W;
    case F_MUL2_LAZY: return 4 * W;
    case P_MUL_AB: case P_MUL_BA: case P_MUL_LAZY_AB: case P_MUL_LAZY_BA: case P_SUB_BA: case P_ALIAS: return 2 * W;
    case P_CHAIN_GLOBAL: return (1 + it) * W;
    case P_FINISH2: return (1 + 2 * it) * W;
    case G_MADD_LAZY: case G_MADD: return WX + WA;
    case G_ADD_LAZY: case G_ADD: return 2 * WX;
    case G_DBL_LAZY: case G_CANON: case G_DBL: return WX;
    case G_MUL_CANON: return WX + W;
    case G_MDBL: return WA;
    case G_MADD_CHAIN: return WX + it * WA;
    default: return W;
  }
}
constexpr int out_words(int op, int it) {
  switch (op) {
    case P_MUL_AB: case P_MUL_BA: case P_SQR: case P_MUL_LAZY_AB: case P_MUL_LAZY_BA: case P_SQR_LAZY:
    case P_ADD2_SELF: case P_SUB_BA: case P_CHAIN_GLOBAL: return it * W;
    case P_FINISH2: return 2 * it * W;
    case P_ALIAS: return ALIAS_OUT * W;
    case G_MADD_CHAIN: return it * WX;
    default: return op >= G_MADD_LAZY ? WX : W;
  }
}

template <class C>
__device__ __forceinline__ Fp<C> ld(const uint32_t *p) {
  Fp<C> a;
#pragma unroll
  for (int i = 0; i < 8; i++) a.v[i] = p[i];
  return a;
}
template <class C>
__device__ __forceinline__ void st(uint32_t *p, const Fp<C> &a) {
#pragma unroll
  for (int i = 0; i < 8; i++) p[i] = a.v[i];
}
__device__ __forceinline__ G1Xyzz ldx(const uint32_t *p) {
  G1Xyzz r;
  r.x = ld<FqCfg>(p), r.y = ld<FqCfg>(p + 8), r.zz = ld<FqCfg>(p + 16), r.zzz = ld<FqCfg>(p + 24);
  return r;
}
__device__ __forceinline__ G1Affine lda(const uint32_t *p) {
  G1Affine r;
  r.x = ld<FqCfg>(p), r.y = ld<FqCfg>(p + 8);
  return r;
}
__device__ __forceinline__ void stx(uint32_t *p, const G1Xyzz &r) {
  st(p, r.x), st(p + 8, r.y), st(p + 16, r.zz), st(p + 24, r.zzz);
}

template <class C, int OP>
__global__ void __launch_bounds__(64) k_field(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t n,
                                              int iters) {
  typedef Fp<C> F;
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t *x = in + i * (size_t)in_words(OP, iters);
  uint32_t *y = out + i * (size_t)out_words(OP, iters);
  if constexpr (OP == F_MUL) st(y, mul(ld<C>(x), ld<C>(x + 8)));
  if constexpr (OP == F_SQR) st(y, sqr(ld<C>(x)));
  if constexpr (OP == F_ADD) st(y, add(ld<C>(x), ld<C>(x + 8)));
  if constexpr (OP == F_SUB) st(y, sub(ld<C>(x), ld<C>(x + 8)));
  if constexpr (OP == F_NEG) st(y, neg(ld<C>(x)));
  if constexpr (OP == F_REDUCE_ONCE) {
    F a = ld<C>(x);
    reduce_once(a);
    st(y, a);
  }
  if constexpr (OP == F_TO_MONT) st(y, to_mont(ld<C>(x)));
  if constexpr (OP == F_FROM_MONT) st(y, from_mont(ld<C>(x)));
  if constexpr (OP == F_INV) st(y, inv(ld<C>(x)));
  if constexpr (OP == F_INV_WINDOW) st(y, inv_window_dev(ld<C>(x)));
  if constexpr (OP == F_INV_BINARY) st(y, inv_binary_dev(ld<C>(x)));
  if constexpr (OP == F_MUL_LAZY) st(y, mul_lazy_dev(ld<C>(x), ld<C>(x + 8)));
  if constexpr (OP == F_SQR_LAZY) st(y, sqr_lazy_dev(ld<C>(x)));
  if constexpr (OP == F_MUL2_LAZY) st(y, mul2_lazy_dev(ld<C>(x), ld<C>(x + 8), ld<C>(x + 16), ld<C>(x + 24)));
  if constexpr (OP == F_ADD2) st(y, add2_dev(ld<C>(x), ld<C>(x + 8)));
  if constexpr (OP == F_SUB2) st(y, sub2_dev(ld<C>(x), ld<C>(x + 8)));
  if constexpr (OP == F_CMINUS_2M) st(y, const_minus_dev<C, true>(ld<C>(x)));
  if constexpr (OP == F_CMINUS_M) st(y, const_minus_dev<C, false>(ld<C>(x)));
  if constexpr (OP == F_REDUCE_2M) {
    F a = ld<C>(x);
    reduce_once_2m_dev(a);
    st(y, a);
  }
  if constexpr (OP == F_CANON2) {  // sumcheck.hip sc_canon: [0, 2M] -> [0, M)
    F a = ld<C>(x);
    reduce_once(a);
    reduce_once(a);
    st(y, a);
  }
  if constexpr (OP == P_MUL_AB || OP == P_MUL_BA || OP == P_MUL_LAZY_AB || OP == P_MUL_LAZY_BA || OP == P_SUB_BA) {
    F a = ld<C>(x);
    const F b = ld<C>(x + 8);
#pragma unroll 1
    for (int j = 0; j < iters; j++) {
      if constexpr (OP == P_MUL_AB) a = mul(a, b);
      if constexpr (OP == P_MUL_BA) a = mul(b, a);
      if constexpr (OP == P_MUL_LAZY_AB) a = mul_lazy_dev(a, b);
      if constexpr (OP == P_MUL_LAZY_BA) a = mul_lazy_dev(b, a);
      if constexpr (OP == P_SUB_BA) a = sub(b, a);
      st(y + 8 * j, a);
    }
  }
  if constexpr (OP == P_SQR || OP == P_SQR_LAZY || OP == P_ADD2_SELF) {
    F a = ld<C>(x);
#pragma unroll 1
    for (int j = 0; j < iters; j++) {
      if constexpr (OP == P_SQR) a = sqr(a);
      if constexpr (OP == P_SQR_LAZY) a = sqr_lazy_dev(a);
      if constexpr (OP == P_ADD2_SELF) a = add2_dev(a, a);
      st(y + 8 * j, a);
    }
  }
  if constexpr (OP == P_CHAIN_GLOBAL) {  // iv = mul(iv, d[j]), d[j] from memory, iv to memory
    F iv = ld<C>(x);
#pragma unroll 1
    for (int j = 0; j < iters; j++) {
      iv = mul(iv, ld<C>(x + 8 * (1 + j)));
      st(y + 8 * j, iv);
    }
  }
  if constexpr (OP == P_FINISH2) {  // lagrange.hip's node-finish shape: two products share iv
    F iv = ld<C>(x);
#pragma unroll 1
    for (int j = 0; j < iters; j++) {
      const F inv_j = mul(iv, ld<C>(x + 8 * (1 + 2 * j)));
      iv = mul(iv, ld<C>(x + 8 * (2 + 2 * j)));
      st(y + 16 * j, inv_j);
      st(y + 16 * j + 8, iv);
    }
  }
  if constexpr (OP == P_ALIAS) {
    const F a = ld<C>(x), b = ld<C>(x + 8);
    st(y, mul(a, a));
    st(y + 8, mul_lazy_dev(a, a));
    st(y + 16, mul2_lazy_dev(a, a, a, a));
    st(y + 24, mul2_lazy_dev(a, b, b, a));
    st(y + 32, add(a, a));
    st(y + 40, sub(a, a));
    st(y + 48, sub2_dev(a, a));
  }
}

template <int OP>
__global__ void __launch_bounds__(64) k_fq(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t n,
                                           int iters) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint32_t *x = in + i * (size_t)in_words(OP, iters);
  uint32_t *y = out + i * (size_t)out_words(OP, iters);
  if constexpr (OP == F_ZERO_LAZY) {
    Fq r = Fq::zero();
    r.v[0] = fq_zero_lazy(ld<FqCfg>(x)) ? 1u : 0u;
    st(y, r);
  }
  if constexpr (OP == F_SQRT) st(y, fq_sqrt_candidate_dev(ld<FqCfg>(x)));
  if constexpr (OP == G_MADD_LAZY) stx(y, xyzz_madd_lazy(ldx(x), lda(x + WX)));
  if constexpr (OP == G_ADD_LAZY) stx(y, xyzz_add_lazy(ldx(x), ldx(x + WX)));
  if constexpr (OP == G_DBL_LAZY) stx(y, xyzz_dbl_lazy(ldx(x)));
  if constexpr (OP == G_CANON) stx(y, xyzz_canon(ldx(x)));
  if constexpr (OP == G_MUL_CANON) stx(y, xyzz_mul_canon(ldx(x), ld<FrCfg>(x + WX)));
  if constexpr (OP == G_ADD) stx(y, xyzz_add(ldx(x), ldx(x + WX)));
  if constexpr (OP == G_MADD) stx(y, xyzz_madd(ldx(x), lda(x + WX)));
  if constexpr (OP == G_DBL) stx(y, xyzz_dbl(ldx(x)));
  if constexpr (OP == G_MDBL) stx(y, xyzz_mdbl(lda(x)));
  if constexpr (OP == G_MADD_CHAIN) {
    G1Xyzz acc = ldx(x);
#pragma unroll 1
    for (int j = 0; j < iters; j++) {
      acc = xyzz_madd_lazy(acc, lda(x + WX + WA * j));
      stx(y + WX * j, acc);
    }
  }
}

typedef void (*Kernel)(const uint32_t *, uint32_t *, size_t, int);

template <int OP>
Kernel pick(int field) {
  if constexpr (OP == F_ZERO_LAZY || OP == F_SQRT || OP >= G_MADD_LAZY)
    return field == 1 ? k_fq<OP> : nullptr;
  else
    return field == 0 ? k_field<FrCfg, OP> : field == 1 ? k_field<FqCfg, OP> : nullptr;
}

template <int OP = 0>
Kernel kernel_of(int op, int field) {
  if constexpr (OP < OP_COUNT) {
    return op == OP ? pick<OP>(field) : kernel_of<OP + 1>(op, field);
  } else {
    return nullptr;
  }
}

}  // namespace

extern "C" {

int fieldprobe_op_count() { return OP_COUNT; }

// words a case of `op` reads and writes (0 for an unknown op)
int fieldprobe_in_words(int op, int iters) { return op >= 0 && op < OP_COUNT ? in_words(op, iters) : 0; }
int fieldprobe_out_words(int op, int iters) { return op >= 0 && op < OP_COUNT ? out_words(op, iters) : 0; }

// Run n cases of `op` over `field` (0 = Fr, 1 = Fq).  Returns the HIP status (0 = success), -1 for
// an unknown op / field or buffer sizes that do not match the op's shape, and -2 for an
// inv_binary_dev operand outside [0, M) (its Euclid loop does not terminate there).
int fieldprobe_run(int op, int field, const uint32_t *in, uint64_t in_total, uint32_t *out, uint64_t out_total,
                   uint64_t n, int iters) {
  if (op < 0 || op >= OP_COUNT || iters < 0 || iters > 64 || n == 0 || n > (1u << 22)) return -1;
  const Kernel k = kernel_of(op, field);
  if (!k) return -1;
  if (in_total != n * (uint64_t)in_words(op, iters) || out_total != n * (uint64_t)out_words(op, iters)) return -1;
  if (op == F_INV_BINARY) {
    const uint32_t *M = field == 0 ? FrCfg::M : FqCfg::M;
    for (uint64_t c = 0; c < n; c++) {
      bool lt = false;
      for (int i = 0; i < 8; i++) lt = in[8 * c + i] < M[i] || (in[8 * c + i] == M[i] && lt);
      if (!lt) return -2;
    }
  }
  uint32_t *din = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc(&din, in_total * 4);
  if (e == hipSuccess) e = hipMalloc(&dout, out_total * 4);
  if (e == hipSuccess) e = hipMemcpy(din, in, in_total * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0xA5, out_total * 4);
  if (e == hipSuccess) {
    k<<<dim3((unsigned)((n + 63) / 64)), dim3(64)>>>(din, dout, (size_t)n, iters);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, out_total * 4, hipMemcpyDeviceToHost);
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return (int)e;
}

}  // extern "C"
