// sc_poly.hpp -- what the generic sum-check's round kernels share (sumcheck.hip: one instance;
// sumcheck_batch.hip: a batch of instances): the nested form of a composition and its evaluation
// at one point, the lazy-domain arithmetic the rounds run in, the wave / block reductions, and
// the dispatch of a launch on the table count.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "sumcheck.hpp"

namespace tns {

// f(std::integral_constant<int, K>()) for k = K in 1..4 tables (any other k: 4), so that a launch
// names its kernel's table count at compile time: k_x<decltype(K)::value><<<...>>>(...)
template <class F>
static void sc_for_tables(int k, F &&f) {
  switch (k) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    default: f(std::integral_constant<int, 4>()); break;
  }
}

// ---------------------------------------------------------------- generic compositions
// A degree <= 3 composition sum_t c_t prod_{j in t} T_j over K <= 4 tables is rewritten on the
// host (sc_poly) in nested form
//     f = c + sum_i T_i (c_i + sum_{j >= i} T_j (c_ij + sum_{l >= j} c_ijl T_l))
// with the tables renumbered for the fewest products per point: the Twist-shaped
// A V - O O V + 2 O becomes V (A - O O) + 2 O, 2 products instead of 3.  The round kernel unrolls
// i, j, l at compile time (table values stay in registers, no run-time selects) and branches only
// on the uniform coefficient kinds; a coefficient multiplies only when it is not 1, -1 or 2.
constexpr int SC_SLOTS = 35;  // 1 constant + 4 linear + 10 quadratic + 20 cubic monomials
enum : int32_t { CK_ZERO = 0, CK_ONE = 1, CK_MONE = 2, CK_TWO = 3, CK_ANY = 4 };
// (the flags are 32-bit words: the kernel reads them with scalar loads.  As bytes they were
// global_load_ubyte -- gfx950 has no sub-dword scalar load -- each followed by a vmcnt(0) wait
// that also waited out the wave's table loads and fold stores: ~20 memory round trips per point)
struct ScPoly {
  Fr coef[SC_SLOTS];
  int32_t kind[SC_SLOTS];
  int32_t has_i[MAX_SC_TABLES];                  // some monomial starts with table i
  int32_t i_lin[MAX_SC_TABLES];                  // ... and i's inner part is more than c_i
  int32_t has_ij[MAX_SC_TABLES][MAX_SC_TABLES];  // some monomial starts with (i, j)
  int32_t ij_lin[MAX_SC_TABLES][MAX_SC_TABLES];  // ... and (i, j)'s inner part is more than c_ij
  int32_t ij_sq[MAX_SC_TABLES][MAX_SC_TABLES];   // ... and that inner part is c_ijj T_j alone: a square
};
__host__ __device__ constexpr int sc_slot1(int i) { return 1 + i; }
__host__ __device__ constexpr int sc_slot2(int i, int j) { return 5 + 4 * i - i * (i - 1) / 2 + (j - i); }
__host__ __device__ constexpr int sc_slot3(int i, int j, int l) {
  int s = 15;
  for (int a = 0; a < 4; a++)
    for (int b = a; b < 4; b++)
      for (int c = b; c < 4; c++) {
        if (a == i && b == j && c == l) return s;
        s++;
      }
  return -1;
}

// The nested form of a composition for one table order perm (perm[m] = the caller's table that
// kernel table m reads); returns its products per evaluation point.
static int sc_poly_for(const SumcheckTerm *terms, int n_terms, int k, const int *perm, ScPoly *out) {
  int inv[MAX_SC_TABLES] = {0, 0, 0, 0};
  for (int m = 0; m < k; m++) inv[perm[m]] = m;
  Fr acc[SC_SLOTS];
  bool used[SC_SLOTS] = {};
  for (int t = 0; t < SC_SLOTS; t++) acc[t] = Fr::zero();
  for (int t = 0; t < n_terms; t++) {
    int ix[3], d = 0;
    for (int j = 0; j < 3; j++)
      if (terms[t].tab[j] >= 0) ix[d++] = inv[terms[t].tab[j]];
    std::sort(ix, ix + d);
    const int slot = d == 0 ? 0 : d == 1 ? sc_slot1(ix[0]) : d == 2 ? sc_slot2(ix[0], ix[1]) : sc_slot3(ix[0], ix[1], ix[2]);
    acc[slot] = add(acc[slot], terms[t].coeff);
    used[slot] = true;
  }
  ScPoly q{};
  const Fr one = Fr::one(), two = add(one, one), mone = neg(one);
  int muls = 0;
  for (int t = 0; t < SC_SLOTS; t++) {
    q.coef[t] = acc[t];
    q.kind[t] = !used[t] || acc[t] == Fr::zero() ? CK_ZERO
                : acc[t] == one                 ? CK_ONE
                : acc[t] == mone                ? CK_MONE
                : acc[t] == two                 ? CK_TWO
                                                : CK_ANY;
  }
  for (int i = 0; i < k; i++) {
    for (int j = i; j < k; j++) {
      bool lin = false;
      for (int l = j; l < k; l++)
        if (q.kind[sc_slot3(i, j, l)]) {
          lin = true;
          muls += q.kind[sc_slot3(i, j, l)] == CK_ANY;
        }
      q.ij_lin[i][j] = lin;
      q.has_ij[i][j] = lin || q.kind[sc_slot2(i, j)];
      bool only_jj = lin && !q.kind[sc_slot2(i, j)];
      for (int l = j + 1; l < k; l++) only_jj = only_jj && !q.kind[sc_slot3(i, j, l)];
      q.ij_sq[i][j] = only_jj;  // T_j (c_ijj T_j) = c_ijj T_j^2
      if (lin) muls += 1;  // T_j * (c_ij + ...)
      else if (q.kind[sc_slot2(i, j)] == CK_ANY) muls += 1;
      q.i_lin[i] |= q.has_ij[i][j];
    }
    q.has_i[i] = q.i_lin[i] || q.kind[sc_slot1(i)];
    if (q.i_lin[i]) muls += 1;  // T_i * (c_i + ...)
    else if (q.kind[sc_slot1(i)] == CK_ANY) muls += 1;
  }
  if (out) *out = q;
  return muls;
}

static void sc_check_terms(const SumcheckTerm *terms, int n_terms, int k) {
  if (n_terms > 64) throw Error(TNS_ERR_INVALID_PARAMETERS, "at most 64 sum-check terms");
  for (int t = 0; t < n_terms; t++)
    for (int j = 0; j < 3; j++)
      if (terms[t].tab[j] >= k) throw Error(TNS_ERR_INVALID_PARAMETERS, "term references a missing table");
}

// The table order with the fewest products (ties: the caller's order), and its nested form.
static ScPoly sc_poly(const SumcheckTerm *terms, int n_terms, int k, int perm[MAX_SC_TABLES]) {
  sc_check_terms(terms, n_terms, k);
  int p[MAX_SC_TABLES] = {0, 1, 2, 3};
  int best = -1;
  do {
    const int m = sc_poly_for(terms, n_terms, k, p, nullptr);
    if (best < 0 || m < best) {
      best = m;
      std::copy(p, p + MAX_SC_TABLES, perm);
    }
  } while (std::next_permutation(p, p + k));
  ScPoly q;
  sc_poly_for(terms, n_terms, k, perm, &q);
  return q;
}

// the composition at one point of the caller's table order (src/sumcheck.rs:104)
static Fr eval_composition_host(const Fr *vals, const SumcheckTerm *terms, int n_terms) {
  Fr s = Fr::zero();
  for (int t = 0; t < n_terms; t++) {
    Fr p = terms[t].coeff;
    for (int j = 0; j < 3; j++)
      if (terms[t].tab[j] >= 0) p = mul(p, vals[terms[t].tab[j]]);
    s = add(s, p);
  }
  return s;
}

// ---------------------------------------------------------------- wave/block reductions
__device__ __forceinline__ Fr shfl_down_fr(const Fr &a, int d) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = __shfl_down(a.v[i], d, 64);
  return r;
}

// Sum NV field elements across the block; thread 0 gets the result.  blockDim <= 1024.
template <int NV>
__device__ void block_sum_fr(Fr (&v)[NV], Fr *lds /* [NV][16] */) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
    for (int k = 0; k < NV; k++) {
      Fr o = shfl_down_fr(v[k], d);
      if (lane + d < 64) v[k] = add(v[k], o);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NV; k++) lds[k * 16 + wid] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 0; k < NV; k++) {
      Fr s = lds[k * 16];
      for (int w = 1; w < nw; w++) s = add(s, lds[k * 16 + w]);
      v[k] = s;
    }
  }
}

// ---------------------------------------------------------------- the lazy domain
// The round kernels' arithmetic runs in the lazy domain [0, 2M] of the MSM accumulation
// (bn254.hpp): products skip the final conditional subtraction (inputs <= 2M give results < 2M,
// 4M < 2^256), sums and differences reduce against 2M; values are canonicalised only where they
// leave the kernel (the round sums, the final table values).
__device__ __forceinline__ Fr sc_canon(Fr a) {
  reduce_once(a);  // [0, 2M] -> [0, M]
  reduce_once(a);  // M -> 0
  return a;
}
__device__ __forceinline__ Fr sc_mul(const Fr &a, const Fr &b) { return mul_lazy_dev(a, b); }
__device__ __forceinline__ Fr sc_sqr(const Fr &a) { return sqr_lazy_dev(a); }
__device__ __forceinline__ Fr sc_cmul(int32_t kind, const Fr &c, const Fr &v) {
  if (kind == CK_ONE) return v;
  if (kind == CK_MONE) return const_minus_dev<FrCfg, true>(v);  // 2M - v
  if (kind == CK_TWO) return add2_dev(v, v);
  return sc_mul(c, v);
}

// the composition at one point (table values v[0..K)), nested form of ScPoly; i, j, l are
// template parameters so every table value and coefficient slot is a compile-time index
template <int K, int I, int J, int L>
__device__ __forceinline__ void sc_eval_l(const ScPoly &q, const Fr (&v)[K], Fr &in2) {
  if constexpr (L < K) {
    constexpr int s3 = sc_slot3(I, J, L);
    if (q.kind[s3]) in2 = add2_dev(in2, sc_cmul(q.kind[s3], q.coef[s3], v[L]));
    sc_eval_l<K, I, J, L + 1>(q, v, in2);
  }
}
template <int K, int I, int J>
__device__ __forceinline__ void sc_eval_j(const ScPoly &q, const Fr (&v)[K], Fr &inner) {
  if constexpr (J < K) {
    if (q.has_ij[I][J]) {
      constexpr int s2 = sc_slot2(I, J);
      if (!q.ij_lin[I][J]) {
        inner = add2_dev(inner, sc_cmul(q.kind[s2], q.coef[s2], v[J]));
      } else if (q.ij_sq[I][J]) {  // c T_j^2: the dedicated square
              constexpr int s3 = sc_slot3(I, J, J);
        inner = add2_dev(inner, sc_cmul(q.kind[s3], q.coef[s3], sc_sqr(v[J])));
      } else {
              Fr in2 = q.coef[s2];
        sc_eval_l<K, I, J, J>(q, v, in2);
        inner = add2_dev(inner, sc_mul(v[J], in2));
      }
    }
    sc_eval_j<K, I, J + 1>(q, v, inner);
  }
}
template <int K, int I>
__device__ __forceinline__ void sc_eval_i(const ScPoly &q, const Fr (&v)[K], Fr &acc) {
  if constexpr (I < K) {
    if (q.has_i[I]) {
      constexpr int s1 = sc_slot1(I);
      if (!q.i_lin[I]) {
        acc = add2_dev(acc, sc_cmul(q.kind[s1], q.coef[s1], v[I]));
      } else {
              Fr inner = q.coef[s1];
        sc_eval_j<K, I, I>(q, v, inner);
        acc = add2_dev(acc, sc_mul(v[I], inner));
      }
    }
    sc_eval_i<K, I + 1>(q, v, acc);
  }
}
template <int K>
__device__ __forceinline__ Fr sc_eval(const ScPoly &q, const Fr (&v)[K]) {
  Fr acc = q.coef[0];  // the constant (zero when absent)
  sc_eval_i<K, 0>(q, v, acc);
  return acc;
}

}  // namespace tns
