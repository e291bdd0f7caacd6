// zero_folds.hip -- binding tables at challenges that are known before any fold runs.
//
// The zero-constraint sum-check of Twist / Shout (src/twist.rs:186-214, src/shout.rs:160-184):
// every round polynomial is [0, 0, 0, 0], so the transcript alone yields the challenges
// (prove.hip zero_closure_transcript) and the host has all of them before any fold runs.  What is
// left of the sum-check is the MLE values the closure evaluates (src/sumcheck.rs:104): each table
// bound at every challenge, T'[s] = T[2s] + r (T[2s+1] - T[2s]) per round, LSB first.  That is pure
// device work with no host wait, and two chains do it, each tuned for its regime:
//
//   the single chain (sumcheck_zero_folds_async; the single provers of prove.hip): up to 4 huge
//     tables of one proof, one challenge a round as a kernel argument.  It streams the tables from
//     HBM three rounds a pass (k_sc_fold3: one read per three rounds; the 0/1 op-type table as its
//     flag bytes), a round a pass where fewer than three are left (k_sc_fold), and the last 12
//     rounds in one workgroup (k_sc_fold_tail).  Launched on a side stream, it runs under the
//     openings.
//   the batched chain (fold_batch; the batched provers of prove_batch.hip): many small tables --
//     every table of every proof of a batch, each proof with challenges of its own, read from
//     device memory.  One launch a round over all tables down to 512 entries (k_fold_first,
//     k_fold_round), then a block a table binds the rest in LDS (k_fold_tail).
//
// The two are not merged: nobody has measured one form in the other's regime.  Neither writes its
// input tables.
#include <hip/hip_runtime.h>

#include <cstring>

#include "ctx.hpp"
#include "host.hpp"
#include "sc_tables.hpp"

namespace tns {

// ---------------------------------------------------------------- the single chain
// A fold by r: T'[s] = T[2s] + r (T[2s+1] - T[2s]) for 2P outputs (the single-round passes; 2P
// entries written, 4P read).
__global__ void __launch_bounds__(256) k_sc_fold(ScTables t, int k, size_t P, Fr r) {
  for (size_t s = blockIdx.x * (size_t)blockDim.x + threadIdx.x; s < P; s += (size_t)gridDim.x * blockDim.x) {
#pragma unroll
    for (int i = 0; i < MAX_SC_TABLES; i++) {
      if (i < k) {
        const Fr *p = t.in[i] + 4 * s;
        const Fr x0 = p[0], x1 = p[1], x2 = p[2], x3 = p[3];
        t.out[i][2 * s] = add(x0, mul(r, sub(x1, x0)));
        t.out[i][2 * s + 1] = add(x2, mul(r, sub(x3, x2)));
      }
    }
  }
}

// The last m folds of the chain in one workgroup.  Tables of 2^m entries in a[]; fold j binds
// ch[j] (LSB first, as k_sc_fold) and ping-pongs a -> b -> c -> b ...; out[i] = table i bound at
// all m challenges.  Replaces m - 1 small k_sc_fold launches and the k final k_mle_fold launches
// (each ~20 us of launch gap).
struct ScTail {
  const Fr *a[MAX_SC_TABLES];  // first input (may be the caller's table: only read)
  Fr *b[MAX_SC_TABLES], *c[MAX_SC_TABLES];  // fold 0 -> b, then c, b, c, ...
};
constexpr unsigned SC_TAIL_LOG = 12;  // tables of <= 2^12 entries fold in the tail kernel

__global__ void __launch_bounds__(1024) k_sc_fold_tail(ScTail t, int k, int m, const Fr *__restrict__ ch,
                                                       Fr *__restrict__ out) {
  for (int j = 0; j < m; j++) {
    const Fr r = ch[j];
    const unsigned half = 1u << (m - 1 - j);
    for (int i = 0; i < k; i++) {
      const Fr *in = j == 0 ? t.a[i] : (j & 1) ? t.b[i] : t.c[i];
      Fr *o = (j & 1) ? t.c[i] : t.b[i];
      for (unsigned s = threadIdx.x; s < half; s += blockDim.x) {
        const Fr x0 = in[2 * s], x1 = in[2 * s + 1];
        o[s] = add(x0, mul(r, sub(x1, x0)));
      }
    }
    __syncthreads();  // fold j's outputs are fold j+1's inputs (other threads' entries)
  }
  if (threadIdx.x == 0)
    for (int i = 0; i < k; i++) out[i] = ((m - 1) & 1 ? t.c[i] : t.b[i])[0];
}

// three folds in one pass (challenges r0, r1, r2 of consecutive rounds): out[s] from
// in[8s .. 8s + 7] -- one read of the tables per three rounds instead of per round
// flags (optional): the last table is 0/1 flags given as bytes (entries >= n_flags are 0), so its
// first fold is a select among 0, 1, r0 and 1 - r0 -- the table itself never exists
__global__ void __launch_bounds__(256) k_sc_fold3(ScTables t, int k, size_t P, Fr r0, Fr r1, Fr r2,
                                                  const uint8_t *__restrict__ flags, size_t n_flags) {
  const Fr one = Fr::one(), omr = sub(Fr::one(), r0);
  for (size_t s = blockIdx.x * (size_t)blockDim.x + threadIdx.x; s < P; s += (size_t)gridDim.x * blockDim.x) {
#pragma unroll
    for (int i = 0; i < MAX_SC_TABLES; i++) {
      if (i < k) {
        Fr a[4];
        if (flags && i == k - 1) {
          uint32_t f[8];
          if (8 * s + 8 <= n_flags && ((uintptr_t)flags & 7) == 0) {
            const uint2 w = *reinterpret_cast<const uint2 *>(flags + 8 * s);  // 8-byte aligned
#pragma unroll
            for (int j = 0; j < 4; j++) {
              f[j] = (w.x >> (8 * j)) & 0xff;
              f[4 + j] = (w.y >> (8 * j)) & 0xff;
            }
          } else {
#pragma unroll
            for (int j = 0; j < 8; j++) f[j] = 8 * s + j < n_flags ? flags[8 * s + j] : 0u;
          }
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const bool f0 = f[2 * j] != 0, f1 = f[2 * j + 1] != 0;  // f0 + r0 (f1 - f0)
            a[j] = f0 ? (f1 ? one : omr) : (f1 ? r0 : Fr::zero());
          }
        } else {
          const Fr *p = t.in[i] + 8 * s;
          Fr x[8];
#pragma unroll
          for (int j = 0; j < 8; j++) x[j] = p[j];
#pragma unroll
          for (int j = 0; j < 4; j++) a[j] = add(x[2 * j], mul(r0, sub(x[2 * j + 1], x[2 * j])));
        }
        const Fr b0 = add(a[0], mul(r1, sub(a[1], a[0]))), b1 = add(a[2], mul(r1, sub(a[3], a[2])));
        t.out[i][s] = add(b0, mul(r2, sub(b1, b0)));
      }
    }
  }
}

static unsigned sc_tail_round(unsigned nv) { return std::max(1u, nv + 1 - std::min(nv, SC_TAIL_LOG)); }

bool sumcheck_folds_take_flag_bytes(unsigned nv) { return sc_tail_round(nv) > 3; }

// The k tables bound at chal_pinned[0 .. nv) land in d_out; everything is queued on `st`.
void sumcheck_zero_folds_async(Ctx *c, hipStream_t st, Fr *const *tables, int k, unsigned nv, const Fr *chal_pinned,
                               Fr *d_out, const uint8_t *flags, size_t n_flags) {
  if (k < 1 || k > MAX_SC_TABLES) throw Error(TNS_ERR_INVALID_PARAMETERS, "at most 4 sum-check tables");
  if (flags && !sumcheck_folds_take_flag_bytes(nv))
    throw Error(TNS_ERR_SUMCHECK, "flag bytes need a first three-round fold pass");
  if (nv == 0) {
    for (int i = 0; i < k; i++) TNS_HIP(hipMemcpyAsync(d_out + i, tables[i], sizeof(Fr), hipMemcpyDeviceToDevice, st));
    return;
  }
  const size_t n = (size_t)1 << nv;
  Fr *bufB[MAX_SC_TABLES], *bufC[MAX_SC_TABLES];
  for (int i = 0; i < k; i++) {
    bufB[i] = (Fr *)c->sc.half[i].ensure(sizeof(Fr) * (n / 2 + 1));
    bufC[i] = (Fr *)c->sc.pong[i].ensure(sizeof(Fr) * (n / 4 + 1));
  }
  Fr *d_ch = (Fr *)c->sc.chal.ensure(sizeof(Fr) * nv);
  TNS_HIP(hipMemcpyAsync(d_ch, chal_pinned, sizeof(Fr) * nv, hipMemcpyHostToDevice, st));
  // rounds 1 .. tail_rnd - 1 fold by r_{rnd-1} in k_sc_fold; the rest (tables of <= 2^12) in
  // one k_sc_fold_tail workgroup, down to one value per table
  const unsigned tail_rnd = sc_tail_round(nv);
  Fr *src[MAX_SC_TABLES], *dst[MAX_SC_TABLES];
  for (int i = 0; i < k; i++) {
    src[i] = tables[i];
    dst[i] = bufB[i];
  }
  Fr ch[64];
  std::memcpy(ch, chal_pinned, sizeof(Fr) * std::min(nv, 64u));
  bool first = true;
  for (unsigned rnd = 1; rnd < tail_rnd;) {
    ScTables tt{};
    for (int i = 0; i < k; i++) {
      tt.in[i] = src[i];
      tt.out[i] = dst[i];
    }
    if (rnd + 2 < tail_rnd) {  // rounds rnd .. rnd + 2 in one pass (one read of the tables per three rounds)
      const size_t P = n >> (rnd + 2);
      TNS_PROF_ON(c, st, "sumcheck_round", 288.0 * (double)P * k);
      k_sc_fold3<<<grid_for(P, 256, 4096), 256, 0, st>>>(tt, k, P, ch[rnd - 1], ch[rnd], ch[rnd + 1],
                                                          first ? flags : nullptr, n_flags);
      TNS_LAUNCH_CHECK();
      rnd += 3;
    } else {
      const size_t P = n >> (rnd + 1);
      TNS_PROF_ON(c, st, "sumcheck_round", 192.0 * (double)P * k);
      k_sc_fold<<<grid_for(P, 256, 2048), 256, 0, st>>>(tt, k, P, ch[rnd - 1]);
      TNS_LAUNCH_CHECK();
      rnd += 1;
    }
    for (int i = 0; i < k; i++) {
      if (first) {  // after the first pass: bufB holds the tables' fold
        src[i] = bufB[i];
        dst[i] = bufC[i];
      } else {
        std::swap(src[i], dst[i]);
      }
    }
    first = false;
  }
  ScTail tl{};
  for (int i = 0; i < k; i++) {
    tl.a[i] = src[i];
    tl.b[i] = dst[i];
    tl.c[i] = first ? bufC[i] : src[i];
  }
  const int m = (int)(nv - tail_rnd + 1);
  TNS_PROF_ON(c, st, "sumcheck_round", 96.0 * (double)(n >> (tail_rnd - 1)) * k);
  k_sc_fold_tail<<<1, 1024, 0, st>>>(tl, k, m, d_ch + (tail_rnd - 1), d_out);
  TNS_LAUNCH_CHECK();
}

// ---------------------------------------------------------------- the batched chain
// Table t of proof b, entry i (FoldIn, ctx.hpp).
__device__ __forceinline__ Fr fold_load(const FoldIn &in, size_t N, size_t b, int t, size_t i) {
  if (t < in.n_fr) return in.tab[t][b * N + i];
  return (i < in.n_flags && in.flags[b * in.n_flags + i]) ? Fr::one() : Fr::zero();
}

// round 0 of every proof and table: out[(b ntab + t) N/2 + s] = T[2s] + r_{b,0} (T[2s+1] - T[2s])
__global__ void __launch_bounds__(256) k_fold_first(FoldIn in, int ntab, size_t N, size_t rows, unsigned nv,
                                                    const Fr *__restrict__ chal, Fr *__restrict__ out) {
  const size_t h = N / 2, total = rows * ntab * h;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t bt = e / h, s = e - bt * h, b = bt / ntab;
    const int t = (int)(bt - b * ntab);
    const Fr lo = fold_load(in, N, b, t, 2 * s), hi = fold_load(in, N, b, t, 2 * s + 1);
    out[e] = add(lo, mul(chal[b * nv + 0], sub(hi, lo)));
  }
}

// round k on the packed tables: src holds `tabs` tables of cur entries, dst tabs tables of cur / 2
__global__ void __launch_bounds__(256) k_fold_round(const Fr *__restrict__ src, size_t cur, size_t tabs, int ntab,
                                                    unsigned nv, unsigned k, const Fr *__restrict__ chal,
                                                    Fr *__restrict__ dst) {
  const size_t h = cur / 2, total = tabs * h;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t bt = e / h, s = e - bt * h, b = bt / ntab;
    const Fr lo = src[bt * cur + 2 * s], hi = src[bt * cur + 2 * s + 1];
    dst[e] = add(lo, mul(chal[b * nv + k], sub(hi, lo)));
  }
}

static_assert(FOLD_TAIL / 2 <= 256, "a round of k_fold_tail is one entry a thread of its 256");

// the rounds k0 .. nv-1 of tables of cur = 2^(nv-k0) <= FOLD_TAIL entries, a block a table:
// finals[b ntab + t] = the table's value at the proof's challenges.  FIRST: cur = N, from the inputs.
template <bool FIRST>
__global__ void __launch_bounds__(256) k_fold_tail(FoldIn in, const Fr *__restrict__ src, size_t cur, size_t tabs,
                                                   int ntab, unsigned nv, unsigned k0, const Fr *__restrict__ chal,
                                                   Fr *__restrict__ finals) {
  __shared__ Fr lds[FOLD_TAIL];
  for (size_t bt = blockIdx.x; bt < tabs; bt += gridDim.x) {
    const size_t b = bt / ntab;
    const int t = (int)(bt - b * ntab);
    for (size_t i = threadIdx.x; i < cur; i += 256) lds[i] = FIRST ? fold_load(in, cur, b, t, i) : src[bt * cur + i];
    __syncthreads();
    unsigned k = k0;
    for (size_t h = cur / 2; h >= 1; h >>= 1, k++) {
      const Fr r = chal[b * nv + k];
      const size_t s = threadIdx.x;  // h <= FOLD_TAIL / 2 = blockDim.x
      Fr v = Fr::zero();
      if (s < h) v = add(lds[2 * s], mul(r, sub(lds[2 * s + 1], lds[2 * s])));
      __syncthreads();
      if (s < h) lds[s] = v;
      __syncthreads();
    }
    if (threadIdx.x == 0) finals[bt] = lds[0];
    __syncthreads();
  }
}

// all tables of all proofs bound at their proofs' challenges (d_chal[b nv + k], LSB-first) into
// d_finals[b ntab + t], on the context stream; f0 / f1: tabs N/2 and tabs N/4 entries of scratch
// (unused when N <= FOLD_TAIL)
void fold_batch(Ctx *c, const FoldIn &in, int ntab, size_t N, size_t rows, unsigned nv, const Fr *d_chal, Fr *f0, Fr *f1,
                Fr *d_finals) {
  TNS_PROF(c, "sumcheck_round", 32.0 * 2 * rows * ntab * N);
  hipStream_t st = c->stream;
  const size_t tabs = rows * (size_t)ntab;
  const unsigned tail_grid = grid_for(tabs, 1, 1u << 16);
  if (N <= FOLD_TAIL) {
    k_fold_tail<true><<<tail_grid, 256, 0, st>>>(in, nullptr, N, tabs, ntab, nv, 0, d_chal, d_finals);
    TNS_LAUNCH_CHECK();
    return;
  }
  k_fold_first<<<grid_for(tabs * (N / 2), 256, 1u << 16), 256, 0, st>>>(in, ntab, N, rows, nv, d_chal, f0);
  TNS_LAUNCH_CHECK();
  size_t cur = N / 2;
  unsigned k = 1;
  Fr *src = f0, *dst = f1;
  while (cur > FOLD_TAIL) {
    k_fold_round<<<grid_for(tabs * (cur / 2), 256, 1u << 16), 256, 0, st>>>(src, cur, tabs, ntab, nv, k, d_chal, dst);
    TNS_LAUNCH_CHECK();
    std::swap(src, dst);
    cur /= 2;
    k++;
  }
  k_fold_tail<false><<<tail_grid, 256, 0, st>>>(in, src, cur, tabs, ntab, nv, k, d_chal, d_finals);
  TNS_LAUNCH_CHECK();
}

}  // namespace tns
