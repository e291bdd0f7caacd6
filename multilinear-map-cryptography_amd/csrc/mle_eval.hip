// mle_eval.hip -- MultilinearExtension::evaluate in one pass, for a batch of tables.
//
// Reference semantics: MultilinearExtension::evaluate (src/polynomials.rs:85-122), variable i <->
// index bit i (LSB first):  value = sum_x T[x] prod_i (x_i ? r_i : 1 - r_i).  mle_evaluate_dev
// (mle.hip) binds one variable a launch through ping-pong scratch, because a prover learns the
// point one coordinate a round.  A verifier knows the whole point before it touches a table, so
// the evaluation is an eq-weighted dot product: every entry read once, one product an entry,
// nothing written but the result.  For `batch` instances of K <= 4 tables of 2^nv entries (the
// layout of tns_sumcheck_prove_batch), instance b at its own point r_b:
//   eq    (nv > 8) one launch builds, per instance, the eq table of the high nv - 8 variables,
//         2^(nv-8) entries shared by the instance's tables;
//   dot   one launch.  nv > 8: lane t of a 256-thread block owns the low index bits t and walks
//         2^log_rpt rows x_hi, acc_j += eq_hi[b][x_hi] T_j[b][x_hi 256 + t] for all K tables at
//         once (eq_hi a uniform load, the table loads coalesced, lazy domain), multiplies once by
//         its own eq_lo[t] -- 8 products from the low coordinates -- and the block sums.
//         nv <= 8: a thread owns one entry and forms the whole weight itself.
// The sum per instance has the three regimes of k_scb_round (sumcheck_batch.hip): an instance is
// part of a wave (nv <= 6: shuffles limited to its lanes), one block (wave sums through LDS), or
// several blocks (per-block partials behind a fence; the last block of the instance to finish
// adds them up and leaves the instance's counter zero for the next call).
// Field sums are exact: the result does not depend on the geometry, and it is canonical.
// Scratch: eq_hi is 1/256 of ONE table, the partials K entries a block of >= 256 K entries read.
#include "abi.hpp"
#include "sc_poly.hpp"

namespace tns {

constexpr unsigned ME_BLOCK_LOG = 8, ME_BLOCK = 1u << ME_BLOCK_LOG;  // 256 threads: four waves

struct MeTables {
  const Fr *t[MAX_SC_TABLES];
};

// prod_{i < m} (bit i of x ? r[i] : 1 - r[i]), canonical
__device__ __forceinline__ Fr me_eq(const Fr *__restrict__ r, unsigned m, uint64_t x) {
  const Fr one = Fr::one();
  Fr w = one;
  for (unsigned i = 0; i < m; i++) {
    const Fr ri = r[i];
    w = mul(w, ((x >> i) & 1) ? ri : sub(one, ri));
  }
  return w;
}

// eq_hi[b 2^h + x] = the weight of the high h = nv - 8 variables of instance b at x; total = batch 2^h
__global__ void __launch_bounds__(ME_BLOCK) k_mle_eq(const Fr *__restrict__ pts, unsigned nv, unsigned h, uint64_t total,
                                                     Fr *__restrict__ eq_hi) {
  const uint64_t g = (uint64_t)blockIdx.x * ME_BLOCK + threadIdx.x;
  if (g >= total) return;
  const uint64_t b = g >> h;
  eq_hi[g] = me_eq(pts + b * nv + ME_BLOCK_LOG, h, g & (((uint64_t)1 << h) - 1));
}

// nv <= 8: entry e = b 2^nv + x of every table at flat index e, one thread an entry; total = batch
// 2^nv.  A partly filled last block reads entry 0 and adds zero.  vals[b K + j].
template <int K>
__global__ void __launch_bounds__(ME_BLOCK)
    k_mle_dot_small(MeTables t, const Fr *__restrict__ pts, unsigned nv, uint64_t total, Fr *__restrict__ vals) {
  __shared__ Fr lds[4 * 16];
  const unsigned tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint64_t e = (uint64_t)blockIdx.x * ME_BLOCK + tid;
  const bool live = e < total;
  const uint64_t el = live ? e : 0;
  const uint64_t b = el >> nv;
  const Fr w = me_eq(pts + b * nv, nv, el & (((uint64_t)1 << nv) - 1));
  Fr a[K];
#pragma unroll
  for (int j = 0; j < K; j++) {
    const Fr p = mul(w, t.t[j][el]);
    a[j] = live ? p : Fr::zero();
  }
  const unsigned P = 1u << nv;
  if (nv <= 6) {  // an instance is 2^nv lanes of this wave
#pragma unroll
    for (unsigned dd = 32; dd > 0; dd >>= 1) {
      if (dd < P) {  // (uniform; the segment's first lane only ever adds lanes of its own segment)
#pragma unroll
        for (int j = 0; j < K; j++) {
          const Fr o = shfl_down_fr(a[j], dd);
          if (lane + dd < 64) a[j] = add(a[j], o);
        }
      }
    }
    if (live && (lane & (P - 1)) == 0) {
#pragma unroll
      for (int j = 0; j < K; j++) vals[b * K + j] = a[j];
    }
    return;
  }
  // an instance is 2 or 4 waves of this block
  const unsigned waves = P >> 6;
#pragma unroll
  for (unsigned dd = 32; dd > 0; dd >>= 1) {
#pragma unroll
    for (int j = 0; j < K; j++) {
      const Fr o = shfl_down_fr(a[j], dd);
      if (lane + dd < 64) a[j] = add(a[j], o);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < K; j++) lds[j * 16 + wid] = a[j];
  }
  __syncthreads();
  if (live && (tid & (P - 1)) == 0) {
#pragma unroll
    for (int j = 0; j < K; j++) {
      Fr s = lds[j * 16 + wid];
      for (unsigned w2 = 1; w2 < waves; w2++) s = add(s, lds[j * 16 + wid + w2]);
      vals[b * K + j] = s;
    }
  }
}

// nv > 8: h = nv - 8 high variables, 2^h rows of 256 entries an instance; a block takes 2^log_rpt
// consecutive rows of one instance, so an instance is 2^(h - log_rpt) whole blocks and every block
// is full.  grid = batch 2^(h - log_rpt).
template <int K>
__global__ void __launch_bounds__(ME_BLOCK)
    k_mle_dot(MeTables t, const Fr *__restrict__ eq_hi, const Fr *__restrict__ pts, unsigned nv, unsigned log_rpt,
              Fr *__restrict__ vals, Fr *__restrict__ partials, unsigned *__restrict__ counters) {
  __shared__ Fr lds[4 * 16];
  __shared__ int last;
  const unsigned tid = threadIdx.x;
  const unsigned h = nv - ME_BLOCK_LOG, log_nblk = h - log_rpt, nblk = 1u << log_nblk;
  const uint64_t b = (uint64_t)blockIdx.x >> log_nblk;
  // the block's first row among the batch 2^h rows of the call (uniform: eq_hi is a scalar load)
  const uint64_t row0 = (b << h) + ((uint64_t)(blockIdx.x & (nblk - 1)) << log_rpt);
  const Fr *__restrict__ wrow = eq_hi + row0;
  Fr acc[K];
#pragma unroll
  for (int j = 0; j < K; j++) acc[j] = Fr::zero();
  const unsigned rows = 1u << log_rpt;
  const uint64_t idx0 = (row0 << ME_BLOCK_LOG) + tid;
  if (rows == 1) {
    const Fr w = wrow[0];
#pragma unroll
    for (int j = 0; j < K; j++) acc[j] = mul_lazy_dev(w, t.t[j][idx0]);
  } else {
    // two rows a trip (rows is a power of two): 2 K independent 32-byte loads in flight a lane
    for (unsigned rr = 0; rr < rows; rr += 2) {
      const uint64_t idx = idx0 + ((uint64_t)rr << ME_BLOCK_LOG);
      Fr v0[K], v1[K];
#pragma unroll
      for (int j = 0; j < K; j++) {
        v0[j] = t.t[j][idx];
        v1[j] = t.t[j][idx + ME_BLOCK];
      }
      const Fr w0 = wrow[rr], w1 = wrow[rr + 1];
#pragma unroll
      for (int j = 0; j < K; j++) {
        acc[j] = add2_dev(acc[j], mul_lazy_dev(w0, v0[j]));
        acc[j] = add2_dev(acc[j], mul_lazy_dev(w1, v1[j]));
      }
    }
  }
  const Fr wl = me_eq(pts + b * nv, ME_BLOCK_LOG, tid);
  Fr a[K];
#pragma unroll
  for (int j = 0; j < K; j++) a[j] = sc_canon(mul_lazy_dev(wl, acc[j]));
  block_sum_fr<K>(a, lds);
  if (nblk == 1) {  // the instance is this block
    if (tid == 0) {
#pragma unroll
      for (int j = 0; j < K; j++) vals[b * K + j] = a[j];
    }
    return;
  }
  if (tid == 0) {
#pragma unroll
    for (int j = 0; j < K; j++) partials[(size_t)K * blockIdx.x + j] = a[j];
    __threadfence();
    last = atomicAdd(&counters[b], 1u) == nblk - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();  // every block's partials (each fenced before its increment) are visible
  const Fr *mine = partials + (size_t)K * ((size_t)b << log_nblk);
#pragma unroll
  for (int j = 0; j < K; j++) a[j] = Fr::zero();
  for (unsigned bb = tid; bb < nblk; bb += ME_BLOCK)
#pragma unroll
    for (int j = 0; j < K; j++) a[j] = add(a[j], mine[(size_t)K * bb + j]);
  block_sum_fr<K>(a, lds);
  if (tid == 0) {
#pragma unroll
    for (int j = 0; j < K; j++) vals[b * K + j] = a[j];
    counters[b] = 0;  // ready for the next call (stream order)
  }
}

namespace {

// rows a thread takes (nv > 8): as many (up to 2^max_log_rows, and an instance's 2^h) as leave the
// launch min_blocks blocks.  More rows amortise the thread's eq_lo products, the block sum and the
// cross-block fence; the accumulators stay K x 8 registers whatever the count, so the count does
// not touch occupancy (106 VGPRs at K = 3, 120 at K = 4: four waves a SIMD).
unsigned me_log_rows(unsigned h, size_t batch, const MleEvalLimits &lim) {
  const uint64_t rows = (uint64_t)batch << h;
  const unsigned cap = std::min(lim.max_log_rows, 16u);
  unsigned l = 0;
  while (l < cap && l < h && (rows >> (l + 1)) >= lim.min_blocks) l++;
  return l;
}

}  // namespace

void mle_evaluate_batch_dev(Ctx *c, const Fr *const *tables, int k, unsigned nv, size_t batch, const Fr *points_host,
                            Fr *values_host, const MleEvalLimits &lim, MleEvalReport *rep_out) {
  MleEvalReport rep;
  if (k > 0 && batch > 0) {
    hipStream_t st = c->stream;
    MleEvalWs &ws = c->mle_eval;
    const size_t n = (size_t)1 << nv;
    Fr *d_pts = (Fr *)ws.points.ensure(sizeof(Fr) * std::max<size_t>(1, batch * nv));
    Fr *d_vals = (Fr *)ws.values.ensure(sizeof(Fr) * batch * k);
    if (nv) TNS_HIP(hipMemcpyAsync(d_pts, points_host, sizeof(Fr) * batch * nv, hipMemcpyHostToDevice, st));
    MeTables tt{};
    for (int j = 0; j < k; j++) tt.t[j] = tables[j];
    const double bytes = (double)sizeof(Fr) * k * batch * n;
    if (nv <= ME_BLOCK_LOG) {
      const uint64_t total = (uint64_t)batch << nv;
      const unsigned g = (unsigned)((total + ME_BLOCK - 1) >> ME_BLOCK_LOG);
      rep.regime = nv <= 6 ? MLE_EVAL_WAVE : MLE_EVAL_BLOCK;
      rep.blocks = g;
      rep.rows_per_thread = 1;
      TNS_PROF(c, "mle_eval_dot", bytes);
      sc_for_tables(k, [&](auto K) {
        k_mle_dot_small<decltype(K)::value><<<g, ME_BLOCK, 0, st>>>(tt, d_pts, nv, total, d_vals);
      });
      TNS_LAUNCH_CHECK();
      rep.launches = 1;
    } else {
      const unsigned h = nv - ME_BLOCK_LOG, log_rpt = me_log_rows(h, batch, lim);
      const uint64_t rows = (uint64_t)batch << h;
      const unsigned g = (unsigned)(rows >> log_rpt);
      rep.regime = log_rpt == h ? MLE_EVAL_BLOCK : MLE_EVAL_BLOCKS;
      rep.blocks = g;
      rep.rows_per_thread = (size_t)1 << log_rpt;
      Fr *eq_hi = (Fr *)ws.eq_hi.ensure(sizeof(Fr) * rows);
      Fr *partials = nullptr;
      unsigned *counters = nullptr;
      if (rep.regime == MLE_EVAL_BLOCKS) {
        partials = (Fr *)ws.partials.ensure(sizeof(Fr) * k * g);
        const bool fresh = ws.counters.bytes < sizeof(unsigned) * batch;
        counters = (unsigned *)ws.counters.ensure(sizeof(unsigned) * batch);
        // (zeroed when allocated; every call leaves them zero)
        if (fresh) TNS_HIP(hipMemsetAsync(counters, 0, ws.counters.bytes, st));
      }
      {
        TNS_PROF(c, "mle_eval_eq", sizeof(Fr) * rows);
        k_mle_eq<<<(unsigned)((rows + ME_BLOCK - 1) >> ME_BLOCK_LOG), ME_BLOCK, 0, st>>>(d_pts, nv, h, rows, eq_hi);
        TNS_LAUNCH_CHECK();
      }
      TNS_PROF(c, "mle_eval_dot", bytes);
      sc_for_tables(k, [&](auto K) {
        k_mle_dot<decltype(K)::value><<<g, ME_BLOCK, 0, st>>>(tt, eq_hi, d_pts, nv, log_rpt, d_vals, partials, counters);
      });
      TNS_LAUNCH_CHECK();
      rep.launches = 2;
    }
    TNS_HIP(hipMemcpyAsync(values_host, d_vals, sizeof(Fr) * batch * k, hipMemcpyDeviceToHost, st));
    TNS_HIP(hipStreamSynchronize(st));
  }
  if (rep_out) *rep_out = rep;
}

int mle_evaluate_batch(tns_ctx *ctx, const uint64_t *const *tables, int n_tables, unsigned nv, size_t batch,
                       const uint64_t *points, uint64_t *values_out, bool resident, const MleEvalLimits &lim,
                       MleEvalReport *rep_out) {
  MleEvalReport rep;
  int status = guarded([&]() {
    if (!ctx) throw Error(TNS_ERR_INVALID_PARAMETERS, "null context");
    if (batch == 0) return (int)TNS_OK;
    if (nv > 30 || n_tables < 0 || n_tables > MAX_SC_TABLES)
      throw Error(TNS_ERR_INVALID_PARAMETERS, "unsupported evaluation shape (<= 4 tables, <= 30 variables)");
    if (n_tables == 0) return (int)TNS_OK;
    sc_check_arrays(tables && values_out && (nv == 0 || points), tables, n_tables, batch, nv);
    CtxScope scope(&ctx->c);
    Ctx *c = &ctx->c;
    StagedTables staged(c, tables, n_tables, (sizeof(Fr) * batch) << nv, resident);
    mle_evaluate_batch_dev(c, staged.tab, n_tables, nv, batch, (const Fr *)points, (Fr *)values_out, lim, &rep);
    return (int)TNS_OK;
  });
  if (rep_out) *rep_out = rep;
  return status;
}

}  // namespace tns

using namespace tns;

extern "C" {

int tns_mle_evaluate_device(tns_ctx *ctx, const uint64_t *d_evals, unsigned nv, const uint64_t *point, uint64_t out[4]) {
  const uint64_t *tabs[1] = {d_evals};
  return mle_evaluate_batch(ctx, tabs, 1, nv, 1, point, out, true, MleEvalLimits(), nullptr);
}
int tns_mle_evaluate_batch(tns_ctx *ctx, const uint64_t *const *tables, int n_tables, unsigned nv, size_t batch,
                           const uint64_t *points, uint64_t *values_out) {
  return mle_evaluate_batch(ctx, tables, n_tables, nv, batch, points, values_out, false, MleEvalLimits(), nullptr);
}
int tns_mle_evaluate_batch_device(tns_ctx *ctx, const uint64_t *const *d_tables, int n_tables, unsigned nv, size_t batch,
                                  const uint64_t *points, uint64_t *values_out) {
  return mle_evaluate_batch(ctx, d_tables, n_tables, nv, batch, points, values_out, true, MleEvalLimits(), nullptr);
}

}  // extern "C"
