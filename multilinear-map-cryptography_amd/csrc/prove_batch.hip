// prove_batch.hip -- a batch of Twist or Shout proofs over one SRS in one call.
//
// Twist::prove (src/twist.rs:107-252) and Shout::prove (src/shout.rs:97-222) for `batch` independent
// traces of one shape.  prove.hip runs two commitment MSMs, a fold chain and two opening MSMs per
// proof; below the sizes where one MSM fills the device that fixed chain of launches and host waits
// is the cost.  Here every stage runs once for all proofs:
//   tables   one row-aware kernel writes the Montgomery address / index rows, zero-padded to N;
//   commit   commit_evals_batch (kzg_batch.hip) of the narrow rows and of the full-width rows;
//   host     one transcript per proof (zero_closure_transcript, prove.hip): all batch * nv
//            challenges and all opening points exist before a fold or an opening is queued, and
//            reach the device in one copy;
//   folds    T'[s] = T[2s] + r_{b,k} (T[2s+1] - T[2s]) for every proof and table, one launch per
//            round down to 512 entries, then one launch for the rest (fold_batch, zero_folds.hip);
//   open     open_evals_batch_points with two rows a point (a proof's two vectors share z).
// Every proof is byte for byte what the single prover returns for its row.  prove_batch_plan.hpp
// decides the route; on the rows route the single prover runs row by row.
#include "abi.hpp"
#include "prove_batch_plan.hpp"

namespace tns {

// mont[b N + i] = in[b n_in + i] as a Montgomery Fr (i < n_in), zero for n_in <= i < N
__global__ void __launch_bounds__(256) k_rows_u64_tables(const uint64_t *__restrict__ in, size_t n_in, size_t N,
                                                         size_t rows, Fr *__restrict__ mont) {
  const size_t total = rows * N;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t b = e / N, i = e - b * N;
    mont[e] = i < n_in ? from_u64<FrCfg>(in[b * n_in + i]) : Fr::zero();
  }
}

namespace {

// the checks both batched provers share, after the NULL handles; true: nothing to do
bool prove_batch_checks(const tns_srs *srs, size_t batch, const void *out) {
  if (batch == 0) return true;
  if (!out) throw Error(TNS_ERR_INVALID_PARAMETERS, "null input or output array");
  const Srs &s = srs->s;
  if (s.first != 0 || s.held < s.n)
    throw Error(TNS_ERR_INVALID_PARAMETERS, "batched calls need the whole SRS (this is a shard)");
  return false;
}
void check_scalars(size_t batch, size_t N) {
  if (batch > BATCH_MAX_SCALARS / N) throw Error(TNS_ERR_INVALID_PARAMETERS, "batch * n exceeds 2^32 scalars");
}

// rows of n_in Fr (host or device) -> rows of N Fr on the device, zero-padded; a resident row set of
// full length is used in place
const Fr *padded_rows(Ctx *c, const uint64_t *in, size_t n_in, size_t N, size_t rows, bool resident, DevBuf &buf) {
  if (resident && n_in == N) return (const Fr *)in;
  Fr *p = (Fr *)buf.ensure(sizeof(Fr) * rows * N);
  if (n_in < N) TNS_HIP(hipMemsetAsync(p, 0, sizeof(Fr) * rows * N, c->stream));
  if (n_in)
    TNS_HIP(hipMemcpy2DAsync(p, sizeof(Fr) * N, in, sizeof(Fr) * n_in, sizeof(Fr) * n_in, rows,
                             resident ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
  return p;
}

struct BatchedProof {
  const char *label[2];        // the commitments' transcript labels (src/twist.rs:170-174, src/shout.rs:137-141)
  const Fr *rows[2];           // the committed vectors, `batch` rows of nodes[k] entries, in commitment order
  size_t nodes[2];
  unsigned nv;                 // sum-check rounds
  FoldIn fold;                 // the tables the closure evaluates, of 2^nv entries a proof
  int ntab;
};

// The batched route from the commitments on: what finish_proof and fill_common_tail (prove.hip) do
// for one proof, for all of them.
void finish_batch(tns_ctx *ctx, const Srs &srs, const BatchedProof &bp, size_t batch, const BatchLimits &lim,
                  tns_proof *out, ProveBatchReport &rep) {
  Ctx *c = &ctx->c;
  hipStream_t st = c->stream;
  const unsigned nv = bp.nv;
  const size_t NF = (size_t)1 << nv;
  // ---- commitments: the rows of one width per call (a batch's window plan comes from its widest scalar)
  double *tm = ctx->timing;  // [2] commitments, [3] the host transcripts, [4] folds and openings
  Timer t_com;
  std::vector<G1Affine> cm[2];
  for (int k = 0; k < 2; k++) {
    cm[k].resize(batch);
    commit_evals_batch(c, srs, bp.rows[k], bp.nodes[k], batch, lim, cm[k].data(), &rep.commit[k]);
  }
  tm[2] = t_com.ms();
  // ---- one transcript per proof (finish_proof, fill_common_tail): every challenge and opening
  // point before any fold or opening is queued
  Timer t_host;
  std::vector<Fr> chal(batch * (size_t)nv), z(batch);
  for (size_t b = 0; b < batch; b++) {  // (nv >= 1 on this route: every proof has an opening point)
    std::memset(&out[b], 0, sizeof out[b]);
    const G1Affine cmb[2] = {cm[0][b], cm[1][b]};
    z[b] = zero_closure_transcript(bp.label[0], bp.label[1], cmb, nv, &chal[b * nv], &out[b]);
  }
  tm[3] = t_host.ms();
  // ---- folds
  Timer t_open;
  const size_t tabs = batch * (size_t)bp.ntab;
  DevBuf cb, fb;
  Fr *d_chal = (Fr *)cb.ensure(sizeof(Fr) * (chal.size() + tabs)), *d_finals = d_chal + chal.size();
  Fr *f0 = nullptr, *f1 = nullptr;
  if (NF > FOLD_TAIL) {
    f0 = (Fr *)fb.ensure(sizeof(Fr) * tabs * (NF / 2 + NF / 4));
    f1 = f0 + tabs * (NF / 2);
  }
  std::vector<Fr> finals(tabs), vals(2 * batch);
  std::vector<G1Affine> pi(2 * batch);
  DevBuf yb;
  try {
    TNS_HIP(hipMemcpyAsync(d_chal, chal.data(), sizeof(Fr) * chal.size(), hipMemcpyHostToDevice, st));
    fold_batch(c, bp.fold, bp.ntab, NF, batch, nv, d_chal, f0, f1, d_finals);
    TNS_HIP(hipMemcpyAsync(finals.data(), d_finals, sizeof(Fr) * tabs, hipMemcpyDeviceToHost, st));
    // ---- openings
    if (bp.nodes[0] == bp.nodes[1]) {  // rows 2b, 2b + 1: proof b's two vectors, sharing its point
      const size_t n = bp.nodes[0];
      Fr *y = (Fr *)yb.ensure(sizeof(Fr) * 2 * batch * n);
      for (int k = 0; k < 2; k++)
        TNS_HIP(hipMemcpy2DAsync(y + k * n, sizeof(Fr) * 2 * n, bp.rows[k], sizeof(Fr) * n, sizeof(Fr) * n, batch,
                                 hipMemcpyDeviceToDevice, st));
      rep.open_calls = 1;
      rep.rows_per_point = 2;
      open_evals_batch_points(c, srs, y, n, 2 * batch, z.data(), 2, lim, vals.data(), pi.data(), &rep.open[0]);
    } else {  // Shout with T != M: the table rows and the index rows, a call each
      rep.open_calls = 2;
      rep.rows_per_point = 1;
      std::vector<Fr> v1(batch);
      std::vector<G1Affine> p1(batch);
      for (int k = 0; k < 2; k++) {
        open_evals_batch_points(c, srs, bp.rows[k], bp.nodes[k], batch, z.data(), 1, lim, v1.data(), p1.data(),
                                &rep.open[k]);
        for (size_t b = 0; b < batch; b++) {
          vals[2 * b + k] = v1[b];
          pi[2 * b + k] = p1[b];
        }
      }
    }
    TNS_HIP(hipStreamSynchronize(st));
  } catch (...) {  // the call's buffers die with the error: nothing may still run on them
    (void)hipStreamSynchronize(st);
    throw;
  }
  tm[4] = t_open.ms();
  for (size_t b = 0; b < batch; b++) {
    tns_proof *o = &out[b];
    for (int k = 0; k < 2; k++) {
      store_proj(pi[2 * b + k], o->opening_proofs[k]);
      std::memcpy(o->final_evaluations[k], &vals[2 * b + k], 32);
    }
    o->num_openings = 2;
    for (int t = 0; t < bp.ntab; t++) std::memcpy(o->final_mle_evals[t], &finals[b * bp.ntab + t], 32);
  }
}

bool basis_for(Ctx *c, const Srs &srs, size_t n) { return n <= srs.n && lagrange_basis_dev(c, srs, n, 0, n) != nullptr; }

// On every exit: nothing queued on the context's streams is still running (the single provers of
// the rows route use the side stream)
struct Drain {
  Ctx *c;
  ~Drain() {
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->side);
  }
};

void zero_timing(tns_ctx *ctx) {
  for (int i = 0; i < 6; i++) ctx->timing[i] = 0;
}

// What both batched provers do around their protocol: the checks every call shares, the route, the
// report, the drain, the timing and the rows route.  The protocol supplies
//   checks   its own argument checks, in the single prover's order; returns the padded node counts
//            (wide, narrow) of its two committed vectors;
//   batched  the batched route: the inputs to the device, its tables, finish_batch;
//   row      the single prover on row b (it takes the context lock itself).
int prove_batch(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, size_t batch, tns_proof *out,
                const BatchLimits &lim, ProveBatchReport *rep_out,
                const std::function<std::pair<size_t, size_t>()> &checks,
                const std::function<void(Ctx *, ProveBatchReport &)> &batched, const std::function<int(size_t)> &row) {
  ProveBatchReport rep;
  rep.route = BATCH_ROUTE_ROWS;
  Timer total;
  int status = guarded([&]() {
    if (!ctx || !srs || !params) throw Error(TNS_ERR_INVALID_PARAMETERS, "null context, SRS or parameters");
    if (prove_batch_checks(srs, batch, out)) return (int)TNS_OK;
    ProveBatchShape shape;
    shape.batch = batch;
    std::tie(shape.n_wide, shape.n_narrow) = checks();
    {
      CtxScope g(&ctx->c);
      Ctx *c = &ctx->c;
      Drain drain{c};
      if (shape.n_narrow >= 2) {
        shape.basis_wide = basis_for(c, srs->s, shape.n_wide);
        shape.basis_narrow = shape.n_wide == shape.n_narrow ? shape.basis_wide : basis_for(c, srs->s, shape.n_narrow);
      }
      rep.route = plan_prove_batch(shape, lim).route;
      if (rep.route == BATCH_ROUTE_BATCHED) {
        zero_timing(ctx);
        TNS_HIP(hipStreamSynchronize(c->side));  // a failed earlier proof's folds may still read the tables
        batched(c, rep);
        ctx->timing[5] = total.ms();
        return (int)TNS_OK;
      }
    }
    for (size_t b = 0; b < batch; b++) {
      const int st = row(b);
      if (st != TNS_OK) return st;  // (its message is the last error)
    }
    zero_timing(ctx);
    ctx->timing[5] = total.ms();
    return (int)TNS_OK;
  });
  if (rep_out) *rep_out = rep;
  return status;
}

}  // namespace

int twist_prove_batch(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, const uint64_t *addr,
                      const uint64_t *value, const uint8_t *is_write, size_t n_ops, size_t batch, tns_proof *out,
                      bool resident, const BatchLimits &lim, ProveBatchReport *rep_out) {
  size_t N = 0;
  auto checks = [&]() {
    if (n_ops && (!addr || !value || !is_write)) throw Error(TNS_ERR_INVALID_PARAMETERS, "null input or output array");
    N = next_pow2(n_ops);
    check_scalars(batch, N);
    if (n_ops > params->max_operations) throw Error(TNS_ERR_INVALID_PARAMETERS, "Too many operations");  // src/twist.rs:108-112
    if (ilog2_exact(N) > TNS_MAX_ROUNDS) throw Error(TNS_ERR_INVALID_PARAMETERS, "trace too long");
    return std::make_pair(N, N);
  };
  auto batched = [&](Ctx *c, ProveBatchReport &rep) {
    DevBuf ab, vb, rb, flb;
    const uint64_t *d_addr = (const uint64_t *)on_device(c, addr, 8 * batch * n_ops, resident, rb);
    const uint8_t *d_fl = (const uint8_t *)on_device(c, is_write, batch * n_ops, resident, flb);
    Fr *A = (Fr *)ab.ensure(sizeof(Fr) * batch * N);
    k_rows_u64_tables<<<grid_for(batch * N, 256, 1u << 16), 256, 0, c->stream>>>(d_addr, n_ops, N, batch, A);
    TNS_LAUNCH_CHECK();
    const Fr *V = padded_rows(c, value, n_ops, N, batch, resident, vb);
    BatchedProof bp;
    bp.label[0] = "address_commitment";
    bp.label[1] = "value_commitment";
    bp.rows[0] = A;
    bp.rows[1] = V;
    bp.nodes[0] = bp.nodes[1] = N;
    bp.nv = ilog2_exact(N);
    bp.fold.tab[0] = A;
    bp.fold.tab[1] = V;
    bp.fold.flags = d_fl;
    bp.fold.n_flags = n_ops;
    bp.fold.n_fr = 2;
    bp.ntab = 3;
    finish_batch(ctx, srs->s, bp, batch, lim, out, rep);
  };
  auto row = [&](size_t b) {
    return resident ? tns_twist_prove_device(ctx, srs, params, addr + b * n_ops, value + 4 * b * n_ops,
                                             is_write + b * n_ops, n_ops, &out[b])
                    : tns_twist_prove(ctx, srs, params, addr + b * n_ops, value + 4 * b * n_ops, is_write + b * n_ops,
                                      n_ops, &out[b]);
  };
  return prove_batch(ctx, srs, params, batch, out, lim, rep_out, checks, batched, row);
}

int shout_prove_batch(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, const uint64_t *entries,
                      size_t n_entries, const uint64_t *indices, size_t n_lookups, size_t batch, tns_proof *out,
                      bool resident, const BatchLimits &lim, ProveBatchReport *rep_out) {
  size_t T = 0, M = 0;
  auto checks = [&]() {
    if ((n_entries && !entries) || (n_lookups && !indices))
      throw Error(TNS_ERR_INVALID_PARAMETERS, "null input or output array");
    T = next_pow2(n_entries), M = next_pow2(n_lookups);  // src/shout.rs:105, :116
    check_scalars(batch, std::max(T, M));
    if (n_lookups > params->max_operations)  // src/shout.rs:98-102
      throw Error(TNS_ERR_INVALID_PARAMETERS, "Too many lookup operations");
    if (ilog2_exact(M) > TNS_MAX_ROUNDS) throw Error(TNS_ERR_INVALID_PARAMETERS, "too many lookups");
    return std::make_pair(T, M);
  };
  auto batched = [&](Ctx *c, ProveBatchReport &rep) {
    hipStream_t st = c->stream;
    DevBuf tb, ib, rb, badb;
    const uint64_t *d_idx = (const uint64_t *)on_device(c, indices, 8 * batch * n_lookups, resident, rb);
    // the bounds over all rows: one bad index fails the call
    if (index_out_of_bounds(st, d_idx, batch * n_lookups, n_entries, (unsigned *)badb.ensure(sizeof(unsigned))))
      throw Error(TNS_ERR_INVALID_PARAMETERS, "Lookup index out of bounds");
    Fr *I = (Fr *)ib.ensure(sizeof(Fr) * batch * M);
    k_rows_u64_tables<<<grid_for(batch * M, 256, 1u << 16), 256, 0, st>>>(d_idx, n_lookups, M, batch, I);
    TNS_LAUNCH_CHECK();
    const Fr *TB = padded_rows(c, entries, n_entries, T, batch, resident, tb);
    BatchedProof bp;
    bp.label[0] = "table_commitment";
    bp.label[1] = "index_commitment";
    bp.rows[0] = TB;
    bp.rows[1] = I;
    bp.nodes[0] = T;
    bp.nodes[1] = M;
    bp.nv = ilog2_exact(M);
    bp.fold.tab[0] = I;  // the closure evaluates only the index MLE (src/shout.rs:175)
    bp.fold.tab[1] = nullptr;
    bp.fold.flags = nullptr;
    bp.fold.n_flags = 0;
    bp.fold.n_fr = 1;
    bp.ntab = 1;
    finish_batch(ctx, srs->s, bp, batch, lim, out, rep);
  };
  auto row = [&](size_t b) {
    return resident ? tns_shout_prove_device(ctx, srs, params, entries + 4 * b * n_entries, n_entries,
                                             indices + b * n_lookups, n_lookups, &out[b])
                    : tns_shout_prove(ctx, srs, params, entries + 4 * b * n_entries, n_entries,
                                      indices + b * n_lookups, n_lookups, &out[b]);
  };
  return prove_batch(ctx, srs, params, batch, out, lim, rep_out, checks, batched, row);
}

}  // namespace tns

using namespace tns;

extern "C" {

int tns_twist_prove_batch(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, const uint64_t *addr,
                          const uint64_t *value, const uint8_t *is_write, size_t n_ops, size_t batch, tns_proof *out) {
  return twist_prove_batch(ctx, srs, params, addr, value, is_write, n_ops, batch, out, false, BatchLimits(), nullptr);
}
int tns_twist_prove_batch_device(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, const uint64_t *d_addr,
                                 const uint64_t *d_value, const uint8_t *d_is_write, size_t n_ops, size_t batch,
                                 tns_proof *out) {
  return twist_prove_batch(ctx, srs, params, d_addr, d_value, d_is_write, n_ops, batch, out, true, BatchLimits(),
                           nullptr);
}
int tns_shout_prove_batch(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, const uint64_t *entries,
                          size_t n_entries, const uint64_t *indices, size_t n_lookups, size_t batch, tns_proof *out) {
  return shout_prove_batch(ctx, srs, params, entries, n_entries, indices, n_lookups, batch, out, false, BatchLimits(),
                           nullptr);
}
int tns_shout_prove_batch_device(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, const uint64_t *d_entries,
                                 size_t n_entries, const uint64_t *d_indices, size_t n_lookups, size_t batch,
                                 tns_proof *out) {
  return shout_prove_batch(ctx, srs, params, d_entries, n_entries, d_indices, n_lookups, batch, out, true, BatchLimits(),
                           nullptr);
}

}  // extern "C"
