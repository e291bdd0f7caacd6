// prove.hip -- the Twist/Shout prove orchestration.
//
// Twist::prove (src/twist.rs:107-252) and Shout::prove (src/shout.rs:97-222) run with
// every bulk vector resident in HBM: one H2D of the trace, exact interpolation
// (interp.hip), two KZG commits (msm.hip), the host transcript, the sum-check fold
// chain (zero_folds.hip), then the two openings (poly.hip synthetic division + msm.hip).
// Only commitments, 4-element round polynomials and challenges cross PCIe.
#include "abi.hpp"

namespace tns {

// shard geometry: `size` ranks over N padded entries (size a power of two <= N)
void check_shard(const Comm &m, size_t N, const char *what) {
  if (m.size & (m.size - 1)) throw Error(TNS_ERR_INVALID_PARAMETERS, "rank count must be a power of two");
  if ((size_t)m.size > N)
    throw Error(TNS_ERR_INVALID_PARAMETERS, std::string("more ranks than padded ") + what + " entries");
}
size_t slice_count(uint64_t n_total, size_t first, size_t L) {
  return n_total <= first ? 0 : (size_t)std::min<uint64_t>(L, n_total - first);
}

// The zero constraint closure (src/twist.rs:186-214, src/shout.rs:160-184) makes every round
// polynomial [0, 0, 0, 0] and final_evaluation 0 (src/sumcheck.rs:77-104), so the transcript alone
// -- the two commitments under the protocol's labels, then the nv zero rounds -- yields the
// challenges, and the opening point after them.
Fr zero_closure_transcript(const char *label0, const char *label1, const G1Affine cm[2], unsigned nv, Fr *chal,
                           tns_proof *out) {
  store_proj(cm[0], out->commitments[0]);
  store_proj(cm[1], out->commitments[1]);
  HostTranscript tr;
  tr.append_label(label0);
  tr.append_fr(commitment_hash(cm[0]));
  tr.append_label(label1);
  tr.append_fr(commitment_hash(cm[1]));
  sumcheck_constant_rounds(tr, nv, Fr::zero(), nullptr, chal);
  out->num_rounds = nv;
  std::memset(out->round_polynomials, 0, 128 * (size_t)nv);  // (a tns_proof's words are not aligned as Fr)
  std::memcpy(out->sumcheck_challenges, chal, 32 * (size_t)nv);
  std::memset(out->final_evaluation, 0, 32);
  // challenge_field_elements("opening_challenges", nv) (src/utils.rs:195-203); only [0] is used
  // (src/twist.rs:219-226, src/shout.rs:189-195), and elements 1..nv-1 only extend a transcript
  // that nothing reads afterwards, so they are not derived (no observable output depends on
  // them; ~0.1 ms of host hashing in front of the openings at nv = 24)
  Fr z = Fr::zero();
  if (nv >= 1) {
    z = tr.challenge("opening_challenges_0");
    std::memcpy(out->opening_point, &z, 32);
  }
  return z;
}

// LookupTable::lookup bounds (src/shout.rs:44-50): whether some idx[i] >= bound.  Zeroes the
// device word `bad`, runs the check on st, copies the word back and waits for st.
__global__ void k_max_index_check(const uint64_t *__restrict__ idx, size_t n, uint64_t bound,
                                  unsigned *__restrict__ bad) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    if (idx[i] >= bound) *bad = 1;
}
bool index_out_of_bounds(hipStream_t st, const uint64_t *idx, size_t n, uint64_t bound, unsigned *bad) {
  unsigned hbad = 0;
  TNS_HIP(hipMemsetAsync(bad, 0, sizeof(unsigned), st));
  k_max_index_check<<<grid_for(n, 256), 256, 0, st>>>(idx, n, bound, bad);
  TNS_LAUNCH_CHECK();
  TNS_HIP(hipMemcpyAsync(&hbad, bad, sizeof hbad, hipMemcpyDeviceToHost, st));
  TNS_HIP(hipStreamSynchronize(st));
  return hbad != 0;
}

}  // namespace tns

using namespace tns;

extern "C" {

// ---------------------------------------------------------------- protocols
// Sum-check over the (zero) constraint closure + the two openings, for the rank's slices.
// The first nv - log2(size) rounds bind variables inside every slice (LSB-first,
// src/polynomials.rs:111-119), so they run locally; the last log2(size) rounds run on
// the host over the one folded value per table and rank (allgathered).
// flags (optional): the last of the mles as 0/1 bytes (sumcheck_zero_folds_async)
static void fill_common_tail(Ctx *c, const Srs &srs, const G1Affine cm[2], const char *label0, const char *label1,
                             Fr *const *mles, int n_mles, unsigned nv, EvalPoly &polyA, EvalPoly &polyB,
                             tns_proof *out, double *timing, Comm &m, const uint8_t *flags = nullptr,
                             size_t n_flags = 0) {
  Timer t_sc;
  unsigned lr = 0;
  while ((1 << lr) < m.size) lr++;
  const unsigned nv_loc = nv - lr;  // check_shard guarantees size <= 2^nv
  if (n_mles < 1 || n_mles > 3) throw Error(TNS_ERR_INVALID_PARAMETERS, "1 to 3 trace tables");
  // all nv rounds run on the host first (the challenges stay in pinned memory: the folds' async
  // copy reads them) ...
  const unsigned nv1 = nv ? nv : 1;
  Fr *chal = (Fr *)c->sc.host.ensure(sizeof(Fr) * (nv1 + 4)), *vals = chal + nv1;
  const Fr z = zero_closure_transcript(label0, label1, cm, nv, chal, out);
  // ... and the folds binding this rank's tables at r_0 .. r_{nv_loc-1} (the MLE values the
  // closure evaluates, src/sumcheck.rs:104) run on the side stream under the openings; their
  // values are collected at the end of the proof
  // (queued behind the quotient kernel instead, under the opening sorts: a tie, 49.19-49.51 vs
  // 49.32-49.51 ms per step, profiles/r04_ab_folds_at.txt)
  // (queued once the openings' barycentric pass is on the device: its launches come first, and the
  // folds' ~80 us of host launches run under its chain kernels, profiles/r06_hiptrace_gaps.txt)
  Fr *d_vals = (Fr *)c->sc.out.ensure(sizeof(Fr) * 4);
  stream_wait(c->side, c->stream);  // the tables were written on the context stream
  bool folds_queued = false;
  auto queue_folds = [&]() {
    if (folds_queued) return;
    folds_queued = true;
    sumcheck_zero_folds_async(c, c->side, mles, n_mles, nv_loc, chal, d_vals, flags, n_flags);
    TNS_HIP(hipMemcpyAsync(vals, d_vals, sizeof(Fr) * n_mles, hipMemcpyDeviceToHost, c->side));
  };
  timing[3] = t_sc.ms();
  Timer t_open;
  // sharded: every rank's folded values travel with the opening partials (one exchange, not two)
  Fr finals[3];
  ExtraPayload fold_x;
  fold_x.data = finals;
  fold_x.bytes = sizeof(Fr) * (size_t)n_mles;
  bool folds_exchanged = false;
  auto folds_ready = [&]() {
    queue_folds();
    TNS_HIP(hipStreamSynchronize(c->side));
    for (int j = 0; j < n_mles; j++) finals[j] = vals[j];
  };
  if (nv >= 1) {
    Fr v[2];
    G1Affine pi[2];
    open_evals_pair(c, srs, polyA, polyB, z, v, pi, c->prove.open_s[0], c->prove.open_s[1], m, lr ? &fold_x : nullptr,
                    folds_ready, queue_folds);
    folds_exchanged = lr > 0;
    store_proj(pi[0], out->opening_proofs[0]);
    store_proj(pi[1], out->opening_proofs[1]);
    std::memcpy(out->final_evaluations[0], &v[0], 32);
    std::memcpy(out->final_evaluations[1], &v[1], 32);
    out->num_openings = 2;
  }
  timing[4] = t_open.ms();
  // the side stream's bound table values; with several ranks each holds its slice's values at
  // r_0 .. r_{nv_loc-1}, and the last lr challenges fold the allgathered rank values
  folds_ready();
  if (lr) {
    std::vector<Fr> all((size_t)n_mles * m.size);  // rank-major
    if (folds_exchanged) std::memcpy(all.data(), fold_x.all.data(), sizeof(Fr) * all.size());
    else all = allgather_fr(c, m, finals, (size_t)n_mles, "sum-check folded table values");
    for (int j = 0; j < n_mles; j++) {
      std::vector<Fr> t(m.size);
      for (int r = 0; r < m.size; r++) t[r] = all[(size_t)r * n_mles + j];
      for (unsigned rnd = nv_loc; rnd < nv; rnd++) {  // T'[s] = T[2s] + r (T[2s+1] - T[2s])
        const size_t h = t.size() / 2;
        for (size_t q = 0; q < h; q++) t[q] = add(t[2 * q], mul(chal[rnd], sub(t[2 * q + 1], t[2 * q])));
        t.resize(h);
      }
      finals[j] = t[0];
    }
  }
  for (int j = 0; j < n_mles; j++) std::memcpy(out->final_mle_evals[j], &finals[j], 32);
}

__global__ void k_write_flags(const uint8_t *__restrict__ in, Fr *__restrict__ out, size_t n_in, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = (i < n_in && in[i]) ? Fr::one() : Fr::zero();
}

// The node ranges the drop-in values arrive in: k equal ranges (Ctx::upload_chunks).  (Splitting the
// last one in two, so the MSM left after the upload is an eighth of the vector, measured equal at
// C4: 56.4-57.5 vs 56.4-57.9 ms per drop-in proof, profiles/r04_ab_upload_split.txt.)
static std::vector<size_t> upload_chunk_offsets(size_t n, int k) {
  std::vector<size_t> off;
  const size_t per = (n + k - 1) / std::max(k, 1);
  for (size_t o = 0; o < n; o += per) off.push_back(o);
  off.push_back(n);
  return off;
}

// On every exit of a prove call (an exception included): nothing this call queued on the side
// stream (the flag table, the zero-closure folds: they read the caller's value / is_write
// buffers in the device-resident entry points) is still running when the call returns.
struct SideDrain {
  Ctx *c;
  ~SideDrain() { (void)hipStreamSynchronize(c->side); }
};

// The close of both prove cores: the transcript of the two commitments (under the protocol's
// labels), the sum-check and the openings, and the wait for the context stream.
static void finish_proof(tns_ctx *ctx, const Srs &srs, const Timer &total, const G1Affine cm[2], const char *label0,
                         const char *label1, Fr *const *mles, int n_mles, unsigned nv, EvalPoly &polyA,
                         EvalPoly &polyB, tns_proof *out, Comm &m, const uint8_t *flags = nullptr,
                         size_t n_flags = 0) {
  fill_common_tail(&ctx->c, srs, cm, label0, label1, mles, n_mles, nv, polyA, polyB, out, ctx->timing, m, flags,
                   n_flags);
  TNS_HIP(hipStreamSynchronize(ctx->c.stream));
  ctx->timing[5] = total.ms();
}

// Twist::prove (src/twist.rs:107-252) for this rank's slice of the trace: operations
// [rank L, rank L + n_local) of n_total, L = next_pow2(n_total) / size.  kind: where
// addr/value/is_write live (H2D or D2D).  size 1 = the unsharded prover.
static void twist_core(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, Comm &m, const uint64_t *addr,
                       const uint64_t *value, const uint8_t *is_write, size_t n_ops, uint64_t n_total,
                       tns_proof *out, hipMemcpyKind kind) {
  Timer total;
  CtxScope g(&ctx->c);
  Ctx *c = &ctx->c;
  hipStream_t st = c->stream;
  std::memset(out, 0, sizeof *out);
  if (n_total > params->max_operations)  // src/twist.rs:108-112
    throw Error(TNS_ERR_INVALID_PARAMETERS, "Too many operations");
  const size_t N = next_pow2(n_total);  // :141 next_power_of_two().max(1)
  const unsigned nv = ilog2_exact(N);
  if (nv > TNS_MAX_ROUNDS) throw Error(TNS_ERR_INVALID_PARAMETERS, "trace too long");
  check_shard(m, N, "trace");
  const size_t L = N / m.size, first = (size_t)m.rank * L;
  if (n_ops != slice_count(n_total, first, L))
    throw Error(TNS_ERR_INVALID_PARAMETERS, "local operation count does not match this rank's slice");
  double *tm = ctx->timing;
  for (int i = 0; i < 6; i++) tm[i] = 0;
  TNS_HIP(hipStreamSynchronize(c->side));  // a failed earlier proof's folds may still read the tables
  SideDrain drain{c};
  HostUpload upload(c);  // host inputs: addresses, flags, then values (under the address commitment)
  // ---- SoA extraction / padding into the resident workspace (src/twist.rs:115-148)
  Timer t_h2d;
  ProveWs &w = c->prove;
  // V: a resident full slice is used in place (nothing below writes it); host input or a
  // padded slice goes through the workspace
  const bool v_in_place = kind == hipMemcpyDeviceToDevice && n_ops == L;
  Fr *A = (Fr *)w.eval[0].ensure(sizeof(Fr) * L), *O = nullptr;
  Fr *V = v_in_place ? (Fr *)const_cast<uint64_t *>(value) : (Fr *)w.eval[1].ensure(sizeof(Fr) * L);
  const uint64_t *ar = addr;
  const uint8_t *fl = is_write;
  // host inputs go through HostUpload (upload.cpp) on the copy stream, in the order the proof
  // needs them: the addresses (the first commitment starts on them), the flags, then the values
  // (32 B an op, 4x the addresses), whose copy runs under the address commitment -- the value MSM
  // is `late` in commit_evals_pair and waits for it
  const bool v_late = kind == hipMemcpyHostToDevice && n_ops > 0;
  int up_a = -1, up_f = -1, up_v = -1;
  // the values arrive in v_chunks node ranges, each committed as it lands (tns_ctx_set_upload_chunks,
  // default 4; 1 = one upload, one MSM after it); padded slices (L > n_ops) keep one MSM
  const std::vector<size_t> v_off =
      upload_chunk_offsets(n_ops, v_late && L == n_ops && n_ops >= ((size_t)1 << 18) ? c->upload_chunks : 1);
  const int v_chunks = std::max(1, (int)v_off.size() - 1);  // ranges actually formed
  uint32_t *dar32 = nullptr;
  // the op-type table is read by the sum-check only: its first fold pass reads the flag bytes
  // themselves (sumcheck_folds_take_flag_bytes), else it is written on the side stream
  unsigned lr = 0;
  while ((1 << lr) < m.size) lr++;
  const bool flag_bytes = sumcheck_folds_take_flag_bytes(nv - lr);
  if (kind == hipMemcpyHostToDevice) {
    uint64_t *dar = (uint64_t *)w.raw.ensure(8 * (n_ops ? n_ops : 1));
    uint8_t *dfl = (uint8_t *)w.flags.ensure(n_ops ? n_ops : 1);
    if (n_ops) {
      // the addresses cross PCIe as u32 when they fit (memory sizes < 2^32: 64 MB fewer at 2^24 ops)
      dar32 = (uint32_t *)w.narrow.ensure(4 * n_ops);
      up_a = upload.add_narrow(dar32, dar, addr, n_ops);
      // flags read by the folds only (after both commitments) go last: their copy then runs under
      // the last value chunk's MSM instead of ahead of the values
      if (!flag_bytes) up_f = upload.add(dfl, is_write, n_ops);
      for (int k = 0; k < v_chunks; k++) {  // item ids up_v, up_v + 1, ...
        const int id = upload.add(V + v_off[k], value + 4 * v_off[k], sizeof(Fr) * (v_off[k + 1] - v_off[k]));
        if (k == 0) up_v = id;
      }
      if (flag_bytes) up_f = upload.add(dfl, is_write, n_ops);
      upload.start();
    }
    ar = dar;
    fl = dfl;
  } else if (n_ops && !v_in_place) {
    TNS_HIP(hipMemcpyAsync(V, value, sizeof(Fr) * n_ops, kind, st));
  }
  if (L > n_ops) fr_fill_zero_dev(c, V + n_ops, L - n_ops);
  if (!flag_bytes) {
    O = (Fr *)w.optype.ensure(sizeof(Fr) * L);
    if (up_f >= 0) upload.wait(up_f, st);
    stream_wait(c->side, st);
    k_write_flags<<<grid_for(L, 256), 256, 0, c->side>>>(fl, O, n_ops, L);
    TNS_LAUNCH_CHECK();
  }
  if (kind == hipMemcpyHostToDevice) TNS_HIP(hipStreamSynchronize(st));
  tm[0] = t_h2d.ms();
  // the address table (Montgomery, for the sum-check and the openings) and its bit length are
  // written on lane 0 as its MSM starts, so the value commitment's lane does not wait for them;
  // the commitment's sort reads the raw u64 addresses (8 bytes a scalar, no canonical copy)
  unsigned *a_bits = (unsigned *)w.bits.ensure(sizeof(unsigned));
  ScalarSource src_a;
  src_a.prep = [=, &upload](hipStream_t s) {
    if (up_a >= 0) {
      upload.wait(up_a, s);
      widen_dev(s, dar32, upload.narrow_width(up_a), n_ops, const_cast<uint64_t *>(ar));
    }
    u64_tables_dev(s, ar, n_ops, L, A, nullptr, a_bits);
  };
  src_a.canon_bits = a_bits;
  src_a.u64 = ar;
  src_a.n_u64 = n_ops;
  // ---- vector_to_polynomial + commit x2 (src/twist.rs:151-163).  The sum-check below
  // reads A and V without overwriting them, so the openings use the same vectors.
  Timer t_int;
  EvalPoly pa, pv;
  pa.N = pv.N = N;
  pa.first = pv.first = first;
  pa.cnt = pv.cnt = L;
  pa.coeffs = m.size == 1 ? (Fr *)w.coeff[0].ensure(sizeof(Fr) * N) : nullptr;
  pv.coeffs = m.size == 1 ? (Fr *)w.coeff[1].ensure(sizeof(Fr) * N) : nullptr;
  pa.y = A;
  pv.y = V;
  tm[1] = t_int.ms();
  Timer t_com;
  G1Affine cm[2];
  ScalarSource src_v;
  if (v_late) {
    src_v.prep = [&upload, up_v, v_chunks](hipStream_t s) {
      for (int k = 0; k < v_chunks; k++) upload.wait(up_v + k, s);
    };
    src_v.late = true;
    if (v_chunks > 1 && m.size == 1) {
      src_v.chunks = v_chunks;
      src_v.chunk_off = v_off;
      src_v.chunk_prep = [&upload, up_v](int k, hipStream_t s) { upload.wait(up_v + k, s); };
    }
  }
  commit_evals_pair(c, srs->s, pa, pv, m, cm, &src_a, v_late ? &src_v : nullptr);
  if (up_v >= 0) upload.wait_all(st);  // everything below on st / side reads the uploaded inputs
  tm[2] = t_com.ms();
  // ---- transcript (src/twist.rs:170-174), sum-check over the addr / value / op-type MLEs +
  // openings (src/twist.rs:177-243)
  Fr *mles[3] = {A, V, O};
  finish_proof(ctx, srs->s, total, cm, "address_commitment", "value_commitment", mles, 3, nv, pa, pv, out, m,
               flag_bytes ? fl : nullptr, n_ops);
}

int tns_twist_prove(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, const uint64_t *addr,
                    const uint64_t *value, const uint8_t *is_write, size_t n_ops, tns_proof *out) {
  return guarded([&]() {
    twist_core(ctx, srs, params, comm_self(), addr, value, is_write, n_ops, n_ops, out, hipMemcpyHostToDevice);
    return TNS_OK;
  });
}

int tns_twist_prove_device(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, const uint64_t *d_addr,
                           const uint64_t *d_value, const uint8_t *d_is_write, size_t n_ops, tns_proof *out) {
  return guarded([&]() {
    twist_core(ctx, srs, params, comm_self(), d_addr, d_value, d_is_write, n_ops, n_ops, out,
               hipMemcpyDeviceToDevice);
    return TNS_OK;
  });
}

int tns_twist_prove_sharded(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, tns_comm *comm,
                            const uint64_t *d_addr, const uint64_t *d_value, const uint8_t *d_is_write,
                            size_t n_local, uint64_t n_total, tns_proof *out) {
  return guarded([&]() {
    if (!comm || !comm->c) throw Error(TNS_ERR_INVALID_PARAMETERS, "null communicator");
    twist_core(ctx, srs, params, *comm->c, d_addr, d_value, d_is_write, n_local, n_total, out,
               hipMemcpyDeviceToDevice);
    return TNS_OK;
  });
}

// Shout::prove (src/shout.rs:97-222) for this rank's slices of the table (T) and the lookup
// index vector (M), sliced like twist_core's trace.
static void shout_core(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, Comm &m, const uint64_t *entries,
                       size_t n_entries, uint64_t n_entries_total, const uint64_t *indices, size_t n_lookups,
                       uint64_t n_lookups_total, tns_proof *out, hipMemcpyKind kind) {
  Timer total;
  CtxScope g(&ctx->c);
  Ctx *c = &ctx->c;
  hipStream_t st = c->stream;
  std::memset(out, 0, sizeof *out);
  if (n_lookups_total > params->max_operations)  // src/shout.rs:98-102
    throw Error(TNS_ERR_INVALID_PARAMETERS, "Too many lookup operations");
  const size_t T = next_pow2(n_entries_total), M = next_pow2(n_lookups_total);  // :105, :116
  const unsigned nv = ilog2_exact(M);
  if (nv > TNS_MAX_ROUNDS) throw Error(TNS_ERR_INVALID_PARAMETERS, "too many lookups");
  check_shard(m, T, "table");
  check_shard(m, M, "lookup");
  const size_t LT = T / m.size, LM = M / m.size, firstT = (size_t)m.rank * LT, firstM = (size_t)m.rank * LM;
  if (n_entries != slice_count(n_entries_total, firstT, LT) || n_lookups != slice_count(n_lookups_total, firstM, LM))
    throw Error(TNS_ERR_INVALID_PARAMETERS, "local table / lookup count does not match this rank's slice");
  double *tm = ctx->timing;
  for (int i = 0; i < 6; i++) tm[i] = 0;
  TNS_HIP(hipStreamSynchronize(c->side));  // a failed earlier proof's folds may still read the tables
  SideDrain drain{c};
  HostUpload upload(c);  // host inputs: lookup indices, then the table (under the index commitment)
  Timer t_h2d;
  ProveWs &w = c->prove;
  Fr *TB = (Fr *)w.eval[0].ensure(sizeof(Fr) * LT), *I = (Fr *)w.eval[1].ensure(sizeof(Fr) * LM);
  if (LT > n_entries) fr_fill_zero_dev(c, TB + n_entries, LT - n_entries);  // the padding (src/shout.rs:105-107)
  const bool t_late = kind == hipMemcpyHostToDevice && n_entries > 0;
  int up_i = -1, up_t = -1;
  const uint64_t *ir = indices;
  uint32_t *dir32 = nullptr;
  if (kind == hipMemcpyHostToDevice) {
    if (n_lookups) {
      uint64_t *dir = (uint64_t *)w.raw.ensure(8 * n_lookups);
      dir32 = (uint32_t *)w.narrow.ensure(4 * n_lookups);  // u32 over PCIe when they fit
      up_i = upload.add_narrow(dir32, dir, indices, n_lookups);
      ir = dir;
    }
    if (t_late) up_t = upload.add(TB, entries, sizeof(Fr) * n_entries);
    upload.start();
  } else if (n_entries) {
    TNS_HIP(hipMemcpyAsync(TB, entries, sizeof(Fr) * n_entries, kind, st));
  }
  // LookupTable::lookup bounds (src/shout.rs:44-50), agreed over the ranks
  unsigned hbad = 0;
  if (n_lookups) {
    if (up_i >= 0) {
      upload.wait(up_i, st);
      widen_dev(st, dir32, upload.narrow_width(up_i), n_lookups, const_cast<uint64_t *>(ir));
    }
    hbad = index_out_of_bounds(st, ir, n_lookups, n_entries_total, (unsigned *)w.flags.ensure(sizeof(unsigned)));
  }
  // (sharded: every rank's verdict travels with the commitments' partial sums and all ranks fail
  // together after that exchange -- the MSMs read the indices as scalars only, so an out-of-range
  // index is harmless until then, and a rank failing alone here would leave its peers waiting)
  if (hbad && m.size == 1) throw Error(TNS_ERR_INVALID_PARAMETERS, "Lookup index out of bounds");
  if (kind == hipMemcpyHostToDevice) TNS_HIP(hipStreamSynchronize(st));
  tm[0] = t_h2d.ms();
  // the index table is written on lane 1 as the index commitment starts (see twist_core)
  unsigned *i_bits = (unsigned *)w.bits.ensure(sizeof(unsigned));
  ScalarSource src_i;
  src_i.prep = [=](hipStream_t s) { u64_tables_dev(s, ir, n_lookups, LM, I, nullptr, i_bits); };
  src_i.canon_bits = i_bits;
  src_i.u64 = ir;
  src_i.n_u64 = n_lookups;
  Timer t_int;
  EvalPoly pt, pi;
  pt.N = T;
  pi.N = M;
  pt.first = firstT;
  pi.first = firstM;
  pt.cnt = LT;
  pi.cnt = LM;
  pt.coeffs = m.size == 1 ? (Fr *)w.coeff[0].ensure(sizeof(Fr) * T) : nullptr;
  pi.coeffs = m.size == 1 ? (Fr *)w.coeff[1].ensure(sizeof(Fr) * M) : nullptr;
  pt.y = TB;
  pi.y = I;  // the sum-check leaves its input tables intact (zero_folds.hip)
  tm[1] = t_int.ms();
  Timer t_com;
  G1Affine cm[2];
  ScalarSource src_t;
  if (t_late) {
    src_t.prep = [&upload, up_t](hipStream_t s) { upload.wait(up_t, s); };
    src_t.late = true;
  }
  ExtraPayload bad_x;
  bad_x.data = &hbad;
  bad_x.bytes = sizeof hbad;
  commit_evals_pair(c, srs->s, pt, pi, m, cm, t_late ? &src_t : nullptr, &src_i,
                    m.size > 1 ? &bad_x : nullptr);  // (src/shout.rs:125-133)
  if (up_t >= 0) upload.wait_all(st);
  if (m.size > 1) {  // LookupTable::lookup bounds (src/shout.rs:44-50), agreed over the ranks
    for (int r = 0; r < m.size; r++) {
      unsigned f;
      std::memcpy(&f, bad_x.all.data() + sizeof f * (size_t)r, sizeof f);
      hbad |= f;
    }
    if (hbad) throw Error(TNS_ERR_INVALID_PARAMETERS, "Lookup index out of bounds");
  }
  tm[2] = t_com.ms();
  Fr *mles[1] = {I};  // the closure evaluates only the index MLE (src/shout.rs:175)
  finish_proof(ctx, srs->s, total, cm, "table_commitment", "index_commitment", mles, 1, nv, pt, pi, out, m);
}

int tns_shout_prove(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, const uint64_t *entries,
                    size_t n_entries, const uint64_t *indices, size_t n_lookups, tns_proof *out) {
  return guarded([&]() {
    shout_core(ctx, srs, params, comm_self(), entries, n_entries, n_entries, indices, n_lookups, n_lookups, out,
               hipMemcpyHostToDevice);
    return TNS_OK;
  });
}

int tns_shout_prove_device(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, const uint64_t *d_entries,
                           size_t n_entries, const uint64_t *d_indices, size_t n_lookups, tns_proof *out) {
  return guarded([&]() {
    shout_core(ctx, srs, params, comm_self(), d_entries, n_entries, n_entries, d_indices, n_lookups, n_lookups,
               out, hipMemcpyDeviceToDevice);
    return TNS_OK;
  });
}

int tns_shout_prove_sharded(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, tns_comm *comm,
                            const uint64_t *d_entries, size_t n_entries_local, uint64_t n_entries_total,
                            const uint64_t *d_indices, size_t n_lookups_local, uint64_t n_lookups_total,
                            tns_proof *out) {
  return guarded([&]() {
    if (!comm || !comm->c) throw Error(TNS_ERR_INVALID_PARAMETERS, "null communicator");
    shout_core(ctx, srs, params, *comm->c, d_entries, n_entries_local, n_entries_total, d_indices, n_lookups_local,
               n_lookups_total, out, hipMemcpyDeviceToDevice);
    return TNS_OK;
  });
}

}  // extern "C"
