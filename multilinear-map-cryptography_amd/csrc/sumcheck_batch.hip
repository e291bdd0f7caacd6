// sumcheck_batch.hip -- a batch of generic sum-checks of one shape in one call.
//
// SumCheck::prove (src/sumcheck.rs:56-110) for `batch` independent instances that share one
// composition over K <= 4 tables of 2^nv entries, each instance on its own transcript.  The single
// prover (sumcheck.hip) is built for one huge instance: round kernels queued behind device-side
// waits, a persistent tail that polls host memory, the last rounds on the host.  For a small
// instance that is a chain of host <-> device turns with the chip idle between them.  Here a
// group of instances advances in lockstep, nv + 1 launches a group whatever the batch:
//   round    one launch over every (instance, pair): fold by the instance's own previous challenge
//            d_chal[b] into ping-pong scratch packed per instance, evaluate the shared composition
//            at X = 0, 2, 3 (and 1 in round 0) in the lazy domain, and reduce the sums per
//            instance into d_sums[b][4] (canonical) -- a segmented reduction in three regimes, see
//            k_scb_round;
//   host     the group's sums in one copy; per instance exactly the single prover's turn
//            (interpolate, check g(0) + g(1), append, draw the challenge, form the next claim);
//            the group's challenges back in one copy;
//   final    a fold-only launch leaves every table's bound value per instance; the host evaluates
//            the composition and checks it against the last claim.
// Nothing on the device waits for the host: a round is launched once its challenges are on the
// device (stream order), and the error path is a stream synchronise.  Every instance's rounds,
// final evaluation, challenges and transcript are byte for byte the single prover's: field sums
// are exact, so neither the order of the additions nor who forms them changes a byte.
// sumcheck_batch_plan.hpp decides the route; on the rows route the single prover runs row by row.
#include "abi.hpp"
#include "sc_poly.hpp"
#include "sumcheck_batch_plan.hpp"

namespace tns {

constexpr unsigned SCB_BLOCK_LOG = 8, SCB_BLOCK = 1u << SCB_BLOCK_LOG;  // 256 threads: four waves

// slot x of d_sums[b][4] <- point X = x; the rounds after the first carry X = 0, 2, 3 only (the
// host takes g(1) as claim - g(0), src/sumcheck.rs:80-84) and leave slot 1 zero
template <bool FIRST>
__device__ __forceinline__ void scb_store_sums(Fr *__restrict__ d_sums, uint64_t b, const Fr (&a)[FIRST ? 4 : 3]) {
  Fr *o = d_sums + 4 * b;
  if (FIRST) {
#pragma unroll
    for (int x = 0; x < 4; x++) o[x] = a[x];
  } else {
    o[0] = a[0];
    o[1] = Fr::zero();
    o[2] = a[1];
    o[3] = a[2];
  }
}

// One sum-check round of every instance of a group.  P = 2^logP pairs an instance, `total` =
// instances x P pairs in all, pair e = b P + s of instance b at flat index e in every packed table.
// FIRST (round 0): tables in[] hold 2P entries an instance, just sum, all four points.
// Else: in[] holds 4P entries an instance; bind d_chal[b] into out[] (2P an instance), then sum the
// round values at X = 0, 2, 3.
// P is a power of two, so either a block holds whole instances or an instance holds whole blocks:
//   P <= 64         an instance is part of a wave: shuffles limited to its P lanes;
//   64 < P <= 256   an instance is one to four waves of one block: wave sums through LDS;
//   P > 256         an instance is 2^(logP - 8 - log_ipt) blocks, each thread taking 2^log_ipt pairs
//                   256 apart: per-block partials, and the last block of the instance to finish
//                   (counters[b]) adds them up and leaves counters[b] zero for the next round.
// A partly filled last block (instances x P no multiple of 256, first two regimes) reads pair 0
// instead of reading past the batch and adds zero; whole segments are live or not (P divides total).
template <int K, bool FIRST>
__global__ void __launch_bounds__(SCB_BLOCK)
    k_scb_round(ScTables t, const ScPoly *__restrict__ qp, unsigned logP, unsigned log_ipt, uint64_t total,
                const Fr *__restrict__ d_chal, Fr *__restrict__ d_sums, Fr *__restrict__ partials,
                unsigned *__restrict__ counters) {
  constexpr int NS = FIRST ? 4 : 3;
  __shared__ Fr lds[4 * 16];
  __shared__ int last;
  const ScPoly &q = *qp;  // device memory, uniform: scalar loads
  const unsigned tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint64_t e0 = ((uint64_t)blockIdx.x << (SCB_BLOCK_LOG + log_ipt)) + tid;
  const bool live0 = e0 < total;
  const uint64_t b = (live0 ? e0 : 0) >> logP;
  Fr r = Fr::zero();
  if (!FIRST) r = d_chal[b];
  Fr acc0 = Fr::zero(), acc1 = Fr::zero(), acc2 = Fr::zero(), acc3 = Fr::zero();
  for (unsigned j = 0; j < (1u << log_ipt); j++) {  // (uniform trip count; log_ipt > 0 only when P > 256)
    const uint64_t e = e0 + ((uint64_t)j << SCB_BLOCK_LOG);
    const bool live = e < total;
    const uint64_t el = live ? e : 0;
    Fr v[K], d[K];
#pragma unroll
    for (int i = 0; i < K; i++) {
      if (!FIRST) {  // (lazy folds: the next round and k_scb_final read [0, 2M] values)
        const Fr *p = t.in[i] + 4 * el;
        const Fr x0 = p[0], x1 = p[1], x2 = p[2], x3 = p[3];
        v[i] = add2_dev(x0, mul_lazy_dev(r, sub2_dev(x1, x0)));
        d[i] = add2_dev(x2, mul_lazy_dev(r, sub2_dev(x3, x2)));
        if (live) {
          t.out[i][2 * e] = v[i];
          t.out[i][2 * e + 1] = d[i];
        }
      } else {
        const Fr *p = t.in[i] + 2 * el;
        v[i] = p[0];
        d[i] = p[1];
      }
      d[i] = sub2_dev(d[i], v[i]);
    }
    const Fr zero = Fr::zero();
#pragma unroll 1
    for (int x = 0; x < 4; x++) {
      if (!(!FIRST && x == 1)) {
        const Fr ev = sc_eval<K>(q, v);
        const Fr ez = live ? ev : zero;
        if (x == 0) acc0 = add2_dev(acc0, ez);
        else if (x == 1) acc1 = add2_dev(acc1, ez);
        else if (x == 2) acc2 = add2_dev(acc2, ez);
        else acc3 = add2_dev(acc3, ez);
      }
      if (x < 3) {
#pragma unroll
        for (int i = 0; i < K; i++) v[i] = add2_dev(v[i], d[i]);
      }
    }
  }
  Fr a[NS];
  a[0] = sc_canon(acc0);
  if (FIRST) {
    a[1] = sc_canon(acc1);
    a[2] = sc_canon(acc2);
    a[3] = sc_canon(acc3);
  } else {
    a[1] = sc_canon(acc2);
    a[2] = sc_canon(acc3);
  }
  if (logP <= 6) {  // an instance is 2^logP lanes of this wave
    const unsigned P = 1u << logP;
#pragma unroll
    for (unsigned dd = 32; dd > 0; dd >>= 1) {
      if (dd < P) {  // (uniform; the segment's first lane only ever adds lanes of its own segment)
#pragma unroll
        for (int x = 0; x < NS; x++) {
          const Fr o = shfl_down_fr(a[x], dd);
          if (lane + dd < 64) a[x] = add(a[x], o);
        }
      }
    }
    if (live0 && (lane & (P - 1)) == 0) scb_store_sums<FIRST>(d_sums, b, a);
    return;
  }
  if (logP <= SCB_BLOCK_LOG) {  // an instance is 2 or 4 waves of this block
    const unsigned P = 1u << logP, waves = P >> 6;
#pragma unroll
    for (unsigned dd = 32; dd > 0; dd >>= 1) {
#pragma unroll
      for (int x = 0; x < NS; x++) {
        const Fr o = shfl_down_fr(a[x], dd);
        if (lane + dd < 64) a[x] = add(a[x], o);
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int x = 0; x < NS; x++) lds[x * 16 + wid] = a[x];
    }
    __syncthreads();
    if (live0 && (tid & (P - 1)) == 0) {
#pragma unroll
      for (int x = 0; x < NS; x++) {
        Fr s = lds[x * 16 + wid];
        for (unsigned w = 1; w < waves; w++) s = add(s, lds[x * 16 + wid + w]);
        a[x] = s;
      }
      scb_store_sums<FIRST>(d_sums, b, a);
    }
    return;
  }
  // an instance is nblk whole blocks (every block full: 256 2^log_ipt divides P)
  const unsigned log_nblk = logP - SCB_BLOCK_LOG - log_ipt, nblk = 1u << log_nblk;
  block_sum_fr<NS>(a, lds);
  if (tid == 0) {
#pragma unroll
    for (int x = 0; x < NS; x++) partials[4 * (size_t)blockIdx.x + x] = a[x];
    __threadfence();
    last = atomicAdd(&counters[b], 1u) == nblk - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();  // every block's partials (each fenced before its increment) are visible
  const Fr *mine = partials + 4 * ((size_t)(blockIdx.x >> log_nblk) << log_nblk);
#pragma unroll
  for (int x = 0; x < NS; x++) a[x] = Fr::zero();
  for (unsigned bb = tid; bb < nblk; bb += SCB_BLOCK)
#pragma unroll
    for (int x = 0; x < NS; x++) a[x] = add(a[x], mine[4 * (size_t)bb + x]);
  block_sum_fr<NS>(a, lds);
  if (tid == 0) {
    scb_store_sums<FIRST>(d_sums, b, a);
    counters[b] = 0;  // ready for the next round (stream order)
  }
}

// The last variable: d_finals[b k + m] = table m of instance b bound at d_chal[b], canonical; in[]
// holds the last round's 2 entries an instance (nv == 1: the caller's tables)
__global__ void __launch_bounds__(SCB_BLOCK) k_scb_final(ScTables t, int k, uint64_t count, const Fr *__restrict__ d_chal,
                                                         Fr *__restrict__ d_finals) {
  const uint64_t e = (uint64_t)blockIdx.x * SCB_BLOCK + threadIdx.x;
  if (e >= count) return;
  const uint64_t b = e / (unsigned)k;
  const int m = (int)(e - b * (unsigned)k);
  const Fr *p = (m == 0 ? t.in[0] : m == 1 ? t.in[1] : m == 2 ? t.in[2] : t.in[3]) + 2 * b;
  const Fr p0 = sc_canon(p[0]), p1 = sc_canon(p[1]);  // (lazy round-kernel folds)
  d_finals[e] = add(p0, mul(d_chal[b], sub(p1, p0)));
}

namespace {

// pairs a thread of the cross-block regime takes: as many (up to 8) as leave the launch at least
// 1024 blocks, and an instance at least one
unsigned scb_log_ipt(unsigned logP, uint64_t total) {
  unsigned l = 0;
  while (l < 3 && logP > SCB_BLOCK_LOG + l && (total >> (SCB_BLOCK_LOG + l + 1)) >= 1024) l++;
  return l;
}

template <bool FIRST>
void scb_launch_round(hipStream_t st, int k, const ScTables &tt, const ScPoly *q_dev, unsigned logP, uint64_t total,
                      const Fr *d_chal, Fr *d_sums, Fr *partials, unsigned *counters) {
  const unsigned log_ipt = logP > SCB_BLOCK_LOG ? scb_log_ipt(logP, total) : 0;
  const uint64_t per = (uint64_t)SCB_BLOCK << log_ipt;
  const unsigned g = (unsigned)((total + per - 1) / per);
  sc_for_tables(k, [&](auto K) {
    k_scb_round<decltype(K)::value, FIRST>
        <<<g, SCB_BLOCK, 0, st>>>(tt, q_dev, logP, log_ipt, total, d_chal, d_sums, partials, counters);
  });
  TNS_LAUNCH_CHECK();
}

struct ScbCall {
  Ctx *c;
  int k;
  unsigned nv;
  const SumcheckTerm *terms;
  int n_terms;
  Fr *const *tables;  // device, batch x 2^nv each, the caller's order
  const Fr *claimed;
  tns_transcript *const *trs;
  Fr *rounds, *chal, *finals;  // host: batch x nv x 4, batch x nv, batch
};

[[noreturn]] void scb_fail_round(size_t inst, unsigned rnd) {
  char lab[96];
  snprintf(lab, sizeof lab, "Instance %zu: Round %u consistency check failed", inst, rnd);
  throw Error(TNS_ERR_SUMCHECK, lab);
}

// instances [g0, g0 + G) in lockstep; returns the launches it queued (nv + 1)
size_t scb_group(const ScbCall &A, const ScPoly *q_dev, const int *perm, size_t g0, size_t G) {
  Ctx *c = A.c;
  hipStream_t st = c->stream;
  const int k = A.k;
  const unsigned nv = A.nv;
  const size_t n = (size_t)1 << nv;
  SumcheckWs &ws = c->sc;
  Fr *ping = (Fr *)ws.batch_fold[0].ensure(sizeof(Fr) * k * G * (n / 2));
  Fr *pong = (Fr *)ws.batch_fold[1].ensure(sizeof(Fr) * k * G * (n / 4));
  // d_chal (G) | d_sums (4 G) | d_finals (k G), then the counters
  Fr *d_chal = (Fr *)ws.batch_state.ensure(sizeof(Fr) * G * (5 + k) + sizeof(unsigned) * G);
  Fr *d_sums = d_chal + G, *d_finals = d_sums + 4 * G;
  unsigned *counters = (unsigned *)(d_finals + (size_t)k * G);
  // (one 4-vector a block of the largest cross-block launch: round 0, one pair a thread)
  Fr *partials = (Fr *)ws.batch_partials.ensure(sizeof(Fr) * 4 * std::max<size_t>(1, (G * (n / 2)) >> SCB_BLOCK_LOG));
  Fr *h_sums = (Fr *)ws.batch_host.ensure(sizeof(Fr) * G * (5 + k));
  Fr *h_chal = h_sums + 4 * G, *h_finals = h_chal + G;
  TNS_HIP(hipMemsetAsync(counters, 0, sizeof(unsigned) * G, st));
  // round rr reads the caller's tables (rr <= 1) or the previous round's output and writes the
  // folded tables into ping (rr odd) / pong (rr even >= 2): the caller's tables stay intact
  auto in_of = [&](unsigned rr, int m) -> const Fr * {
    if (rr <= 1) return A.tables[perm[m]] + g0 * n;
    return rr % 2 == 0 ? ping + (size_t)m * G * (n / 2) : pong + (size_t)m * G * (n / 4);
  };
  auto out_of = [&](unsigned rr, int m) -> Fr * {
    return rr % 2 == 1 ? ping + (size_t)m * G * (n / 2) : pong + (size_t)m * G * (n / 4);
  };
  std::vector<Fr> cur(A.claimed + g0, A.claimed + g0 + G);
  size_t launches = 0;
  for (unsigned rnd = 0; rnd < nv; rnd++) {
    const unsigned logP = nv - 1 - rnd;
    const SumcheckLabels lab(rnd);
    ScTables tt{};
    for (int m = 0; m < k; m++) {
      tt.in[m] = in_of(rnd, m);
      tt.out[m] = rnd ? out_of(rnd, m) : nullptr;
    }
    const uint64_t total = (uint64_t)G << logP;
    if (rnd == 0) scb_launch_round<true>(st, k, tt, q_dev, logP, total, d_chal, d_sums, partials, counters);
    else scb_launch_round<false>(st, k, tt, q_dev, logP, total, d_chal, d_sums, partials, counters);
    launches++;
    TNS_HIP(hipMemcpyAsync(h_sums, d_sums, sizeof(Fr) * 4 * G, hipMemcpyDeviceToHost, st));
    // the round's challenge hash over each state so far, while the device works
    for (size_t b = 0; b < G; b++) sumcheck_prehash(A.trs[g0 + b]->t, lab);
    TNS_HIP(hipStreamSynchronize(st));
    for (size_t b = 0; b < G; b++) {  // the host's turn (sumcheck_host.cpp), per instance
      // Only round 0 can fail the check (later rounds take g(1) from the claim), and the instances
      // are visited in order: the first failure seen is the lowest instance of the earliest round
      Fr coeffs[4];
      if (!sumcheck_round_coeffs(h_sums + 4 * b, cur[b], rnd > 0, coeffs)) scb_fail_round(g0 + b, rnd);
      Fr *rounds = A.rounds + ((g0 + b) * nv + rnd) * 4;
      for (int x = 0; x < 4; x++) rounds[x] = coeffs[x];
      const Fr ch = sumcheck_absorb_round(A.trs[g0 + b]->t, lab, coeffs);
      h_chal[b] = ch;
      A.chal[(g0 + b) * nv + rnd] = ch;
      cur[b] = sumcheck_next_claim(coeffs, ch);
    }
    // (h_chal is rewritten only after the next round's synchronise: the copy has landed by then)
    TNS_HIP(hipMemcpyAsync(d_chal, h_chal, sizeof(Fr) * G, hipMemcpyHostToDevice, st));
  }
  ScTables tt{};
  for (int m = 0; m < k; m++) tt.in[m] = nv <= 1 ? A.tables[perm[m]] + g0 * n : out_of(nv - 1, m);
  const uint64_t count = (uint64_t)G * k;
  k_scb_final<<<(unsigned)((count + SCB_BLOCK - 1) / SCB_BLOCK), SCB_BLOCK, 0, st>>>(tt, k, count, d_chal, d_finals);
  TNS_LAUNCH_CHECK();
  launches++;
  TNS_HIP(hipMemcpyAsync(h_finals, d_finals, sizeof(Fr) * count, hipMemcpyDeviceToHost, st));
  TNS_HIP(hipStreamSynchronize(st));
  for (size_t b = 0; b < G; b++) {
    Fr vals[MAX_SC_TABLES];
    for (int m = 0; m < k; m++) vals[perm[m]] = h_finals[b * k + m];
    const Fr fe = eval_composition_host(vals, A.terms, A.n_terms);  // polynomial(&fixed_variables), :104
    A.finals[g0 + b] = fe;
    // the last round's claim is f(r): the check that catches a device miscompute, kept per instance
    if (fe != cur[b]) {
      char lab[128];
      snprintf(lab, sizeof lab,
               "Instance %zu: final evaluation does not match the last round's claim (device result inconsistent)",
               g0 + b);
      throw Error(TNS_ERR_SUMCHECK, lab);
    }
  }
  return launches;
}

}  // namespace

int sumcheck_prove_batch(tns_ctx *ctx, const uint64_t *const *tables, int n_tables, unsigned nv, size_t batch,
                         const uint64_t *claimed_sums, const tns_term *terms, int n_terms,
                         tns_transcript *const *transcripts, uint64_t *rounds_out, uint64_t *finals_out,
                         uint64_t *challenges_out, bool resident, const ScBatchLimits &lim, ScBatchReport *rep_out) {
  ScBatchReport rep;
  int status = guarded([&]() {
    // ---- the checks, before anything touches a device
    if (!ctx) throw Error(TNS_ERR_INVALID_PARAMETERS, "null context");
    if (batch == 0) return (int)TNS_OK;
    sc_check_shape(nv, n_tables, n_terms);
    sc_check_arrays(claimed_sums && transcripts && finals_out && (nv == 0 || rounds_out) && (n_terms == 0 || terms) &&
                        (n_tables == 0 || tables),
                    tables, n_tables, batch, nv);
    sc_check_transcripts(transcripts, batch);
    ScBatchShape shape;
    const std::vector<SumcheckTerm> st = sc_terms(terms, n_terms, &shape.table_terms);
    sc_check_terms(st.data(), n_terms, n_tables);
    shape.batch = batch;
    shape.nv = nv;
    shape.n_tables = n_tables;
    const ScBatchPlan plan = plan_sumcheck_batch(shape, lim);
    rep.route = plan.route;
    rep.group_rows = plan.group_rows;
    rep.groups = plan.groups;

    const size_t n = (size_t)1 << nv;
    CtxScope scope(&ctx->c);
    Ctx *c = &ctx->c;
    StagedTables staged(c, tables, n_tables, sizeof(Fr) * batch * n, resident);
    Fr *const *tabs = staged.tab;
    std::vector<Fr> rounds(4 * (size_t)nv * batch + 1), chal((size_t)nv * batch + 1), fin(batch), cl(batch);
    std::memcpy((void *)cl.data(), claimed_sums, sizeof(Fr) * batch);

    if (plan.route == BATCH_ROUTE_BATCHED) {
      ScbCall A{c, n_tables, nv, st.data(), n_terms, tabs, cl.data(), transcripts, rounds.data(), chal.data(), fin.data()};
      int perm[MAX_SC_TABLES];
      ScPoly *qh = (ScPoly *)c->sc.poly_host.ensure(sizeof(ScPoly));  // pinned: outlives the async copy
      *qh = sc_poly(st.data(), n_terms, n_tables, perm);
      ScPoly *qd = (ScPoly *)c->sc.poly.ensure(sizeof(ScPoly));
      TNS_HIP(hipMemcpyAsync(qd, qh, sizeof(ScPoly), hipMemcpyHostToDevice, c->stream));
      for (size_t g = 0; g < plan.groups; g++) {
        const size_t g0 = g * plan.group_rows;
        rep.launches += scb_group(A, qd, perm, g0, std::min(plan.group_rows, batch - g0));
      }
    } else {
      for (size_t b = 0; b < batch; b++) {
        Fr *row[MAX_SC_TABLES];
        for (int j = 0; j < n_tables; j++) row[j] = tabs[j] + b * n;
        try {
          sumcheck_prove_dev(c, row, n_tables, nv, cl[b], st.data(), n_terms, transcripts[b]->t,
                             rounds.data() + 4 * (size_t)nv * b, chal.data() + (size_t)nv * b, &fin[b]);
        } catch (const Error &e) {
          if (e.code != TNS_ERR_SUMCHECK) throw;
          throw Error(TNS_ERR_SUMCHECK, "Instance " + std::to_string(b) + ": " + e.what());
        }
      }
    }
    TNS_HIP(hipStreamSynchronize(c->stream));
    std::memcpy(rounds_out, rounds.data(), sizeof(Fr) * 4 * (size_t)nv * batch);
    std::memcpy(finals_out, fin.data(), sizeof(Fr) * batch);
    if (challenges_out) std::memcpy(challenges_out, chal.data(), sizeof(Fr) * (size_t)nv * batch);
    return (int)TNS_OK;
  });
  if (rep_out) *rep_out = rep;
  return status;
}

}  // namespace tns

using namespace tns;

extern "C" {

int tns_sumcheck_prove_batch(tns_ctx *ctx, const uint64_t *const *tables, int n_tables, unsigned nv, size_t batch,
                             const uint64_t *claimed_sums, const tns_term *terms, int n_terms,
                             tns_transcript *const *transcripts, uint64_t *rounds_out, uint64_t *finals_out,
                             uint64_t *challenges_out) {
  return sumcheck_prove_batch(ctx, tables, n_tables, nv, batch, claimed_sums, terms, n_terms, transcripts, rounds_out,
                              finals_out, challenges_out, false, ScBatchLimits(), nullptr);
}
int tns_sumcheck_prove_batch_device(tns_ctx *ctx, const uint64_t *const *d_tables, int n_tables, unsigned nv, size_t batch,
                                    const uint64_t *claimed_sums, const tns_term *terms, int n_terms,
                                    tns_transcript *const *transcripts, uint64_t *rounds_out, uint64_t *finals_out,
                                    uint64_t *challenges_out) {
  return sumcheck_prove_batch(ctx, d_tables, n_tables, nv, batch, claimed_sums, terms, n_terms, transcripts, rounds_out,
                              finals_out, challenges_out, true, ScBatchLimits(), nullptr);
}

}  // extern "C"
