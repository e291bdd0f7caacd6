// kzg.hip -- the KZG commit / open routes behind the C ABI: device-resident coefficients, and the
// evaluation vectors of Twist/Shout::prove (Lagrange basis or interpolated coefficients), singly
// and as the pair of a proof.
#include "abi.hpp"

namespace tns {

// KZGCommitment::commit on device-resident coefficients (src/commitments.rs:162-180)
G1Affine commit_dev(Ctx *c, const Srs &srs, const Fr *coeffs, size_t n) {
  if (n > srs.n) throw Error(TNS_ERR_COMMITMENT, "Polynomial degree exceeds setup size");
  if (srs.first != 0 || srs.held < n)
    throw Error(TNS_ERR_INVALID_PARAMETERS, "coefficient commitments need the whole SRS (this is a shard)");
  return xyzz_to_affine(msm_dev(c, srs.points.as<G1Affine>(), coeffs, n, srs_fixed_base(c, srs, n)));
}

// KZGCommitment::open on device-resident coefficients (src/commitments.rs:182-199)
void open_dev(Ctx *c, const Srs &srs, const Fr *coeffs, size_t n, const Fr &z, Fr *value, G1Affine *proof,
              DevBuf &sbuf) {
  if (n == 0) {
    *value = Fr::zero();
    proof->x = Fq::zero();
    proof->y = Fq::zero();
    return;
  }
  Fr *s = (Fr *)sbuf.ensure(sizeof(Fr) * n);
  *value = synthetic_division_dev(c, coeffs, n, z, s);
  // quotient q_i = s_{i+1}, length n - 1 (empty for n == 1 -> identity)
  *proof = commit_dev(c, srs, s + 1, n - 1);
}

G1Affine commit_evals(Ctx *c, const Srs &srs, EvalPoly &p, Comm &m) {
  if (p.N > srs.n) throw Error(TNS_ERR_COMMITMENT, "Polynomial degree exceeds setup size");
  p.basis = lagrange_basis_dev(c, srs, p.N, p.first, p.cnt);
  if (p.basis) {
    const G1Xyzz part = msm_dev(c, p.basis->points.as<G1Affine>(), p.y, p.cnt, p.basis->fb.get());
    return xyzz_to_affine(allgather_sum_g1(c, m, part, "commitment partial MSM"));
  }
  if (m.size > 1) throw Error(TNS_ERR_INVALID_PARAMETERS, "sharded proving needs an SRS with tau (Lagrange basis)");
  if (p.N & (p.N - 1))
    throw Error(TNS_ERR_POLYNOMIAL, "interpolation of a non-power-of-two vector needs an SRS with tau (Lagrange basis)");
  interpolate_consecutive_dev(c, p.y, p.N, p.coeffs);
  p.have_coeffs = true;
  return commit_dev(c, srs, p.coeffs, p.N);
}

void open_evals(Ctx *c, const Srs &srs, EvalPoly &p, const Fr &z, Fr *value, G1Affine *proof, DevBuf &sbuf,
                Comm &m) {
  if (p.basis && m.size == 1 && fr_is_node(z, p.N)) {  // z = j0 is a node: value y_j0, derivative term
    const size_t j0 = (size_t)from_mont(z).v[0];
    Fr *q = (Fr *)sbuf.ensure(sizeof(Fr) * p.N);
    TNS_HIP(hipMemcpyAsync(value, p.y + j0, sizeof(Fr), hipMemcpyDeviceToHost, c->stream));
    lagrange_node_quotient_dev(c, p.y, p.N, j0, q);  // synchronises
    *proof = xyzz_to_affine(msm_dev(c, p.basis->points.as<G1Affine>(), q, p.N, p.basis->fb.get()));
    return;
  }
  if (p.basis && !fr_is_node(z, p.N)) {
    Fr *q = (Fr *)sbuf.ensure(sizeof(Fr) * p.cnt);
    Fr part[2];
    lagrange_open_partial_dev(c, p.y, p.N, p.first, p.cnt, z, q, &part[0], &part[1]);
    Fr ell = Fr::one(), S = Fr::zero();
    if (m.size == 1) {
      ell = part[0];
      S = part[1];
    } else {
      const std::vector<Fr> all = allgather_fr(c, m, part, 2, "barycentric partials");
      for (int r = 0; r < m.size; r++) {
        ell = mul(ell, all[2 * r]);
        S = add(S, all[2 * r + 1]);
      }
    }
    *value = mul(ell, S);  // P(z) = ell(z) sum_j w_j y_j / (z - j)
    lagrange_quotient_finish_dev(c, p.y, p.cnt, *value, q);
    const G1Xyzz pp = msm_dev(c, p.basis->points.as<G1Affine>(), q, p.cnt, p.basis->fb.get());
    *proof = xyzz_to_affine(allgather_sum_g1(c, m, pp, "opening partial MSM"));
    return;
  }
  if (m.size > 1)  // z on a node: probability ~2^-230; the coefficient route is unsharded
    throw Error(TNS_ERR_PROOF_GENERATION, "opening challenge is an interpolation node (sharded prover)");
  if (!p.have_coeffs) {  // no basis: coefficient form
    if (p.N & (p.N - 1))
      throw Error(TNS_ERR_POLYNOMIAL, "interpolation of a non-power-of-two vector needs an SRS with tau (Lagrange basis)");
    interpolate_consecutive_dev(c, p.y, p.N, p.coeffs);
    p.have_coeffs = true;
  }
  open_dev(c, srs, p.coeffs, p.N, z, value, proof, sbuf);
}

// Both vectors of a proof at once (the two commitments; the two openings at the same z):
// their MSMs overlap on the context's two lanes and each exchange step carries both.
static G1Xyzz sum_rank_parts(const G1Xyzz *all, int size, int stride, int k) {
  G1Xyzz acc = G1Xyzz::inf();
  for (int r = 0; r < size; r++) acc = xyzz_add(acc, all[(size_t)r * stride + k]);
  return acc;
}

static void allgather_sum_g1_pair(Ctx *c, Comm &m, const G1Xyzz part[2], G1Affine out[2], const char *what,
                                  ExtraPayload *extra = nullptr) {
  const size_t xb = extra ? extra->bytes : 0;
  if (m.size == 1) {
    xyzz_to_affine2(part[0], part[1], out[0], out[1]);
    if (xb) extra->all.assign((const uint8_t *)extra->data, (const uint8_t *)extra->data + xb);
    return;
  }
  // one message per rank: [partial 0 | partial 1 | extra], G1Xyzz-aligned
  const size_t rec = 2 * sizeof(G1Xyzz) + (xb + sizeof(G1Xyzz) - 1) / sizeof(G1Xyzz) * sizeof(G1Xyzz);
  const size_t recw = rec / sizeof(G1Xyzz);
  std::vector<G1Xyzz> mine(recw), all(recw * (size_t)m.size);
  mine[0] = part[0];
  mine[1] = part[1];
  if (xb) std::memcpy(&mine[2], extra->data, xb);
  m.exchange(c, mine.data(), rec, all.data(), what);
  xyzz_to_affine2(sum_rank_parts(all.data(), m.size, (int)recw, 0), sum_rank_parts(all.data(), m.size, (int)recw, 1),
                  out[0], out[1]);
  if (xb) {
    extra->all.resize(xb * (size_t)m.size);
    for (int r = 0; r < m.size; r++)
      std::memcpy(extra->all.data() + xb * (size_t)r, &all[recw * (size_t)r + 2], xb);
  }
}

// src0 / src1 (optional): how p0.y / p1.y get written (on the MSM lane that reads them)
// extra (optional, sharded): data exchanged with the commitments' partial sums
void commit_evals_pair(Ctx *c, const Srs &srs, EvalPoly &p0, EvalPoly &p1, Comm &m, G1Affine out[2],
                       const ScalarSource *src0, const ScalarSource *src1, ExtraPayload *extra) {
  if (p0.N > srs.n || p1.N > srs.n) throw Error(TNS_ERR_COMMITMENT, "Polynomial degree exceeds setup size");
  p0.basis = lagrange_basis_dev(c, srs, p0.N, p0.first, p0.cnt);
  p1.basis = lagrange_basis_dev(c, srs, p1.N, p1.first, p1.cnt);
  if (!p0.basis || !p1.basis) {
    for (const ScalarSource *s : {src0, src1})
      if (s && s->prep) s->prep(c->stream);
    if (extra && extra->bytes && m.size > 1)  // (the coefficient route is unsharded: never taken here)
      throw Error(TNS_ERR_PROOF_GENERATION, "sharded commitment without a Lagrange basis");
    if (extra) extra->all.assign((const uint8_t *)extra->data, (const uint8_t *)extra->data + extra->bytes);
    out[0] = commit_evals(c, srs, p0, m);
    out[1] = commit_evals(c, srs, p1, m);
    return;
  }
  auto args = [](const EvalPoly &p, const ScalarSource *s) {
    MsmArgs a{p.basis->points.as<G1Affine>(), p.y, p.cnt, p.basis->fb.get()};
    if (s) a.src = *s;
    return a;
  };
  G1Xyzz part[2];
  msm_pair_dev(c, args(p0, src0), args(p1, src1), part);
  allgather_sum_g1_pair(c, m, part, out, "commitment pair partial MSMs", extra);
}

// extra (optional): exchanged with the openings' partial sums once extra_ready() has run (the
// sharded sum-check's folded table values, which the side stream computes under the openings)
// side_work (optional): host work to queue once the barycentric pass is on the device (it runs
// before the pass's first host wait instead of in front of its launches)
void open_evals_pair(Ctx *c, const Srs &srs, EvalPoly &p0, EvalPoly &p1, const Fr &z, Fr value[2], G1Affine proof[2],
                     DevBuf &sbuf0, DevBuf &sbuf1, Comm &m, ExtraPayload *extra,
                     const std::function<void()> &extra_ready, const std::function<void()> &side_work) {
  const bool same_nodes = p0.N == p1.N && p0.first == p1.first && p0.cnt == p1.cnt;
  const bool pair_pass = p0.basis && p1.basis && !fr_is_node(z, p0.N) && !fr_is_node(z, p1.N) && same_nodes;
  if (side_work && !pair_pass) side_work();
  if (!p0.basis || !p1.basis || fr_is_node(z, p0.N) || fr_is_node(z, p1.N)) {
    open_evals(c, srs, p0, z, &value[0], &proof[0], sbuf0, m);
    open_evals(c, srs, p1, z, &value[1], &proof[1], sbuf0, m);
    if (extra) {  // (unsharded here: open_evals refuses a node z with several ranks)
      if (extra_ready) extra_ready();
      extra->all.assign((const uint8_t *)extra->data, (const uint8_t *)extra->data + extra->bytes);
    }
    return;
  }
  Fr *q0 = (Fr *)sbuf0.ensure(sizeof(Fr) * p0.cnt), *q1 = (Fr *)sbuf1.ensure(sizeof(Fr) * p1.cnt);
  Fr part[4];
  // the shared-inverse pass hands the MSMs canonical quotients and their bit lengths; its
  // inverses come out canonical too, so the quotient kernel needs no reduction pass
  // (0.540 -> 0.504 ms at C4, profiles/r04_c4_step_timeline_canon_inv.txt)
  const bool canon_q = same_nodes && p0.cnt > 64, canon_inv = canon_q;
  if (same_nodes) {  // Twist: one batch inversion for both vectors (inverses land in q1)
    Fr p3[3];
    lagrange_open_partial2_dev(c, p0.y, p1.y, p0.N, p0.first, p0.cnt, z, q1, p3, canon_inv, side_work);
    part[0] = part[2] = p3[0];
    part[1] = p3[1];
    part[3] = p3[2];
  } else {
    lagrange_open_partial_dev(c, p0.y, p0.N, p0.first, p0.cnt, z, q0, &part[0], &part[1]);
    lagrange_open_partial_dev(c, p1.y, p1.N, p1.first, p1.cnt, z, q1, &part[2], &part[3]);
  }
  Fr ell[2] = {Fr::one(), Fr::one()}, S[2] = {Fr::zero(), Fr::zero()};
  const std::vector<Fr> all = allgather_fr(c, m, part, 4, "barycentric pair partials");
  for (int r = 0; r < m.size; r++)
    for (int k = 0; k < 2; k++) {
      ell[k] = mul(ell[k], all[4 * (size_t)r + 2 * k]);
      S[k] = add(S[k], all[4 * (size_t)r + 2 * k + 1]);
    }
  for (int k = 0; k < 2; k++) value[k] = mul(ell[k], S[k]);  // P(z) = ell(z) sum_j w_j y_j / (z - j)
  unsigned *qbits = canon_q ? (unsigned *)c->qbits.ensure(2 * sizeof(unsigned)) : nullptr;
  // the shared-table plan both opening MSMs will take (full-width quotients): the quotient kernel
  // also counts pass 1 of both bucket sorts (their count kernels and one read of q0 / q1 go)
  const FixedBase *f0 = p0.basis->fb.get(), *f1 = p1.basis->fb.get();
  const uint32_t *pre[2] = {nullptr, nullptr};
  bool fused = false;
  WindowPlan full;
  if (same_nodes && canon_inv && c->msm_tables && f0 && f1 && f0->c == f1->c && f0->W == f1->W) {
    full = WindowPlan{f0->c, f0->W, true, f0->c - 1, 0u};  // (the counts do not depend on the table's stride)
    fused = quotient2_count_dev(c, p0.y, p1.y, p0.cnt, value[0], value[1], q1, q0, q1, qbits, full, pre);
  }
  if (fused) {
  } else if (same_nodes) {
    lagrange_quotient_finish2_dev(c, p0.y, p1.y, p0.cnt, value[0], value[1], q1, q0, q1, qbits, canon_inv);
  } else {
    lagrange_quotient_finish_dev(c, p0.y, p0.cnt, value[0], q0);
    lagrange_quotient_finish_dev(c, p1.y, p1.cnt, value[1], q1);
  }
  G1Xyzz pp[2];
  MsmArgs a0{p0.basis->points.as<G1Affine>(), q0, p0.cnt, p0.basis->fb.get()};
  MsmArgs a1{p1.basis->points.as<G1Affine>(), q1, p1.cnt, p1.basis->fb.get()};
  a0.src.canon_bits = qbits;
  a1.src.canon_bits = qbits ? qbits + 1 : nullptr;
  if (fused) {  // (lane 0 sorts a0, lane 1 a1: neither is late)
    a0.precounted = pre[0];
    a1.precounted = pre[1];
    a0.pre = a1.pre = full;
    a0.plan_bits = a1.plan_bits = 254;  // (the counts assumed the full-width table plan)
  }
  msm_pair_dev(c, a0, a1, pp);
  if (extra && extra_ready) extra_ready();
  allgather_sum_g1_pair(c, m, pp, proof, extra ? "opening pair partial MSMs + folded table values" : "opening pair partial MSMs",
                        extra);
}

}  // namespace tns
