// srs.hpp -- the structured reference string and what is derived from it and cached with it (its
// window table, the Lagrange bases of node sets, the all-index opening plans), with the entry
// points of the modules that build or use those: lagrange.hip, tfree.hip, vc_open.hip, srs_io.hip.
#pragma once
#include <functional>
#include <map>
#include <memory>
#include <tuple>

#include "bn254.hpp"
#include "hip_util.hpp"
#include "msm.hpp"

namespace tns {

struct Ctx;

struct LagrangeBasis {
  DevBuf points;                  // G1Affine[N]: G * L_j(tau)
  std::unique_ptr<FixedBase> fb;  // its window table (N >= 2^12)
};

// What tns_vc_open_all keeps per (SRS, n) (vc_open.hip): the correlation A_i = sum_j Lambda_j / (j - i)
// of the Lagrange basis, the spectrum of its kernel, and the vector-independent scalars of f'(i).
struct OpenAllPlan {
  size_t n = 0, M = 0;  // M = next_pow2(2 n - 1): the cyclic length
  DevBuf A;             // G1Affine[n]
  DevBuf spec;          // Fr[M]: fr_ntt of the kernel, scaled by 1 / M (Montgomery, bit-reversed order)
  DevBuf iw, D;         // Fr[n]: 1 / w_i, and (1 / w_i) sum_j w_j / (i - j)
};

struct Srs {
  DevBuf points;  // G1Affine[n]
  size_t n = 0;
  int device = 0;
  // setup_params keeps tau in CommitmentParams (src/utils.rs:94-100); with it the setup
  // also yields the Lagrange basis of the nodes {0..N-1}: G * L_j(tau) (lagrange.hip).
  bool has_tau = false;
  Fr tau;
  // (N, first node, node count) -> basis slice (cache)
  mutable std::map<std::tuple<size_t, size_t, size_t>, std::unique_ptr<LagrangeBasis>> lagrange;
  size_t first = 0, held = 0;  // points[0..held) are g1_powers[first .. first + held) (sharded SRS)
  mutable std::unique_ptr<FixedBase> fb;                              // window table of `points` (lazy)
  mutable std::map<size_t, std::unique_ptr<OpenAllPlan>> open_all;  // n -> tns_vc_open_all's plan (cache)
  Srs() = default;
  Srs(const Srs &) = delete;
  Srs &operator=(const Srs &) = delete;
};

// lagrange.hip: KZG on evaluations over the nodes {0..N-1}, for the node slice
// [first, first + cnt) a rank holds (first = 0, cnt = N unsharded).
// Basis slice G * L_j(tau) (cached in srs); nullptr when srs has no tau or tau is a node.
const LagrangeBasis *lagrange_basis_dev(Ctx *c, const Srs &srs, size_t N, size_t first, size_t cnt);
// inv[i] = 1 / (z - j) (j = first + i); ell_part = prod (z - j); sum_part = sum w_j y_j / (z - j)
// over the slice.  P(z) = (prod of all ell parts) * (sum of all sum parts).  z not a node.
void lagrange_open_partial_dev(Ctx *c, const Fr *y, size_t N, size_t first, size_t cnt, const Fr &z, Fr *inv,
                               Fr *ell_part, Fr *sum_part);
// q_i = (v - y_i) * inv_i in place: the quotient's values on the slice
void lagrange_quotient_finish_dev(Ctx *c, const Fr *y, size_t cnt, const Fr &v, Fr *q);
// canon_inv: inv receives the inverses in canonical form (for the CI quotient kernel)
// queued (optional): run on the host once the pass's first kernels are queued, before its first
// host wait (side-stream work that should not delay the pass)
void lagrange_open_partial2_dev(Ctx *c, const Fr *y0, const Fr *y1, size_t N, size_t first, size_t cnt, const Fr &z,
                                Fr *inv, Fr parts[3], bool canon_inv = false,
                                const std::function<void()> &queued = nullptr);
// bits != nullptr: q0 / q1 come out CANONICAL with their largest bit lengths in bits[0..1];
// canon_inv (requires bits): inv holds canonical inverses (lagrange_open_partial2_dev's canon_inv)
void lagrange_quotient_finish2_dev(Ctx *c, const Fr *y0, const Fr *y1, size_t cnt, const Fr &v0, const Fr &v1,
                                   const Fr *inv, Fr *q0, Fr *q1, unsigned *bits, bool canon_inv = false);
// quotient values for an opening AT the node j0 (value y_j0), unsharded
void lagrange_node_quotient_dev(Ctx *c, const Fr *y, size_t N, size_t j0, Fr *q);
bool fr_is_node(const Fr &x, size_t N);
// the shared inverses of opening many vectors at one z: inv[j] = 1 / (z - j), j < N (0 at j == skip, the
// node z is; SIZE_MAX: none), *ell_dev = prod over the other nodes of (z - j); device outputs, queued
void lagrange_inverses_dev(Ctx *c, size_t N, const Fr &z, size_t skip, Fr *inv, Fr *ell_dev);
// barycentric weights w_j = (-1)^(N-1-j) / (j! (N-1-j)!) of the nodes [first, first + cnt) (cached)
const Fr *bary_weights_dev(Ctx *c, size_t N, size_t first, size_t cnt);
// tfree.hip: the Lagrange basis [L_j(tau)]G, j < N, from g1_powers[0..N) alone (no tau); cached in
// srs.lagrange under (N, 0, N) like the tau-derived one
const LagrangeBasis *lagrange_basis_from_powers_dev(Ctx *c, const Srs &srs, size_t N);
// vc_open.hip: every opening of a KZG vector commitment in one pass (tns_vc_open_all).  proofs_dev:
// n affine points on the device; vec_dev: the n entries (Montgomery), only read.  Throws
// TNS_ERR_INVALID_PARAMETERS when the SRS provides no Lagrange basis of n nodes.
const OpenAllPlan *open_all_plan_dev(Ctx *c, const Srs &srs, size_t n);
void vc_open_all_dev(Ctx *c, const Srs &srs, const Fr *vec_dev, size_t n, G1Affine *proofs_dev);
// whether k openings of a vector of n entries take the all-index pass (tns_vc_open_many's rule)
bool vc_open_many_takes_all(size_t n, size_t k);
// srs_io.hip: Vec<G1Affine> in ark-serialize form (u64 LE count, then 32 / 64 bytes a point),
// decoded, validated and encoded on the device.  g1_vec_header returns the count of a file whose
// length must match it exactly; g1_decode_dev / g1_encode_dev move n points between wire bytes on
// the host and points on the device (a refused point throws, naming the lowest such index).
size_t g1_vec_serialized_size(size_t n, bool compressed);
size_t g1_vec_header(const uint8_t *in, size_t len, bool compressed);
void g1_vec_put_header(size_t n, uint8_t *out);
void g1_decode_dev(Ctx *c, const uint8_t *bytes, size_t n, bool compressed, G1Affine *out);
void g1_encode_dev(Ctx *c, const G1Affine *pts, size_t n, bool compressed, uint8_t *bytes);
// the stored basis [L_j(tau)]G, j < N (wire bytes), checked against g1_powers[0..N) with scalars
// from `seed` (nullptr: from the OS) and then cached in srs.lagrange under (N, 0, N)
void lagrange_basis_attach_dev(Ctx *c, const Srs &srs, const uint8_t *bytes, size_t N, bool compressed,
                               const uint8_t seed[32]);

}  // namespace tns
