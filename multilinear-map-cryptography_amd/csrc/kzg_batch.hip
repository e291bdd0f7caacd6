// kzg_batch.hip -- many vectors over one SRS in one call: `batch` MSMs over the same points, and the
// two KZG operations on evaluation vectors that reduce to them (commit every row; open every row at
// one shared z, a node included).  msm_batch_plan.hpp's plan_batch decides the route from numbers
// alone: the batched pass of msm.hip (groups of rows, each one sort / accumulation / reduction /
// finish kernel) or the single-vector functions in a loop on the one uploaded copy.
//
// Opening B rows y_b at z (lagrange.hip's barycentric form, per row):
//   off a node  f_b(z) = ell(z) sum_j w_j y_bj / (z - j),   q_bj = (f_b(z) - y_bj) / (z - j);
//   at node j0  f_b(z) = y_bj0,  q_bj = (y_bj0 - y_bj) / (j0 - j)  (j != j0),
//               q_bj0 = (1 / w_j0) sum_{j != j0} w_j (y_bj - y_bj0) / (j0 - j).
// The inverses 1 / (z - j) are shared by the rows (lagrange_inverses_dev, once); three kernels whose
// launch count does not depend on B form every row's sum, its value and its quotient scalars.
// With one point per row (open_evals_batch_points: the batched provers' openings, "open vector b at
// index i_b") z, ell(z), the inverses and j0 are per-point quantities: all P n inverses come from
// one batch inversion, and off-node and node points may be mixed in one call.
#include "abi.hpp"

namespace tns {

constexpr int BARY_TILE = 1024;  // nodes a block of 256 threads sums for one row

// coef[j] = w_j inv_j (inv_j = 0 at the punctured node: no term)
__global__ void __launch_bounds__(256) k_batch_coef(const Fr *__restrict__ w, const Fr *__restrict__ inv, size_t n,
                                                    Fr *__restrict__ coef) {
  for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x)
    coef[j] = mul(w[j], inv[j]);
}

// parts[b tiles + t] = sum over node tile t of coef_j (y_bj - yoff_b); yoff_b = y_b,j0 when the rows
// are opened at the node j0 (j0 < n), else 0.  Grid: (tiles, rows-strided y).
__global__ void __launch_bounds__(256) k_batch_bary(const Fr *__restrict__ y, const Fr *__restrict__ coef, size_t n,
                                                    size_t rows, size_t j0, size_t tiles, Fr *__restrict__ parts) {
  __shared__ Fr lds[256];
  const size_t t = blockIdx.x;
  for (size_t b = blockIdx.y; b < rows; b += gridDim.y) {
    const Fr *yb = y + b * n;
    const bool node = j0 < n;
    const Fr yoff = node ? yb[j0] : Fr::zero();
    Fr acc = Fr::zero();
    const size_t a = t * BARY_TILE, e = min(n, a + (size_t)BARY_TILE);
    for (size_t j = a + threadIdx.x; j < e; j += 256) acc = add(acc, mul(coef[j], node ? sub(yb[j], yoff) : yb[j]));
    lds[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) lds[threadIdx.x] = add(lds[threadIdx.x], lds[threadIdx.x + s]);
      __syncthreads();
    }
    if (threadIdx.x == 0) parts[b * tiles + t] = lds[0];
    __syncthreads();
  }
}

// per row: S_b = sum of its parts; off a node value_b = ell S_b; at the node j0 value_b = y_b,j0 and
// dq_b = S_b / w_j0 (the quotient's value at j0)
__global__ void __launch_bounds__(64) k_batch_values(const Fr *__restrict__ parts, size_t tiles, size_t rows,
                                                     const Fr *__restrict__ y, size_t n, size_t j0,
                                                     const Fr *__restrict__ ell, const Fr *__restrict__ w,
                                                     Fr *__restrict__ values, Fr *__restrict__ dq) {
  __shared__ Fr iw;
  const bool node = j0 < n;
  if (node && threadIdx.x == 0) iw = inv(w[j0]);
  __syncthreads();
  const size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (b >= rows) return;
  Fr s = Fr::zero();
  for (size_t t = 0; t < tiles; t++) s = add(s, parts[b * tiles + t]);
  if (node) {
    values[b] = y[b * n + j0];
    dq[b] = mul(s, iw);
  } else {
    values[b] = mul(ell[0], s);
  }
}

// q[b n + j] = (value_b - y_bj) inv_j, and dq_b at the node j0
__global__ void __launch_bounds__(256) k_batch_quotients(const Fr *__restrict__ y, const Fr *__restrict__ inv,
                                                         const Fr *__restrict__ values, const Fr *__restrict__ dq,
                                                         size_t n, size_t rows, size_t j0, Fr *__restrict__ q) {
  const size_t total = rows * n;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t b = e / n, j = e - b * n;
    q[e] = j == j0 ? dq[b] : mul(sub(values[b], y[e]), inv[j]);
  }
}

// ---------------------------------------------------------------- one opening point per row group
// open_evals_batch_points: row r is opened at point p = r / g (g rows share a point: a proof's two
// vectors).  z, ell(z), the inverses and the node index j0 become per-point quantities; the flat
// arrays below are P x n, entry e = p n + j.  j0[p] = the node z_p is (j0[p] < n), else SIZE_MAX.
constexpr int PTS_CH = 4;                  // differences a thread of k_pts_inv inverts
constexpr int PTS_SEG = 256 * PTS_CH;      // ... and a block: one modular inverse per PTS_SEG elements

// ell[p] = prod_j (z_p - j) over the non-zero differences (a block per point: chains of one block
// never leave their point)
__global__ void __launch_bounds__(256) k_pts_ell(const Fr *__restrict__ z, size_t n, size_t P, Fr *__restrict__ ell) {
  __shared__ Fr lds[256];
  const Fr step = from_u64<FrCfg>(256);
  for (size_t p = blockIdx.x; p < P; p += gridDim.x) {
    Fr d = sub(z[p], from_u64<FrCfg>((uint64_t)threadIdx.x));
    Fr acc = Fr::one();
    for (size_t j = threadIdx.x; j < n; j += 256) {
      if (!d.is_zero()) acc = mul(acc, d);
      d = sub(d, step);
    }
    lds[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) lds[threadIdx.x] = mul(lds[threadIdx.x], lds[threadIdx.x + s]);
      __syncthreads();
    }
    if (threadIdx.x == 0) ell[p] = lds[0];
    __syncthreads();
  }
}

// inv[e] = 1 / (z_p - j) and coef[e] = w_j inv[e] for all `total` = P n entries by batch inversion:
// a block inverts a segment of PTS_SEG entries with ONE modular inverse (k_chain_inv's prefix and
// suffix products over the threads' own products of PTS_CH differences).  The zero difference at a
// node counts as one in the products and gets inverse 0.
__global__ void __launch_bounds__(256) k_pts_inv(const Fr *__restrict__ z, const Fr *__restrict__ w, size_t n,
                                                 size_t total, Fr *__restrict__ inv_out, Fr *__restrict__ coef) {
  __shared__ Fr sh[256];
  __shared__ Fr inv_total;
  const int tid = threadIdx.x;
  const size_t nseg = (total + PTS_SEG - 1) / PTS_SEG;
  for (size_t seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
    Fr a[PTS_CH], pre[PTS_CH];
    bool hole[PTS_CH];
    Fr prod = Fr::one();
#pragma unroll
    for (int k = 0; k < PTS_CH; k++) {
      const size_t e = seg * PTS_SEG + (size_t)k * 256 + tid;
      a[k] = Fr::one();
      hole[k] = true;
      if (e < total) {
        const size_t p = e / n, j = e - p * n;
        const Fr d = sub(z[p], from_u64<FrCfg>((uint64_t)j));
        hole[k] = d.is_zero();
        if (!hole[k]) a[k] = d;
      }
      pre[k] = prod;
      prod = mul(prod, a[k]);
    }
    Fr lo = prod, hi = prod;  // inclusive prefix / suffix products over the block
    for (int off = 1; off < 256; off <<= 1) {
      sh[tid] = lo;
      __syncthreads();
      const Fr o = tid >= off ? sh[tid - off] : Fr::one();
      __syncthreads();
      lo = mul(o, lo);
    }
    for (int off = 1; off < 256; off <<= 1) {
      sh[tid] = hi;
      __syncthreads();
      const Fr o = tid + off < 256 ? sh[tid + off] : Fr::one();
      __syncthreads();
      hi = mul(hi, o);
    }
    if (tid == 0) inv_total = inv_binary_dev(hi);  // (never zero: holes count as one)
    sh[tid] = lo;
    __syncthreads();
    const Fr before = tid ? sh[tid - 1] : Fr::one();
    __syncthreads();
    sh[tid] = hi;
    __syncthreads();
    const Fr after = tid < 255 ? sh[tid + 1] : Fr::one();
    Fr iv = mul(mul(before, after), inv_total);  // 1 / (this thread's product)
#pragma unroll
    for (int k = PTS_CH - 1; k >= 0; k--) {
      const size_t e = seg * PTS_SEG + (size_t)k * 256 + tid;
      if (e < total) {
        const Fr r = hole[k] ? Fr::zero() : mul(iv, pre[k]);
        inv_out[e] = r;
        coef[e] = mul(w[e % n], r);
      }
      iv = mul(iv, a[k]);
    }
    __syncthreads();  // (sh and inv_total are rewritten by the next segment)
  }
}

// k_batch_bary with row b's coefficients and node those of point b / g
__global__ void __launch_bounds__(256) k_pts_bary(const Fr *__restrict__ y, const Fr *__restrict__ coef, size_t n,
                                                  size_t rows, size_t g, const size_t *__restrict__ j0, size_t tiles,
                                                  Fr *__restrict__ parts) {
  __shared__ Fr lds[256];
  const size_t t = blockIdx.x;
  for (size_t b = blockIdx.y; b < rows; b += gridDim.y) {
    const Fr *yb = y + b * n;
    const size_t p = b / g, jn = j0[p];
    const Fr *cf = coef + p * n;
    const bool node = jn < n;
    const Fr yoff = node ? yb[jn] : Fr::zero();
    Fr acc = Fr::zero();
    const size_t a = t * BARY_TILE, e = min(n, a + (size_t)BARY_TILE);
    for (size_t j = a + threadIdx.x; j < e; j += 256) acc = add(acc, mul(cf[j], node ? sub(yb[j], yoff) : yb[j]));
    lds[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) lds[threadIdx.x] = add(lds[threadIdx.x], lds[threadIdx.x + s]);
      __syncthreads();
    }
    if (threadIdx.x == 0) parts[b * tiles + t] = lds[0];
    __syncthreads();
  }
}

// k_batch_values per point: off a node value_b = ell_p S_b; at the node j0_p value_b = y_b,j0 and
// dq_b = S_b / w_j0 (one inverse per row at a node: nodes are the rare, deliberate points)
__global__ void __launch_bounds__(64) k_pts_values(const Fr *__restrict__ parts, size_t tiles, size_t rows, size_t g,
                                                   const Fr *__restrict__ y, size_t n, const size_t *__restrict__ j0,
                                                   const Fr *__restrict__ ell, const Fr *__restrict__ w,
                                                   Fr *__restrict__ values, Fr *__restrict__ dq) {
  const size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (b >= rows) return;
  const size_t p = b / g, jn = j0[p];
  Fr s = Fr::zero();
  for (size_t t = 0; t < tiles; t++) s = add(s, parts[b * tiles + t]);
  if (jn < n) {
    values[b] = y[b * n + jn];
    dq[b] = mul(s, inv(w[jn]));
  } else {
    values[b] = mul(ell[p], s);
    dq[b] = Fr::zero();
  }
}

// q[b n + j] = (value_b - y_bj) inv_pj, and dq_b at the node j0_p
__global__ void __launch_bounds__(256) k_pts_quotients(const Fr *__restrict__ y, const Fr *__restrict__ inv_all,
                                                       const Fr *__restrict__ values, const Fr *__restrict__ dq,
                                                       size_t n, size_t rows, size_t g,
                                                       const size_t *__restrict__ j0, Fr *__restrict__ q) {
  const size_t total = rows * n;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t b = e / n, j = e - b * n, p = b / g;
    q[e] = j == j0[p] ? dq[b] : mul(sub(values[b], y[e]), inv_all[p * n + j]);
  }
}

// ---------------------------------------------------------------- the three operations
static void set_identity(G1Affine *out, size_t rows) {
  if (rows) std::memset((void *)out, 0, sizeof(G1Affine) * rows);
}

// rows x n Montgomery scalars on the device over `base` (n points): the batched route when plan_batch
// takes it (false: it does not -- the caller loops over the single-vector function)
static bool batch_over_base(Ctx *c, const G1Affine *base, const Fr *d_s, size_t n, size_t rows, bool basis_ok,
                            const BatchLimits &lim, G1Affine *out_host, BatchReport &R) {
  R = BatchReport();
  R.route = BATCH_ROUTE_ROWS;
  R.groups = rows;
  R.group_rows = 1;
  // (no batched route whatever the scalars' width: no bit-length pass either)
  if (!basis_ok || n == 0 || lim.force_route == BATCH_ROUTE_ROWS || (lim.force_route < 0 && rows < 2)) return false;
  const unsigned bits = msm_batch_bits_dev(c, d_s, rows * n);
  BatchPlan B;
  if (bits) {
    B = plan_batch(n, rows, (int)bits, true, lim);
    if (B.route != BATCH_ROUTE_BATCHED) return false;
  }
  R.route = BATCH_ROUTE_BATCHED;
  if (!bits) {  // every scalar zero
    R.groups = 0;
    set_identity(out_host, rows);
    return true;
  }
  R.groups = B.groups;
  R.group_rows = B.group_rows;
  DevBuf ob;
  G1Affine *d_out = (G1Affine *)ob.ensure(sizeof(G1Affine) * rows);
  msm_batch_groups_dev(c, base, d_s, n, rows, bits, B, d_out, &R);
  TNS_HIP(hipMemcpy(out_host, d_out, sizeof(G1Affine) * rows, hipMemcpyDeviceToHost));
  return true;
}

void msm_batch_srs(Ctx *c, const Srs &srs, const Fr *d_s, size_t n, size_t rows, const BatchLimits &lim,
                   G1Affine *out_host, BatchReport *rep) {
  BatchReport R;
  if (n == 0) {
    set_identity(out_host, rows);
  } else if (!batch_over_base(c, srs.points.as<G1Affine>(), d_s, n, rows, true, lim, out_host, R)) {
    for (size_t b = 0; b < rows; b++) out_host[b] = commit_dev(c, srs, d_s + b * n, n);
  }
  if (rep) *rep = R;
}

void commit_evals_batch(Ctx *c, const Srs &srs, const Fr *d_y, size_t n, size_t rows, const BatchLimits &lim,
                        G1Affine *out_host, BatchReport *rep) {
  BatchReport R;
  const LagrangeBasis *basis = lagrange_basis_dev(c, srs, n, 0, n);
  const G1Affine *base = basis ? basis->points.as<G1Affine>() : nullptr;
  if (!batch_over_base(c, base, d_y, n, rows, basis != nullptr, lim, out_host, R)) {
    DevBuf cf;
    for (size_t b = 0; b < rows; b++) {
      EvalPoly p;
      p.y = d_y + b * n;
      p.N = p.cnt = n;
      p.coeffs = (Fr *)cf.ensure(sizeof(Fr) * n);
      out_host[b] = commit_evals(c, srs, p, comm_self());
    }
  }
  if (rep) *rep = R;
}

void open_evals_batch(Ctx *c, const Srs &srs, const Fr *d_y, size_t n, size_t rows, const Fr &z, const BatchLimits &lim,
                      Fr *values_host, G1Affine *proofs_host, BatchReport *rep) {
  BatchReport R;
  R.route = BATCH_ROUTE_ROWS;
  R.groups = rows;
  R.group_rows = 1;
  const LagrangeBasis *basis = lagrange_basis_dev(c, srs, n, 0, n);
  bool done = false;
  // (the route before the scalars exist: the quotients are full-width field elements)
  if (plan_batch(n, rows, 254, basis != nullptr, lim).route == BATCH_ROUTE_BATCHED) {
    hipStream_t st = c->stream;
    const size_t j0 = fr_is_node(z, n) ? (size_t)from_mont(z).v[0] | ((size_t)from_mont(z).v[1] << 32) : SIZE_MAX;
    const size_t tiles = (n + BARY_TILE - 1) / BARY_TILE;
    const Fr *w = bary_weights_dev(c, n, 0, n);
    DevBuf ib, qb, pb, vb;
    Fr *inv = (Fr *)ib.ensure(sizeof(Fr) * (2 * n + 1)), *coef = inv + n, *ell = coef + n;
    Fr *q = (Fr *)qb.ensure(sizeof(Fr) * rows * n);
    Fr *parts = (Fr *)pb.ensure(sizeof(Fr) * rows * tiles);
    Fr *vals = (Fr *)vb.ensure(sizeof(Fr) * 2 * rows), *dq = vals + rows;
    try {
      lagrange_inverses_dev(c, n, z, j0, inv, ell);
      {
        TNS_PROF(c, "open_batch_prep", 32.0 * 3 * rows * n);
        k_batch_coef<<<grid_for(n, 256), 256, 0, st>>>(w, inv, n, coef);
        TNS_LAUNCH_CHECK();
        k_batch_bary<<<dim3((unsigned)tiles, (unsigned)std::min<size_t>(rows, 32768)), 256, 0, st>>>(d_y, coef, n, rows,
                                                                                                   j0, tiles, parts);
        TNS_LAUNCH_CHECK();
        k_batch_values<<<grid_for(rows, 64, 1u << 30), 64, 0, st>>>(parts, tiles, rows, d_y, n, j0, ell, w, vals, dq);
        TNS_LAUNCH_CHECK();
        k_batch_quotients<<<grid_for(rows * n, 256, 1u << 16), 256, 0, st>>>(d_y, inv, vals, dq, n, rows, j0, q);
        TNS_LAUNCH_CHECK();
      }
      done = batch_over_base(c, basis->points.as<G1Affine>(), q, n, rows, true, lim, proofs_host, R);
      if (done) TNS_HIP(hipMemcpy(values_host, vals, sizeof(Fr) * rows, hipMemcpyDeviceToHost));  // one copy
      else TNS_HIP(hipStreamSynchronize(st));
    } catch (...) {  // the scratch above dies with the error: nothing may still run on it
      (void)hipStreamSynchronize(st);
      throw;
    }
  }
  if (!done) {
    DevBuf cf, s;
    for (size_t b = 0; b < rows; b++) {
      EvalPoly p;
      p.y = d_y + b * n;
      p.N = p.cnt = n;
      p.coeffs = (Fr *)cf.ensure(sizeof(Fr) * n);
      p.basis = basis;
      open_evals(c, srs, p, z, &values_host[b], &proofs_host[b], s, comm_self());
    }
  }
  if (rep) *rep = R;
}

void open_evals_batch_points(Ctx *c, const Srs &srs, const Fr *d_y, size_t n, size_t rows, const Fr *points_host,
                             size_t g, const BatchLimits &lim, Fr *values_host, G1Affine *proofs_host,
                             BatchReport *rep) {
  BatchReport R;
  R.route = BATCH_ROUTE_ROWS;
  R.groups = rows;
  R.group_rows = 1;
  if (g == 0) throw Error(TNS_ERR_INVALID_PARAMETERS, "rows per opening point must be positive");
  const LagrangeBasis *basis = lagrange_basis_dev(c, srs, n, 0, n);
  bool done = false;
  if (plan_batch(n, rows, 254, basis != nullptr, lim).route == BATCH_ROUTE_BATCHED) {
    hipStream_t st = c->stream;
    const size_t P = (rows + g - 1) / g, total = P * n;
    const size_t tiles = (n + BARY_TILE - 1) / BARY_TILE;
    const Fr *w = bary_weights_dev(c, n, 0, n);
    // the points and their node indices: one upload
    std::vector<uint8_t> hp(P * (sizeof(Fr) + sizeof(size_t)));
    std::memcpy(hp.data(), points_host, sizeof(Fr) * P);
    size_t *hj = (size_t *)(hp.data() + sizeof(Fr) * P);
    for (size_t p = 0; p < P; p++) {
      const Fr k = from_mont(points_host[p]);
      hj[p] = fr_is_node(points_host[p], n) ? (size_t)k.v[0] | ((size_t)k.v[1] << 32) : SIZE_MAX;
    }
    DevBuf zb, ib, qb, pb, vb;
    Fr *z = (Fr *)zb.ensure(hp.size() + sizeof(Fr) * P), *ell = z + P;
    const size_t *j0 = (const size_t *)(ell + P);
    Fr *inv_all = (Fr *)ib.ensure(sizeof(Fr) * 2 * total), *coef = inv_all + total;
    Fr *q = (Fr *)qb.ensure(sizeof(Fr) * rows * n);
    Fr *parts = (Fr *)pb.ensure(sizeof(Fr) * rows * tiles);
    Fr *vals = (Fr *)vb.ensure(sizeof(Fr) * 2 * rows), *dq = vals + rows;
    try {
      TNS_HIP(hipMemcpyAsync(z, hp.data(), sizeof(Fr) * P, hipMemcpyHostToDevice, st));
      TNS_HIP(hipMemcpyAsync((void *)j0, hj, sizeof(size_t) * P, hipMemcpyHostToDevice, st));
      {
        TNS_PROF(c, "open_scan", 32.0 * 3 * total);
        k_pts_ell<<<grid_for(P, 1, 1u << 16), 256, 0, st>>>(z, n, P, ell);
        TNS_LAUNCH_CHECK();
        k_pts_inv<<<grid_for(total, PTS_SEG, 1u << 20), 256, 0, st>>>(z, w, n, total, inv_all, coef);
        TNS_LAUNCH_CHECK();
      }
      {
        TNS_PROF(c, "open_batch_prep", 32.0 * 3 * rows * n);
        k_pts_bary<<<dim3((unsigned)tiles, (unsigned)std::min<size_t>(rows, 32768)), 256, 0, st>>>(d_y, coef, n, rows, g,
                                                                                                 j0, tiles, parts);
        TNS_LAUNCH_CHECK();
        k_pts_values<<<grid_for(rows, 64, 1u << 30), 64, 0, st>>>(parts, tiles, rows, g, d_y, n, j0, ell, w, vals, dq);
        TNS_LAUNCH_CHECK();
        k_pts_quotients<<<grid_for(rows * n, 256, 1u << 16), 256, 0, st>>>(d_y, inv_all, vals, dq, n, rows, g, j0, q);
        TNS_LAUNCH_CHECK();
      }
      done = batch_over_base(c, basis->points.as<G1Affine>(), q, n, rows, true, lim, proofs_host, R);
      if (done) TNS_HIP(hipMemcpy(values_host, vals, sizeof(Fr) * rows, hipMemcpyDeviceToHost));  // one copy
      else TNS_HIP(hipStreamSynchronize(st));
    } catch (...) {  // the scratch above (and the host staging of the points) dies with the error
      (void)hipStreamSynchronize(st);
      throw;
    }
  }
  if (!done) {
    DevBuf cf, s;
    for (size_t b = 0; b < rows; b++) {
      EvalPoly p;
      p.y = d_y + b * n;
      p.N = p.cnt = n;
      p.coeffs = (Fr *)cf.ensure(sizeof(Fr) * n);
      p.basis = basis;
      open_evals(c, srs, p, points_host[b / g], &values_host[b], &proofs_host[b], s, comm_self());
    }
  }
  if (rep) *rep = R;
}

// ---------------------------------------------------------------- the C ABI
namespace {

enum BatchOp { OP_MSM, OP_COMMIT, OP_OPEN, OP_OPEN_POINTS };

// the checks of all eight entry points, in the order tns.h documents them; true: nothing to do
bool batch_checks(const tns_ctx *ctx, const tns_srs *srs, const void *in, size_t n, size_t batch, const void *out,
                  BatchOp op, const void *z, const void *values) {
  if (!ctx || !srs) throw Error(TNS_ERR_INVALID_PARAMETERS, "null context or SRS");
  if (batch == 0) return true;
  if ((n && !in) || !out || ((op == OP_OPEN || op == OP_OPEN_POINTS) && (!z || !values)))
    throw Error(TNS_ERR_INVALID_PARAMETERS, "null input or output array");
  const Srs &s = srs->s;
  if (s.first != 0 || s.held < s.n) throw Error(TNS_ERR_INVALID_PARAMETERS, "batched calls need the whole SRS (this is a shard)");
  if (n && batch > BATCH_MAX_SCALARS / n) throw Error(TNS_ERR_INVALID_PARAMETERS, "batch * n exceeds 2^32 scalars");
  if (batch > BATCH_MAX_SCALARS) throw Error(TNS_ERR_INVALID_PARAMETERS, "batch exceeds 2^32 rows");
  if (op != OP_MSM && n == 0) throw Error(TNS_ERR_POLYNOMIAL, "empty evaluation vector");
  if (n > s.n) throw Error(TNS_ERR_COMMITMENT, "Polynomial degree exceeds setup size");
  return false;
}

int batch_call(tns_ctx *ctx, const tns_srs *srs, const uint64_t *in, size_t n, size_t batch, const uint64_t *z,
               uint64_t *values_out, uint64_t *out_affine, BatchOp op, bool resident) {
  return guarded([&]() {
    if (batch_checks(ctx, srs, in, n, batch, out_affine, op, z, values_out)) return (int)TNS_OK;
    CtxScope g(&ctx->c);
    DevBuf d;
    std::vector<G1Affine> out(batch);
    const bool opens = op == OP_OPEN || op == OP_OPEN_POINTS;
    std::vector<Fr> vals(opens ? batch : 0);
    try {
      const Fr *rows = (const Fr *)on_device(&ctx->c, in, sizeof(Fr) * batch * n, resident, d);  // (one upload)
      if (op == OP_MSM) {
        msm_batch_srs(&ctx->c, srs->s, rows, n, batch, BatchLimits(), out.data(), nullptr);
      } else if (op == OP_COMMIT) {
        commit_evals_batch(&ctx->c, srs->s, rows, n, batch, BatchLimits(), out.data(), nullptr);
      } else if (op == OP_OPEN) {
        Fr zz;
        std::memcpy(&zz, z, sizeof zz);
        open_evals_batch(&ctx->c, srs->s, rows, n, batch, zz, BatchLimits(), vals.data(), out.data(), nullptr);
      } else {  // z: batch points, one a row
        std::vector<Fr> pts(batch);
        std::memcpy((void *)pts.data(), z, sizeof(Fr) * batch);
        open_evals_batch_points(&ctx->c, srs->s, rows, n, batch, pts.data(), 1, BatchLimits(), vals.data(), out.data(),
                                nullptr);
      }
      TNS_HIP(hipStreamSynchronize(ctx->c.stream));
    } catch (...) {  // (the upload buffer dies with the error)
      (void)hipStreamSynchronize(ctx->c.stream);
      throw;
    }
    if (opens) std::memcpy(values_out, vals.data(), sizeof(Fr) * batch);
    std::memcpy(out_affine, out.data(), sizeof(G1Affine) * batch);
    return (int)TNS_OK;
  });
}

}  // namespace
}  // namespace tns

using namespace tns;

extern "C" {

int tns_msm_batch(tns_ctx *ctx, const tns_srs *srs, const uint64_t *scalars, size_t n, size_t batch,
                  uint64_t *out_affine) {
  return batch_call(ctx, srs, scalars, n, batch, nullptr, nullptr, out_affine, OP_MSM, false);
}
int tns_msm_batch_device(tns_ctx *ctx, const tns_srs *srs, const uint64_t *d_scalars, size_t n, size_t batch,
                         uint64_t *out_affine) {
  return batch_call(ctx, srs, d_scalars, n, batch, nullptr, nullptr, out_affine, OP_MSM, true);
}
int tns_kzg_commit_evals_batch(tns_ctx *ctx, const tns_srs *srs, const uint64_t *evals, size_t n, size_t batch,
                               uint64_t *out_affine) {
  return batch_call(ctx, srs, evals, n, batch, nullptr, nullptr, out_affine, OP_COMMIT, false);
}
int tns_kzg_commit_evals_batch_device(tns_ctx *ctx, const tns_srs *srs, const uint64_t *d_evals, size_t n, size_t batch,
                                      uint64_t *out_affine) {
  return batch_call(ctx, srs, d_evals, n, batch, nullptr, nullptr, out_affine, OP_COMMIT, true);
}
int tns_kzg_open_evals_batch(tns_ctx *ctx, const tns_srs *srs, const uint64_t *evals, size_t n, size_t batch,
                             const uint64_t z[4], uint64_t *values_out, uint64_t *proofs_affine_out) {
  return batch_call(ctx, srs, evals, n, batch, z, values_out, proofs_affine_out, OP_OPEN, false);
}
int tns_kzg_open_evals_batch_device(tns_ctx *ctx, const tns_srs *srs, const uint64_t *d_evals, size_t n, size_t batch,
                                    const uint64_t z[4], uint64_t *values_out, uint64_t *proofs_affine_out) {
  return batch_call(ctx, srs, d_evals, n, batch, z, values_out, proofs_affine_out, OP_OPEN, true);
}
int tns_kzg_open_evals_batch_points(tns_ctx *ctx, const tns_srs *srs, const uint64_t *evals, size_t n, size_t batch,
                                    const uint64_t *points, uint64_t *values_out, uint64_t *proofs_affine_out) {
  return batch_call(ctx, srs, evals, n, batch, points, values_out, proofs_affine_out, OP_OPEN_POINTS, false);
}
int tns_kzg_open_evals_batch_points_device(tns_ctx *ctx, const tns_srs *srs, const uint64_t *d_evals, size_t n,
                                           size_t batch, const uint64_t *points, uint64_t *values_out,
                                           uint64_t *proofs_affine_out) {
  return batch_call(ctx, srs, d_evals, n, batch, points, values_out, proofs_affine_out, OP_OPEN_POINTS, true);
}

}  // extern "C"
