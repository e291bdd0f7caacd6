// msm_batch_plan.hpp -- how a batch of `rows` MSMs over the same n points runs (msm.hip
// msm_batch_dev; tns_msm_batch, tns_kzg_commit_evals_batch, tns_kzg_open_evals_batch and their
// _device forms): the route, the window plan of one group and how the rows split into groups.
// Host arithmetic alone (plain C++17, no HIP), like msm_plan.hpp: tests/test_msm_batch_plan_cpu.py.
#pragma once
#include "msm_plan.hpp"

namespace tns {

// BATCH_ROUTE_ROWS: the single-vector functions in a loop on the one uploaded copy;
// BATCH_ROUTE_BATCHED: groups of rows, each ONE sort, accumulation, reduction and finish kernel
enum { BATCH_ROUTE_ROWS = 0, BATCH_ROUTE_BATCHED = 1 };

// what one sort allows: W B n < 2^31 entries (32-bit entry positions, k_accumulate) and keys of at
// most 31 bits
constexpr size_t BATCH_ENTRY_LIMIT = (size_t)1 << 31;
constexpr int BATCH_KEY_BITS = 31;
// A group's buffers live in lane 0's workspaces, which keep their high-water mark for the
// context's life: a group is sized so that batch_ws_bytes stays below this cap (tns.h states it)
constexpr size_t BATCH_WS_CAP = (size_t)1 << 30;
// batch * n above this is refused (TNS_ERR_INVALID_PARAMETERS): 2^32 scalars are 128 GiB
constexpr size_t BATCH_MAX_SCALARS = (size_t)1 << 32;
// Rows of at least this many digit entries (W n: windows x scalars, so narrow scalars count for
// less) take the row route: one MSM of that size fills the device by itself.  Measured
// (profiles/msm_batch_bench.json): full-width rows of 2^16 scalars (22 windows,
// 1.4 M entries) are faster batched in every scalar family, those of 2^18 (17 windows, 4.5 M) are
// not; 30-bit rows of 2^18 (2 windows, 0.5 M) are.
#ifndef TNS_BATCH_CROSSOVER
#define TNS_BATCH_CROSSOVER ((size_t)1 << 22)
#endif
constexpr size_t BATCH_CROSSOVER = TNS_BATCH_CROSSOVER;

// the limits as arguments (defaults: the real ones) so that tests and the probe can force a route
// or a split with small numbers
struct BatchLimits {
  size_t entries = BATCH_ENTRY_LIMIT;
  size_t ws_bytes = BATCH_WS_CAP;
  size_t crossover = BATCH_CROSSOVER;  // digit entries a row
  int force_route = -1;  // BATCH_ROUTE_*: taken whenever it is possible at all
};

struct BatchPlan {
  int route = BATCH_ROUTE_ROWS;
  MsmPlan P;                // a full group's plan: rows = group_rows, Wr = group_rows W bucket sets
  size_t group_rows = 0;    // rows of every group but the last
  size_t groups = 0;        // the groups cover the rows in order: group k = rows [k group_rows, ...)
  size_t ws_bytes = 0;      // batch_ws_bytes of a full group
};

inline int ceil_log2_sz(size_t x) {
  int b = 0;
  while (((size_t)1 << b) < x) b++;
  return b;
}

// the window of a batch's rows: the per-window optimum of ONE row, as plan_msm takes it (the cost
// model W n + 3 W 2^(c-1) per row: a batch multiplies both terms by its rows)
inline int batch_window(size_t n, int bits) { return best_window(n, bits, 20, false, 23); }

// the plan of g rows of n scalars of `bits` bits sorted as one: g W bucket sets; g == 1 is
// plan_msm's per-window plan to the letter
inline MsmPlan plan_batch_group(size_t n, size_t g, int bits) {
  MsmPlan P;
  P.c = batch_window(n, bits);
  P.W = windows_for(bits, P.c);
  if (g > 1) {
    P.rows = (uint32_t)g;
    P.n_row = n;
  }
  P.half = (size_t)1 << (P.c - 1);
  P.Wr = (int)(g * (size_t)P.W);
  P.bucket_bits = ceil_log2_sz((size_t)P.Wr) + P.c - 1;
  P.nb = (size_t)P.Wr * P.half;
  return P;
}

// Device bytes a group of g rows holds in the lane's workspaces, an upper bound: per digit entry 16 B of
// keys and values (ping and pong), <= 9 B of accumulation chunk partials, bounds and fix levels
// (256-byte head/tail pairs, chunks of >= 32 entries) and <= 3 B of pass histograms; per bucket its
// 128-byte sum, 64 B of reduction level sums and <= 128 B of masked-sum parts; per key value the
// sort's segment, tile and count tables
inline size_t batch_ws_bytes(size_t n, size_t g, int c, int W) {
  const size_t E = (size_t)W * g * n, nb = (g * (size_t)W) << (c - 1);
  const int keybits = ceil_log2_sz(g * (size_t)W) + c - 1;
  return 28 * E + 320 * nb + 40 * ((size_t)1 << keybits);
}

// whether g rows fit one sort under the limits
inline bool batch_group_fits(size_t n, size_t g, int c, int W, const BatchLimits &lim) {
  if (g == 0 || g > ((size_t)1 << 24) / (size_t)W) return false;  // (g W: an int's worth of bucket sets)
  if ((double)W * (double)g * (double)n >= (double)lim.entries) return false;
  if (ceil_log2_sz(g * (size_t)W) + c - 1 > BATCH_KEY_BITS) return false;
  return batch_ws_bytes(n, g, c, W) <= lim.ws_bytes;
}

// The route of `rows` MSMs of n scalars (the largest of all rows x n is `bits` bits long) and its
// groups.  basis_ok: the base the batched pass would run over exists (the evals calls without a
// Lagrange basis of n nodes can only loop over the single calls).
inline BatchPlan plan_batch(size_t n, size_t rows, int bits, bool basis_ok, const BatchLimits &lim = BatchLimits()) {
  BatchPlan B;
  B.group_rows = 1;
  B.groups = rows;
  if (n == 0 || rows == 0 || bits <= 0 || !basis_ok) return B;
  const int c = batch_window(n, bits), W = windows_for(bits, c);
  bool batched = rows > 1 && (double)W * (double)n < (double)lim.crossover;
  if (lim.force_route >= 0) batched = lim.force_route == BATCH_ROUTE_BATCHED;
  if (!batched || !batch_group_fits(n, 1, c, W, lim)) return B;
  size_t lo = 1, hi = rows;  // the largest g that fits (batch_group_fits is monotone in g)
  while (lo < hi) {
    const size_t mid = lo + (hi - lo + 1) / 2;
    if (batch_group_fits(n, mid, c, W, lim)) lo = mid;
    else hi = mid - 1;
  }
  B.route = BATCH_ROUTE_BATCHED;
  B.group_rows = lo;
  B.groups = (rows + lo - 1) / lo;
  B.P = plan_batch_group(n, lo, bits);
  B.ws_bytes = batch_ws_bytes(n, lo, c, W);
  return B;
}

}  // namespace tns
