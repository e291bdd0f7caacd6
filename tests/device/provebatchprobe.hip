// provebatchprobe.hip -- the batched provers' internal entry points (csrc/prove_batch.hip:
// twist_prove_batch, shout_prove_batch; their folds are csrc/zero_folds.hip's batched chain) and the per-row-point openings (csrc/kzg_batch.hip:
// open_evals_batch_points) with forced limits, for tests/test_gpu_prove_batch.py and
// tests/test_gpu_open_batch_points.py: each C entry point calls the shipped function with the
// BatchLimits it is given and returns the results with the route, groups and group rows that the
// commit and open stages took.  Like batchprobe.hip nothing is re-implemented on the device: this
// file has no kernel, and libtns_provebatchprobe.so links libtns.so for every symbol it calls.
#include <hip/hip_runtime.h>

#include <vector>

#include "abi.hpp"

namespace {
using namespace tns;
// the words of `info`, in order: the call's route, then (route, groups, group rows) of commitment 0,
// commitment 1, opening call 0, opening call 1, then the opening calls and their rows per point
enum { I_ROUTE, I_C0, I_C1 = I_C0 + 3, I_O0 = I_C1 + 3, I_O1 = I_O0 + 3, I_OPEN_CALLS = I_O1 + 3, I_ROWS_PER_POINT, I_COUNT };

BatchLimits limits(int force_route, uint64_t entry_limit, uint64_t ws_limit, uint64_t crossover) {
  BatchLimits lim;
  lim.force_route = force_route;
  if (entry_limit) lim.entries = (size_t)entry_limit;
  if (ws_limit) lim.ws_bytes = (size_t)ws_limit;
  if (crossover) lim.crossover = (size_t)crossover;
  return lim;
}
void put(int64_t *info, int at, const BatchReport &r) {
  info[at] = r.route;
  info[at + 1] = (int64_t)r.groups;
  info[at + 2] = (int64_t)r.group_rows;
}
void put_all(int64_t *info, const ProveBatchReport &r) {
  for (int i = 0; i < I_COUNT; i++) info[i] = 0;
  info[I_ROUTE] = r.route;
  put(info, I_C0, r.commit[0]);
  put(info, I_C1, r.commit[1]);
  put(info, I_O0, r.open[0]);
  put(info, I_O1, r.open[1]);
  info[I_OPEN_CALLS] = r.open_calls;
  info[I_ROWS_PER_POINT] = r.rows_per_point;
}
}  // namespace

extern "C" {

int provebatchprobe_info_words() { return I_COUNT; }

// force_route: -1 the rule, 0 rows, 1 batched; entry_limit, ws_limit, crossover: 0 = the shipped
// default.  resident: the inputs are device pointers.  Returns the call's status.
int provebatchprobe_twist(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, const uint64_t *addr,
                          const uint64_t *value, const uint8_t *is_write, uint64_t n_ops, uint64_t batch, int resident,
                          int force_route, uint64_t entry_limit, uint64_t ws_limit, uint64_t crossover, tns_proof *out,
                          int64_t *info) {
  if (!info || force_route < -1 || force_route > 1) return -1;
  ProveBatchReport r;
  const int st = twist_prove_batch(ctx, srs, params, addr, value, is_write, n_ops, batch, out, resident != 0,
                                   limits(force_route, entry_limit, ws_limit, crossover), &r);
  put_all(info, r);
  return st;
}

int provebatchprobe_shout(tns_ctx *ctx, const tns_srs *srs, const tns_params *params, const uint64_t *entries,
                          uint64_t n_entries, const uint64_t *indices, uint64_t n_lookups, uint64_t batch, int resident,
                          int force_route, uint64_t entry_limit, uint64_t ws_limit, uint64_t crossover, tns_proof *out,
                          int64_t *info) {
  if (!info || force_route < -1 || force_route > 1) return -1;
  ProveBatchReport r;
  const int st = shout_prove_batch(ctx, srs, params, entries, n_entries, indices, n_lookups, batch, out, resident != 0,
                                   limits(force_route, entry_limit, ws_limit, crossover), &r);
  put_all(info, r);
  return st;
}

// open_evals_batch_points on host rows (batch x n Montgomery Fr, uploaded here) with g rows a point:
// points = ceil(batch / g) x uint64_t[4].  info: route, groups, group rows (3 words).
int provebatchprobe_open(tns_ctx *ctx, const tns_srs *srs, const uint64_t *rows, uint64_t n, uint64_t batch,
                         const uint64_t *points, uint64_t g, int force_route, uint64_t entry_limit, uint64_t ws_limit,
                         uint64_t crossover, uint64_t *values_out, uint64_t *out_affine, int64_t *info) {
  if (!ctx || !srs || !rows || !points || !values_out || !out_affine || !info || n == 0 || batch == 0 || g == 0 ||
      n > srs->s.n || force_route < -1 || force_route > 1)
    return -1;
  return guarded([&]() {
    CtxScope scope(&ctx->c);
    Ctx *c = &ctx->c;
    DevBuf d;
    Fr *up = (Fr *)d.ensure(sizeof(Fr) * batch * n);
    TNS_HIP(hipMemcpy(up, rows, sizeof(Fr) * batch * n, hipMemcpyHostToDevice));
    const size_t P = (batch + g - 1) / g;
    std::vector<Fr> pts(P), vals(batch);
    std::memcpy((void *)pts.data(), points, sizeof(Fr) * P);
    std::vector<G1Affine> out(batch);
    BatchReport R;
    try {
      open_evals_batch_points(c, srs->s, up, n, batch, pts.data(), g,
                              limits(force_route, entry_limit, ws_limit, crossover), vals.data(), out.data(), &R);
    } catch (...) {
      (void)hipDeviceSynchronize();  // (d is freed on return: nothing may still read it)
      throw;
    }
    TNS_HIP(hipDeviceSynchronize());
    std::memcpy(values_out, vals.data(), sizeof(Fr) * batch);
    std::memcpy(out_affine, out.data(), sizeof(G1Affine) * batch);
    put(info, 0, R);
    return (int)TNS_OK;
  });
}

}  // extern "C"
