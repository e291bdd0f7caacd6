// batchprobe.hip -- the batched MSM's internal entry points (csrc/kzg_batch.hip: msm_batch_srs,
// commit_evals_batch, open_evals_batch) with forced limits, for tests/test_gpu_msm_batch_probe.py:
// one C entry point uploads the rows, calls the shipped function with the BatchLimits it is given
// and returns the rows' points with the route, groups, window plan and sort passes the code took.
// Nothing is re-implemented on the device: this file has no kernel, and libtns_batchprobe.so links
// libtns.so for every symbol it calls.
#include <hip/hip_runtime.h>

#include <vector>

#include "abi.hpp"

namespace {
using namespace tns;
// the words of batchprobe_run's `info`, in order
enum { I_ROUTE, I_GROUPS, I_GROUP_ROWS, I_C, I_W, I_NPASS, I_COUNT };
}  // namespace

extern "C" {

int batchprobe_info_words() { return I_COUNT; }

// op 0: msm_batch_srs, 1: commit_evals_batch, 2: open_evals_batch (z, values_out required).
// rows: batch x n Montgomery Fr, on the host (resident 0: uploaded here) or already on the device
// (resident 1: tools/msm_batch_bench.py times the forced routes without the copy).  force_route: -1 the rule, 0 rows, 1 batched; entry_limit,
// ws_limit, crossover: 0 = the shipped default.  out_affine: batch x uint64_t[8].
// Returns 0, a TNS_* status, or -1 for arguments the entry point does not take.
int batchprobe_run(tns_ctx *ctx, const tns_srs *srs, int op, const uint64_t *rows, uint64_t n, uint64_t batch,
                   const uint64_t *z, int resident, int force_route, uint64_t entry_limit, uint64_t ws_limit, uint64_t crossover,
                   uint64_t *values_out, uint64_t *out_affine, int64_t *info) {
  if (!ctx || !srs || !rows || !out_affine || !info || op < 0 || op > 2 || n == 0 || batch == 0 || n > srs->s.n ||
      (op == 2 && (!z || !values_out)) || force_route < -1 || force_route > 1)
    return -1;
  return guarded([&]() {
    CtxScope g(&ctx->c);
    Ctx *c = &ctx->c;
    BatchLimits lim;
    lim.force_route = force_route;
    if (entry_limit) lim.entries = (size_t)entry_limit;
    if (ws_limit) lim.ws_bytes = (size_t)ws_limit;
    if (crossover) lim.crossover = (size_t)crossover;
    DevBuf d;
    const Fr *dr = (const Fr *)rows;
    if (!resident) {
      Fr *up = (Fr *)d.ensure(sizeof(Fr) * batch * n);
      TNS_HIP(hipMemcpy(up, rows, sizeof(Fr) * batch * n, hipMemcpyHostToDevice));
      dr = up;
    }
    std::vector<G1Affine> out(batch);
    std::vector<Fr> vals(batch);
    BatchReport R;
    try {
      if (op == 0) {
        msm_batch_srs(c, srs->s, dr, n, batch, lim, out.data(), &R);
      } else if (op == 1) {
        commit_evals_batch(c, srs->s, dr, n, batch, lim, out.data(), &R);
      } else {
        Fr zz;
        std::memcpy(&zz, z, sizeof zz);
        open_evals_batch(c, srs->s, dr, n, batch, zz, lim, vals.data(), out.data(), &R);
        std::memcpy(values_out, vals.data(), sizeof(Fr) * batch);
      }
    } catch (...) {
      (void)hipDeviceSynchronize();  // (d is freed on return: nothing may still read it)
      throw;
    }
    TNS_HIP(hipDeviceSynchronize());
    std::memcpy(out_affine, out.data(), sizeof(G1Affine) * batch);
    info[I_ROUTE] = R.route;
    info[I_GROUPS] = (int64_t)R.groups;
    info[I_GROUP_ROWS] = (int64_t)R.group_rows;
    info[I_C] = R.c;
    info[I_W] = R.W;
    info[I_NPASS] = R.npass;
    return (int)TNS_OK;
  });
}

}  // extern "C"
