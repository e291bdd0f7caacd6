// sortprobe.hip -- the MSM's bucket sort (csrc/bucket_sort.hip) alone, for
// tests/test_gpu_bucket_sort.py: one C entry point hands scalars to the shipped
// tns::bucket_sort_begin / _passes / _finish (optionally through bucket_sort_precount_bits, as
// msm.hip's bits_launch + msm_launch_sort do) on the context's lane 0 and returns the order it
// produced with the geometry the code chose.  Nothing is re-implemented on the device: this file
// has no kernel, and libtns_sortprobe.so links libtns.so for every symbol it calls.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "abi.hpp"

namespace {

using namespace tns;

// the words of sortprobe_sort's `info`, in order
enum {
  I_NPASS, I_BITS0, I_KF0 = I_BITS0 + 8, I_PK = I_KF0 + 8, I_VO, I_TILE, I_IDENT, I_MULTI, I_BIG_ROUTE, I_CT, I_KS,
  I_ENTRIES, I_VALID0, I_VALID1, I_HAS_KEYS, I_PRE_BITS, I_PRE_OK, I_LOW64_USED, I_KEYBITS, I_WB, I_IBITS, I_LAST_S,
  I_COPIED, I_COUNT
};

}  // namespace

extern "C" {

int sortprobe_info_words() { return I_COUNT; }

// Sort the digit entries of n scalars for the plan (c, W, shared, stride, bucket_bits).
//   form 0: fr = n canonical 32-byte scalars; 1: fr = n Montgomery forms; 2: u64 = n_u64 <= n raw values
//   precount (form 1 only) 1: first bucket_sort_precount_bits, 2: the same with want_low64; the sort
//     then reads the SortInput it returned, its u64 low words when the bit length it wrote is <= 64
//     (sort_input_for_bits, as msm_launch_sort)
//   vals / keys: room for `cap` words each, bstart: for 2^bucket_bits + 1
// Returns 0, a TNS_* status (every HIP error: TNS_ERR_DEVICE, the message in tns_last_error()),
// or -1 for arguments the entry point does not take.
int sortprobe_sort(tns_ctx *ctx, int form, const void *fr, const uint64_t *u64, uint64_t n_u64, uint64_t n, int c,
                   int W, int shared, uint32_t stride, int bucket_bits, int precount, uint32_t *vals, uint32_t *keys,
                   uint64_t cap, uint32_t *bstart, int64_t *info) {
  if (!ctx || !info || !vals || !keys || !bstart || n == 0 || form < 0 || form > 2 || c < 2 || c > 23 || W < 1 ||
      bucket_bits < 1 || bucket_bits > 27 || (form == 2 ? (!u64 || n_u64 > n) : !fr) || (precount && form != 1) ||
      precount < 0 || precount > 2)
    return -1;
  return guarded([&]() {
    CtxScope g(&ctx->c);
    MsmLane &ln = ctx->c.lanes[0];
    hipStream_t st = ln.stream;
    for (int i = 0; i < I_COUNT; i++) info[i] = 0;
    DevBuf d_in, d_one;
    SortInput in;
    if (form == 2) {
      uint64_t *d = (uint64_t *)d_in.ensure(sizeof(uint64_t) * std::max<uint64_t>(n_u64, 1));
      if (n_u64) TNS_HIP(hipMemcpyAsync(d, u64, sizeof(uint64_t) * n_u64, hipMemcpyHostToDevice, st));
      in.u64 = d;
      in.n_u64 = n_u64;
    } else {
      Fr *d = (Fr *)d_in.ensure(sizeof(Fr) * n);
      TNS_HIP(hipMemcpyAsync(d, fr, sizeof(Fr) * n, hipMemcpyHostToDevice, st));
      in.fr = d;
      in.mont = form == 1;
    }
    const WindowPlan plan{c, W, shared != 0, bucket_bits, stride};
    uint32_t *words = (uint32_t *)ln.msm.words.ensure(2 * sizeof(uint32_t));
    // whether a compile-time pass-1 plan matches (c, W): the shipped answer, from a precount of one
    // zero scalar (it queues nothing when there is none; the sort below recounts either way)
    {
      Fr *one = (Fr *)d_one.ensure(sizeof(Fr));
      TNS_HIP(hipMemsetAsync(one, 0, sizeof(Fr), st));
      TNS_HIP(hipMemsetAsync(words, 0, 2 * sizeof(uint32_t), st));
      SortInput tmp;
      info[I_CT] = bucket_sort_precount_bits(ln, one, 1, plan, words, tmp, false) ? 1 : 0;
    }
    if (precount) {  // msm.hip bits_launch, then msm_launch_sort's low-word substitution
      TNS_HIP(hipMemsetAsync(words, 0, sizeof(uint32_t), st));
      const bool ok = bucket_sort_precount_bits(ln, in.fr, n, plan, words, in, precount == 2);
      info[I_PRE_OK] = ok ? 1 : 0;
      uint32_t b = 0;
      TNS_HIP(hipMemcpyAsync(&b, words, sizeof b, hipMemcpyDeviceToHost, st));
      TNS_HIP(hipStreamSynchronize(st));
      info[I_PRE_BITS] = ok ? (int64_t)b : -1;
      in = sort_input_for_bits(in, n, b);
      info[I_LOW64_USED] = in.low64 && in.u64 == in.low64;
    }
    BucketSortJob J;
    bucket_sort_begin(ln, in, n, plan, words, J);
    bucket_sort_passes(J);
    const bool pending = J.pending;
    info[I_LAST_S] = (int64_t)J.S;
    const BucketOrder o = bucket_sort_finish(J);
    TNS_HIP(hipStreamSynchronize(st));
    uint32_t valid[2] = {0, 0};
    TNS_HIP(hipMemcpy(valid, words, sizeof valid, hipMemcpyDeviceToHost));
    const SortGeom &sg = J.g;
    const uint64_t take = std::min<uint64_t>(std::min<uint64_t>(valid[0], cap), sg.E);
    if (take) TNS_HIP(hipMemcpy(vals, o.vals, sizeof(uint32_t) * take, hipMemcpyDeviceToHost));
    if (take && o.keys) TNS_HIP(hipMemcpy(keys, o.keys, sizeof(uint32_t) * take, hipMemcpyDeviceToHost));
    TNS_HIP(hipMemcpy(bstart, o.bstart, sizeof(uint32_t) * (((size_t)1 << bucket_bits) + 1), hipMemcpyDeviceToHost));
    info[I_NPASS] = sg.npass;
    for (int p = 0; p < 8; p++) {
      info[I_BITS0 + p] = sg.bits[p];
      info[I_KF0 + p] = sg.kf[p];
      // (a pass over S segments with S + 1 > SCAN_SMALL takes k_bs_tiles + exclusive_scan, not k_bs_geom)
      if (p >= 1 && p < sg.npass && !sg.one_launch[p]) info[I_BIG_ROUTE] = 1;
    }
    info[I_PK] = sg.pk;
    info[I_VO] = sg.vo;
    info[I_TILE] = sg.npass > 1 ? J.tile : 0;
    if (pending && J.readback) {  // the last pass's tile totals: all | those of multi-tile segments | entries
      const uint32_t *h = (const uint32_t *)J.readback;
      info[I_IDENT] = h[1] == 0;
      info[I_MULTI] = h[1];
    }
    info[I_KS] = o.ks;
    info[I_ENTRIES] = o.entries == SIZE_MAX ? -1 : (int64_t)o.entries;
    info[I_VALID0] = valid[0];
    info[I_VALID1] = valid[1];
    info[I_HAS_KEYS] = o.keys != nullptr;
    info[I_KEYBITS] = sg.keybits;
    info[I_WB] = sg.wb;
    info[I_IBITS] = sg.ibits;
    info[I_COPIED] = (int64_t)take;
    TNS_HIP(hipDeviceSynchronize());  // (d_in is freed on return: nothing of the sort may still read it)
    TNS_LAUNCH_CHECK();
    return TNS_OK;
  });
}

// the plan hint lane 0's last MSM of Montgomery scalars left: n, c, W, bucket_bits, shared
int sortprobe_hint(tns_ctx *ctx, int64_t out[5]) {
  if (!ctx || !out) return -1;
  return guarded([&]() {
    CtxScope g(&ctx->c);
    const MsmLane::PlanHint &h = ctx->c.lanes[0].hint;
    out[0] = (int64_t)h.n;
    out[1] = h.plan.c;
    out[2] = h.plan.W;
    out[3] = h.plan.bucket_bits;
    out[4] = h.plan.shared ? 1 : 0;
    return TNS_OK;
  });
}

}  // extern "C"
