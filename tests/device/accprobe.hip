// accprobe.hip -- the MSM's stages after the sort (csrc/msm.hip: the accumulation with its fix-up,
// the bucket reduction and the host finish) alone, for tests/test_gpu_accumulate.py: one C entry
// point uploads a point pool and one or two bucket orders written by the test and hands them to the
// shipped tns::msm_from_order_dev, which runs msm_launch_accumulate, msm_launch_tails and the host
// finish as every MSM does.  Nothing is re-implemented on the device: this file has no kernel, and
// libtns_accprobe.so links libtns.so for every symbol it calls.  Every index a kernel would follow
// is checked on the host first; an order that breaks the sort's promises is refused (-1), not run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "abi.hpp"

namespace {

using namespace tns;

// the words of accprobe_run's `info`, in order
enum {
  I_L0, I_L1, I_G1, I_G, I_NBITS, I_SPECS, I_CH, I_NCH, I_TREE, I_LG0, I_WEIGHT, I_SUM_N, I_WR, I_HALF, I_NB,
  I_INPUTS_INTACT, I_COUNT
};

constexpr int XW = (int)(sizeof(G1Xyzz) / 4);  // 32 words a point

}  // namespace

extern "C" {

// one bucket order and what comes back for it (tests/test_gpu_accumulate.py mirrors the layout)
struct accprobe_set {
  const uint32_t *vals;    // entries: point index | sign << 31
  const uint32_t *bstart;  // nb + 1 bucket starts, bstart[nb] = entries
  const uint32_t *keys;    // optional: entries keys, bucket = key >> ks
  int32_t ks, acc_k;
  uint64_t entries, nchunks;
  uint32_t *buckets;  // out, optional: nb x 32 words, the buckets after the fix-up (lazy domain)
  uint32_t *sums;     // out: Wr x 32 words, the window sums before Horner
  uint32_t *result;   // out: 32 words
  uint32_t flags;     // out: valid[1] after the run
  int32_t fix_levels;  // out: fix levels built
};

int accprobe_info_words() { return I_COUNT; }

// Run nj = 1 or 2 orders (two: shared layout only) over `pool` (npool affine points, 16 words each,
// the identity as all zeros) with the plan (c, W, shared).
// Returns 0, a TNS_* status (every HIP error: TNS_ERR_DEVICE, the message in tns_last_error()),
// or -1 for arguments the entry point does not take.
int accprobe_run(tns_ctx *ctx, const uint32_t *pool, uint64_t npool, int c, int W, int shared, int nj,
                 accprobe_set *sets, int64_t *info) {
  if (!ctx || !pool || !sets || !info || npool == 0 || npool >= ((uint64_t)1 << 31) || c < 4 || c > 23 || W < 1 ||
      W > 64 || nj < 1 || nj > 2 || (nj == 2 && !shared))
    return -1;
  MsmPlan P;
  P.c = c;
  P.W = W;
  P.shared = shared != 0;
  finish_plan(P);
  if (P.nb > ((size_t)1 << 24)) return -1;
  for (int j = 0; j < nj; j++) {  // what the sort promises and the kernels rely on
    const accprobe_set &s = sets[j];
    if (!s.vals || !s.bstart || !s.sums || !s.result || s.entries == 0 || s.entries >= ((uint64_t)1 << 31) ||
        s.acc_k < 1 || s.acc_k > 4096 || s.nchunks == 0 || s.nchunks >= ((uint64_t)1 << 31) / s.acc_k ||
        s.nchunks * (uint64_t)s.acc_k < s.entries || s.ks < 0 || s.ks > 8)
      return -1;
    if (s.bstart[0] != 0 || s.bstart[P.nb] != s.entries) return -1;
    for (size_t b = 0; b < P.nb; b++)
      if (s.bstart[b] > s.bstart[b + 1]) return -1;
    for (uint64_t p = 0; p < s.entries; p++)
      if ((s.vals[p] & 0x7fffffffu) >= npool) return -1;
    if (s.keys)
      for (size_t b = 0; b < P.nb; b++)
        for (uint32_t p = s.bstart[b]; p < s.bstart[b + 1]; p++)
          if ((s.keys[p] >> s.ks) != b) return -1;
  }
  return guarded([&]() {
    CtxScope g(&ctx->c);
    hipStream_t st = ctx->c.lanes[0].stream;
    for (int i = 0; i < I_COUNT; i++) info[i] = 0;
    DevBuf d_pool, d_vals[2], d_bstart[2], d_keys[2], d_valid[2];
    const size_t pool_bytes = sizeof(G1Affine) * npool;
    G1Affine *pts = (G1Affine *)d_pool.ensure(pool_bytes);
    TNS_HIP(hipMemcpyAsync(pts, pool, pool_bytes, hipMemcpyHostToDevice, st));
    OrderedSet os[2];
    for (int j = 0; j < nj; j++) {
      const accprobe_set &s = sets[j];
      uint32_t *v = (uint32_t *)d_vals[j].ensure(4 * s.entries);
      uint32_t *b = (uint32_t *)d_bstart[j].ensure(4 * (P.nb + 1));
      uint32_t *k = s.keys ? (uint32_t *)d_keys[j].ensure(4 * s.entries) : nullptr;
      uint32_t *w = (uint32_t *)d_valid[j].ensure(2 * sizeof(uint32_t));
      const uint32_t words[2] = {(uint32_t)s.entries, 0};
      TNS_HIP(hipMemcpyAsync(v, s.vals, 4 * s.entries, hipMemcpyHostToDevice, st));
      TNS_HIP(hipMemcpyAsync(b, s.bstart, 4 * (P.nb + 1), hipMemcpyHostToDevice, st));
      if (k) TNS_HIP(hipMemcpyAsync(k, s.keys, 4 * s.entries, hipMemcpyHostToDevice, st));
      TNS_HIP(hipMemcpyAsync(w, words, sizeof words, hipMemcpyHostToDevice, st));
      TNS_HIP(hipStreamSynchronize(st));  // (`words` is this iteration's)
      os[j] = OrderedSet{BucketOrder{k, v, b, s.ks, (size_t)s.entries}, w, pts, s.acc_k, (size_t)s.nchunks};
    }
    OrderedMsm out;
    msm_from_order_dev(&ctx->c, P, os, nj, out);
    TNS_HIP(hipStreamSynchronize(st));
    bool intact = true;
    std::vector<uint32_t> back;
    auto same = [&](const void *dev, const void *host, size_t bytes) {
      back.resize(bytes / 4);
      TNS_HIP(hipMemcpy(back.data(), dev, bytes, hipMemcpyDeviceToHost));
      if (std::memcmp(back.data(), host, bytes)) intact = false;
    };
    same(pts, pool, pool_bytes);
    for (int j = 0; j < nj; j++) {
      accprobe_set &s = sets[j];
      same(os[j].order.vals, s.vals, 4 * s.entries);
      same(os[j].order.bstart, s.bstart, 4 * (P.nb + 1));
      if (s.keys) same(os[j].order.keys, s.keys, 4 * s.entries);
      uint32_t words[2] = {0, 0};
      TNS_HIP(hipMemcpy(words, os[j].valid, sizeof words, hipMemcpyDeviceToHost));
      if (words[0] != s.entries) intact = false;
      s.flags = words[1];
      s.fix_levels = out.fix_levels[j];
      if ((int)out.window_sums[j].size() != P.Wr) throw Error(TNS_ERR_DEVICE, "accprobe: window sums of another plan");
      std::memcpy(s.sums, out.window_sums[j].data(), sizeof(G1Xyzz) * P.Wr);
      std::memcpy(s.result, &out.result[j], sizeof(G1Xyzz));
      if (s.buckets) TNS_HIP(hipMemcpy(s.buckets, out.buckets[j], sizeof(G1Xyzz) * P.nb, hipMemcpyDeviceToHost));
    }
    const TailGeom &t = out.tail;
    info[I_L0] = t.L0;
    info[I_L1] = t.L1;
    info[I_G1] = (int64_t)t.g1;
    info[I_G] = (int64_t)t.g;
    info[I_NBITS] = t.nbits;
    info[I_SPECS] = t.specs;
    info[I_CH] = t.CH;
    info[I_NCH] = (int64_t)t.nch;
    info[I_TREE] = t.tree;
    info[I_LG0] = t.lg0;
    info[I_WEIGHT] = t.weight;
    info[I_SUM_N] = (int64_t)t.sum_n;
    info[I_WR] = P.Wr;
    info[I_HALF] = (int64_t)P.half;
    info[I_NB] = (int64_t)P.nb;
    info[I_INPUTS_INTACT] = intact;
    static_assert(XW == 32, "a G1Xyzz is 32 words");
    TNS_HIP(hipDeviceSynchronize());  // (the uploads are freed on return: nothing may still read them)
    TNS_LAUNCH_CHECK();
    return TNS_OK;
  });
}

}  // extern "C"
