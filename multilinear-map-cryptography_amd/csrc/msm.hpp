// msm.hpp -- the multi-scalar multiplication (msm.hip) and its bucket sort (bucket_sort.hip): the
// per-stream lane with its named device workspaces and host readbacks, the fixed-base window
// table, how an MSM's scalars are described, and the two modules' entry points.  The window plan
// and the sort's geometry are decided in msm_plan.hpp.
//
// An MSM's scalars have three descriptions:
//  * MsmArgs: the caller of msm_pair_dev (kzg.hip, kzg_verify.hip) fills it -- one whole MSM;
//  * ScalarSource (MsmArgs::src): the same caller fills it -- when and in which form the scalars arrive;
//  * SortInput: msm.hip's msm_prepare_scalars fills it from the two -- what the sort's pass 1 reads.
#pragma once
#include <functional>
#include <memory>
#include <vector>

#include "bn254.hpp"
#include "hip_util.hpp"
#include "msm_batch_plan.hpp"
#include "msm_plan.hpp"

namespace tns {

struct Ctx;
struct Srs;
struct MsmLane;

// Window-shifted copies of a fixed point set for the shared-bucket MSM (msm.hip):
// table[j n + i] = 2^(c j) P_i, j < W.
struct FixedBase {
  DevBuf table;
  size_t n = 0;
  int c = 0, W = 0;
};

// ---------------------------------------------------------------- bucket_sort.hip
// the MSM's digit entries grouped by bucket (bucket k = [bstart[k], bstart[k+1]))
struct BucketOrder {
  uint32_t *keys, *vals, *bstart;  // keys == nullptr: packed tail, the runs come from bstart alone
  int ks;          // bucket = key >> ks
  size_t entries;  // sorted entries (non-zero digits) when read back, else SIZE_MAX
};
// What the bucket sort's digit pass reads: canonical scalars, Montgomery scalars (converted in
// the pass: no canonical copy is written), or raw u64 values (trace addresses, lookup indices:
// 8 bytes a scalar instead of 32; entries [0, n_u64), zero above).
struct SortInput {
  const Fr *fr = nullptr;
  bool mont = false;
  const uint64_t *u64 = nullptr;
  size_t n_u64 = 0;
  // set: pass 1's tile histograms are already in the lane's count buffer (SortWs::counts ==
  // precounted), computed for the plan `pre` over these n scalars (quotient2_count_dev: the
  // opening quotients' kernel counts their digits as it writes them); another plan recounts
  const uint32_t *precounted = nullptr;
  WindowPlan pre;
  // set (with precounted, Montgomery scalars): the count kernel also wrote each scalar's canonical
  // low 64 bits here; when the bit length shows the scalars fit 64 bits the sort reads these
  // (8 bytes a scalar, no Montgomery reduction) instead of the 32-byte scalars
  const uint64_t *low64 = nullptr;
};
// A lane's bucket-sort workspaces.  Every one belongs to the sort alone; all are written and read
// on the lane's stream by one sort at a time (a BucketSortJob holds pointers into them from
// bucket_sort_begin to bucket_sort_finish, and the MSM reads the order until its accumulation is
// queued: the lane runs no second sort before that).
struct SortWs {
  DevBuf keys[2], vals[2];  // the entries, ping and pong (E = W n words each)
  DevBuf seg[2];            // segment starts, ping and pong; the last one becomes the bucket starts
  DevBuf scan;              // exclusive_scan's block sums
  // pass histograms and their scan.  quotient2_count_dev and bucket_sort_precount_bits fill
  // `counts` ahead of the sort, which keeps them when SortInput::precounted is this very buffer
  DevBuf counts, offs;
  DevBuf tiles;             // per segment: tile counts | tile bases (one allocation, split at begin)
  DevBuf desc;              // tile descriptors
  DevBuf mtiles;            // the last pass's multi-tile segments: counts | bases (one allocation)
  DevBuf low64;             // the scalars' canonical low words (bucket_sort_precount_bits)
};
// A sort in flight: bucket_sort_begin (pass 1), bucket_sort_passes (the passes up to the last
// pass's tile-total readback), bucket_sort_finish (waits for that readback, queues the rest);
// all but the wait are queued on the lane without blocking the host.
struct BucketSortJob {
  MsmLane *ln = nullptr;
  SortGeom g;
  // what changes while the sort runs: the pass p in flight with its bins, shift and tile, the
  // segments S before it, and which of the ping / pong buffers holds them (cur)
  size_t S = 0;
  int cur = 0, p = 0, nb = 0, shift = 0, tile = 0;
  bool pending = false;            // the last pass waits for its tile totals' readback
  const void *readback = nullptr;  // the last pass's tile totals once read back (host memory)
  uint32_t *K[2] = {nullptr, nullptr}, *V[2] = {nullptr, nullptr}, *seg[2] = {nullptr, nullptr};
  uint32_t *counts = nullptr, *offs = nullptr, *tcount = nullptr, *tbase = nullptr, *desc = nullptr;
  uint32_t *mcount = nullptr, *mbase = nullptr;
  uint32_t *valid = nullptr;  // device: the entry count
};
void bucket_sort_begin(MsmLane &ln, const SortInput &in, size_t n, const WindowPlan &plan, uint32_t *valid,
                       BucketSortJob &J);
void bucket_sort_passes(BucketSortJob &J);
void bucket_sort_pass_rest(BucketSortJob &J, bool readback);
BucketOrder bucket_sort_finish(BucketSortJob &J);
// The two opening MSMs' scalars q_k,i = (v_k - y_k,i) inv_i (canonical: the inverses are) with their
// bit lengths, as lagrange_quotient_finish2_dev, AND pass 1's tile histograms of both sorts for the
// shared-table plan straight into lanes[0] / lanes[1]'s count buffers: the sorts skip their
// count kernels (one read of both quotient vectors less).  false (nothing queued): no fused kernel
// for the plan -- the caller runs the plain quotient kernel.
bool quotient2_count_dev(Ctx *c, const Fr *y0, const Fr *y1, size_t n, const Fr &v0, const Fr &v1, const Fr *inv,
                         Fr *q0, Fr *q1, unsigned *bits, const WindowPlan &plan, const uint32_t *counts_out[2]);
// n Montgomery scalars' largest bit length (into *bits, zeroed by the caller) together with pass 1's
// histograms for `plan` in the lane's count buffer; `in` then carries them as precounted.  false
// (nothing queued): no compile-time pass-1 shape for it.
bool bucket_sort_precount_bits(MsmLane &ln, const Fr *scalars, size_t n, const WindowPlan &plan, unsigned *bits,
                               SortInput &in, bool want_low64);
// What the sort reads once the scalars' bit length is known: scalars that fit 64 bits are read
// from their canonical low words where pass 1's precount wrote them (SortInput::low64)
inline SortInput sort_input_for_bits(SortInput in, size_t n, unsigned bits) {
  if (in.low64 && bits <= 64) in.u64 = in.low64, in.n_u64 = n, in.fr = nullptr, in.mont = false;
  return in;
}

// ---------------------------------------------------------------- msm.hip
// A lane's MSM workspaces beside the sort's: written on the lane's stream (the accumulation of a
// pair on Ctx::acc, ordered against the lane by events) by one MSM at a time; msm.hip's MsmJob
// holds the pointers from the launch to msm_complete, before which the lane starts no other MSM.
struct MsmWs {
  // two words, used one after the other by the same MSM: [0] the scalars' bit length, which the
  // host has read back (bits_result) before it queues the sort; then the sort's entry count with,
  // in [1], the accumulation's flags (a run crosses a chunk, a chunk group lies in one bucket)
  DevBuf words;
  DevBuf buckets;     // the bucket sums (a pair's two-set tail: both MSMs' buckets, adjoining, in lane 0's)
  DevBuf head_tail;   // per accumulation chunk: its first and last partial runs
  DevBuf chunk_bounds;  // per accumulation chunk: its first and last bucket
  DevBuf fix;         // heavy-bucket level sums
  DevBuf level_sums;  // the reduction's group sums T | S (| the second level's) in one allocation
  DevBuf parts;       // the masked sums' chunk parts | their summing scratch | the per-set sums
  DevBuf tiny_out;    // the n <= 64 path's one point
};
// One stream's MSM workspaces (msm.hip): two lanes let two independent MSMs of a proof
// (the two commitments, the two opening quotients) overlap on the device.
struct MsmLane {
  hipStream_t stream = nullptr;
  SortWs sort;
  MsmWs msm;
  // the lane's host readbacks without a stream synchronize: a one-block kernel copies the words
  // into this fine-grained host buffer and then sets the slot's flag, which the host polls
  // (lane_publish / lane_wait, msm.hip).  Slots: 0 scalar bit length, 1 the sort's last-pass
  // tile totals, 2 the MSM's per-set sums
  MappedHostBuf mapped;
  uint32_t pub_seq = 0;
  // the window plan this lane's last MSM of Montgomery scalars took, and its n: the next
  // such MSM of n scalars counts pass 1 for it while it computes the scalars' bit length, and the
  // sort uses those counts when the bit length confirms the plan (bucket_sort_precount_bits)
  struct PlanHint {
    size_t n = 0;
    WindowPlan plan;
  } hint;
  uint32_t slot_seq[3] = {0, 0, 0};
};
// readbacks through MsmLane::mapped: parts (device pointer, bytes; bytes % 4 == 0) are
// copied back to back into the slot's data; lane_wait returns it once the flag shows the publish
constexpr int LANE_SLOT_BITS = 0, LANE_SLOT_SORT = 1, LANE_SLOT_SUMS = 2;
void lane_publish(MsmLane &ln, int slot, int n, const void *const *src, const size_t *bytes);
const void *lane_wait(MsmLane &ln, int slot);
// for kernels that publish themselves: the slot's data and flag (device views) and its new seq
void lane_publish_slot(MsmLane &ln, int slot, uint32_t **data, uint32_t **flag, uint32_t *seq);

// (fb: optional window table of `points`, enabling the shared-bucket layout)
// fb_off: the points are entries [fb_off, fb_off + n) of the set fb was built for
G1Xyzz msm_dev(Ctx *c, const G1Affine *points, const Fr *scalars, size_t n, const FixedBase *fb = nullptr,
               size_t fb_off = 0);
// An MSM from a given bucket order: the accumulation with its fix-up, the bucket reduction and the
// host finish, without the scalar prep and the sort (tests/device/accprobe.hip hands it orders no
// affordable scalar vector produces).  One set, or two of the same shared-layout plan whose tails
// run as one two-set launch sequence, as a pair of table-plan openings.
struct OrderedSet {
  BucketOrder order;       // device; keys optional (with ks), entries unused
  uint32_t *valid;         // device, two words as the sort leaves them: [0] the entries, [1] = 0
  const G1Affine *points;  // what the values index
  int acc_k;               // entries per accumulation chunk
  size_t nchunks;          // acc_k nchunks >= the entries (chunks past them are skipped)
};
struct OrderedMsm {
  G1Xyzz result[2];
  std::vector<G1Xyzz> window_sums[2];  // per set, before Horner: P.Wr points
  G1Xyzz *buckets[2];                  // device: P.nb buckets after the fix-up, lazy domain
  TailGeom tail;                       // the reduction's geometry as run
  int fix_levels[2];                   // fix levels built per set
};
void msm_from_order_dev(Ctx *c, const MsmPlan &P, const OrderedSet *sets, int nj, OrderedMsm &out);
// how the scalars of one MSM of a pair get ready and in which form the sort reads them
struct ScalarSource {
  // enqueued on the lane's stream before anything else of this MSM: produces the scalars
  // (and canon / canon_bits) without holding up the other lane
  std::function<void(hipStream_t)> prep;
  // the scalars are still arriving (a host upload in flight; prep waits for it): msm_pair_dev
  // queues the other MSM whole before this one's prep
  bool late = false;
  // late and chunks > 1: the scalars arrive in `chunks` node ranges, chunk k = scalars
  // [chunk_off[k], chunk_off[k + 1]), ready once chunk_prep(k, stream) returns; msm_pair_dev sums
  // one MSM per chunk as each lands (table plans use the window table at the chunk's offset), so
  // only the last chunk's MSM follows the upload
  int chunks = 0;
  std::vector<size_t> chunk_off;  // chunks + 1 offsets, increasing, chunk_off[chunks] = n
  std::function<void(int, hipStream_t)> chunk_prep;
  // set: the scalars' largest bit length is at this device address and the sort reads
  // canonical scalars -- `canon` if set (then `scalars` stay Montgomery, for the tiny path),
  // else `scalars` themselves (n > 64 only: the tiny path reads Montgomery scalars)
  const Fr *canon = nullptr;
  const unsigned *canon_bits = nullptr;
  // set (with canon_bits): the sort reads these raw u64 values (entries [0, n_u64)) instead
  const uint64_t *u64 = nullptr;
  size_t n_u64 = 0;
};
struct MsmArgs {
  const G1Affine *points;
  const Fr *scalars;
  size_t n;
  const FixedBase *fb;
  size_t fb_off = 0;  // the points are entries [fb_off, fb_off + n) of the set fb was built for
  // set (with src.canon_bits, canonical scalars): pass 1's histograms are precounted for the plan
  // `pre` (SortInput::precounted)
  const uint32_t *precounted = nullptr;
  WindowPlan pre;
  // > 0: plan the MSM for scalars of this bit length without reading src.canon_bits back (the opening
  // quotients: full width -- the table plan's extra windows of a narrower quotient carry no digits,
  // so the entries are the same); the sort can be queued right behind the kernel writing the scalars
  int plan_bits = 0;
  ScalarSource src;
};
// two independent MSMs overlapped on the context's two lanes (inputs ready on c->stream)
void msm_pair_dev(Ctx *c, const MsmArgs &a, const MsmArgs &b, G1Xyzz out[2]);
// A batch of `rows` MSMs over the same n points (msm_batch_plan.hpp), scalars rows x n Montgomery
// forms on the device, all on lane 0 (= the context stream):
//  * msm_batch_bits_dev: the largest bit length of all `total` scalars (one pass, one host wait);
//  * msm_batch_groups_dev: the batched route of plan B (plan_batch with those bits) -- out[b], rows
//    affine points on the device, = sum_i scalars[b n + i] points[i]; synchronises before it returns.
// rep (optional): what the last group took.
struct BatchReport {
  int route = 0, c = 0, W = 0, npass = 0;
  size_t groups = 0, group_rows = 0;
};
unsigned msm_batch_bits_dev(Ctx *c, const Fr *scalars, size_t total);
void msm_batch_groups_dev(Ctx *c, const G1Affine *points, const Fr *scalars, size_t n, size_t rows, unsigned bits,
                          const BatchPlan &B, G1Affine *out, BatchReport *rep = nullptr);
std::unique_ptr<FixedBase> fixed_base_build_dev(Ctx *c, const G1Affine *points, size_t n);
// the same, or nullptr when the table does not fit in device memory (TNS_ERR_OOM)
std::unique_ptr<FixedBase> fixed_base_try_build(Ctx *c, const G1Affine *points, size_t n);
// the SRS's window table, built on first use by an MSM of >= 2^16 points (nullptr below)
const FixedBase *srs_fixed_base(Ctx *c, const Srs &srs, size_t n);

// ---------------------------------------------------------------- device helpers of both
// bit length of a canonical field element (0 for zero)
__device__ __forceinline__ unsigned fr_bit_length(const Fr &k) {
  unsigned b = 0;
#pragma unroll
  for (int l = 0; l < 8; l++)
    if (k.v[l]) b = 32 * l + 32 - __builtin_clz(k.v[l]);
  return b;
}
// max over the block of (b0, b1) -> one atomicMax per block and target (blockDim.x a multiple
// of 64, at most 1024; every thread of the block calls it).  A per-wave atomic on one address
// serialises in L2: 8 K of them were ~80 us of a 2^20-scalar bit-length pass.
__device__ __forceinline__ void block_atomic_max2(unsigned b0, unsigned b1, unsigned *dst0, unsigned *dst1) {
  __shared__ unsigned wmax[2][16];
  for (int o = 32; o > 0; o >>= 1) {
    b0 = max(b0, (unsigned)__shfl_xor(b0, o));
    b1 = max(b1, (unsigned)__shfl_xor(b1, o));
  }
  const int w = (int)(threadIdx.x >> 6);
  if ((threadIdx.x & 63) == 0) {
    wmax[0][w] = b0;
    wmax[1][w] = b1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < (int)(blockDim.x >> 6); i++) {
      b0 = max(b0, wmax[0][i]);
      b1 = max(b1, wmax[1][i]);
    }
    if (b0) atomicMax(dst0, b0);
    if (b1 && dst1) atomicMax(dst1, b1);
  }
}

}  // namespace tns
