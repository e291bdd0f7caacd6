// msm.hip -- BN254 G1 multi-scalar multiplication (Pippenger, signed windows).
//
// Replaces KZGCommitment::commit's per-term scalar multiplications
// (src/commitments.rs:173-177): C = sum_i c_i * g1_powers[i].  The group element
// is unique, so any correct algorithm reproduces it exactly.
//
// Two bucket layouts share one pipeline:
//  * per-window: W windows of c bits, W * 2^(c-1) buckets, windows combined by Horner;
//  * shared (fixed bases: the SRS and its Lagrange bases never change): a precomputed
//    table T[j n + i] = 2^(c j) P_i turns window j's digit of scalar i into a digit of
//    point T[j n + i], so all windows land in ONE set of 2^(c-1) buckets -- the bucket
//    reduction runs once instead of W times, no Horner doublings remain, and a wider c
//    (fewer windows, fewer bucket additions) becomes affordable.
//
// Pipeline (per MSM lane stream):
//  0. k_scalar_bits: bit length of the largest scalar -> windows above it are skipped
//     (trace commitments -- addresses, small values, flags -- are narrow).
//  1.-3. the bucket order (bucket_sort.hip): the signed c-bit digits are computed inside the
//     first pass of a hand-written MSD counting sort (no digit array, zero digits never enter it);
//     its last pass writes the point indices | sign<<31 alone and the bucket starts.
//  4. k_accumulate: load-balanced -- each thread owns acc_k consecutive sorted entries
//     and XYZZ-madds the (possibly negated) affine points run by run; runs that cross a
//     chunk boundary leave a head/tail partial; k_bucket_fixup completes those buckets (heavy buckets'
//     chunk heads through FIX_FAN-ary level sums, so no thread walks a long run).
//  5. k_reduce_level: per group of L buckets of a window, running sums
//     T_g = sum_{j in g} (j - a + 1) B_j and S_g = sum_{j in g} B_j; then
//     sum_j (j+1) B_j = sum_g T_g + L sum_g g S_g, and sum_g g S_g = sum_b 2^b M_b with
//     M_b the sum of the S_g whose index has bit b set: k_masked_sums + chunked sums
//     (short dependency chains -- single-thread point-add chains are the slow part).
//  6. host: per-window Horner (per-window layout) or nothing (shared layout).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <cstdlib>
#include <vector>

#include "ctx.hpp"
#include "srs.hpp"

namespace tns {

// (RED_L, FIX_FAN, FIX_LEVELS, FIX_WAVE_SPAN and the tail's geometry: msm_plan.hpp)

// *bits = max over i of bitlen(canonical scalar_i); canon (optional) = the canonical scalars
// (the bucket sort canonicalises Montgomery scalars itself, so the MSMs pass none)
__global__ void __launch_bounds__(256) k_scalar_bits(const Fr *__restrict__ scalars, size_t n,
                                                     unsigned *__restrict__ bits, Fr *__restrict__ canon) {
  unsigned b = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    Fr k = from_mont(scalars[i]);
    if (canon) canon[i] = k;
    b = max(b, fr_bit_length(k));
  }
  block_atomic_max2(b, 0u, bits, nullptr);
}

// the accumulation's point gather
__device__ __forceinline__ G1Affine load_point(const G1Affine *__restrict__ pts, uint32_t i) { return pts[i]; }

struct HeadTail {
  G1Xyzz head, tail;
};

// the bucket holding sorted entry p < valid: the largest k with bstart[k] <= p (bstart is
// non-decreasing, bstart[0] = 0, bstart[nb] = valid; empty buckets repeat their successor's start)
__device__ __forceinline__ uint32_t bucket_of(const uint32_t *__restrict__ bstart, size_t nb, size_t p) {
  size_t lo = 0, hi = nb;
  while (hi - lo > 1) {
    const size_t mid = (lo + hi) >> 1;
    if (bstart[mid] <= p) lo = mid;
    else hi = mid;
  }
  return (uint32_t)lo;
}

// keys == nullptr (values-only sort tail): a chunk finds its first bucket by a binary search of the
// bucket starts and every later run boundary from the next start -- no key per entry.
// KEYS (a template parameter, so the default values-only sort's variant carries none of the key
// path's registers): the sort left a key per entry (else the runs come from the bucket starts)
template <bool KEYS>
__global__ void __launch_bounds__(256) k_accumulate(const uint32_t *__restrict__ keys,
                                                    const uint32_t *__restrict__ vals,
                                                    const uint32_t *__restrict__ valid_p,
                                                    const G1Affine *__restrict__ pts,
                                                    G1Xyzz *__restrict__ buckets,
                                                    HeadTail *__restrict__ ht, size_t nchunks, int ks,
                                                    int acc_k, const uint32_t *__restrict__ bstart, size_t nb,
                                                    uint2 *__restrict__ cbk, uint32_t *__restrict__ spans) {
  // entry positions are 32-bit (a sort holds < 2^31 entries, msm_launch_sort): one VGPR each
  const uint32_t valid = *valid_p;
  bool crossed = false;  // this thread left a head or tail partial (k_fix_level / k_bucket_fixup work)
  bool grouped = false;  // ... and a level-1 group of 8 chunks lies inside one bucket (k_fix_level's)
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < nchunks;
       t += (size_t)gridDim.x * blockDim.x) {
    const uint32_t a = (uint32_t)t * (uint32_t)acc_k;
    uint32_t fb = 0xffffffffu, lb = 0xfffffffeu;  // the chunk's first / last bucket (none past valid)
    if (a < valid) {
    const uint32_t b = a + acc_k < valid ? a + acc_k : valid;
    // a run is a head (it began before this chunk) iff it is the chunk's first run and entry
    // a - 1 has its bucket, a tail (it goes on after the chunk) iff it is the last run and entry
    // b has its bucket: two key loads per chunk instead of the run's bounds at every flush.
    // Flushed sums stay in the lazy domain [0, 2M): the fixup and the reduction add them lazily.
    uint32_t cur, after;
    bool head_run;
    uint32_t nxt = 0;  // (no keys) the start of the bucket after `cur`
    if (KEYS) {
      cur = keys[a] >> ks;
      head_run = a > 0 && (keys[a - 1] >> ks) == cur;
      after = b < valid ? keys[b] >> ks : 0xffffffffu;
    } else {
      cur = bucket_of(bstart, nb, a);
      head_run = bstart[cur] < a;
      nxt = bstart[cur + 1];
      after = 0xffffffffu;
    }
    bool first = true;
    const uint32_t first_bucket = cur;
    G1Xyzz acc = G1Xyzz::inf();
    for (uint32_t p = a;; p++) {
      const bool brk = KEYS ? p >= b || (keys[p] >> ks) != cur : p >= b || p >= nxt;
      if (brk) {  // flush the run of bucket `cur`
        const bool tail = KEYS ? after == cur : nxt > b;
        if (first && head_run) ht[t].head = acc;
        else if (p >= b && tail) ht[t].tail = acc;
        else buckets[cur] = acc;
        crossed |= (first && head_run) || (p >= b && tail);
        if (p >= b) {
          cbk[t] = make_uint2(first_bucket, cur);  // the buckets of entries a and b - 1 (k_fix_level)
          fb = first_bucket;
          lb = cur;
          break;
        }
        first = false;
        if (KEYS) {
          cur = keys[p] >> ks;
        } else {
          do {  // skip empty buckets
            cur++;
            nxt = bstart[cur + 1];
          } while (nxt <= p);
        }
        acc = G1Xyzz::inf();
      }
      // (gathering entry p + 1 ahead of this addition measured no faster: 39.48 vs 39.46 ms of
      // accumulation per C4 step -- three waves per SIMD hide the gather)
      const uint32_t v = vals[p];
      G1Affine q = load_point(pts, v & 0x7fffffffu);
      // -y = M - y (y canonical); the identity (0, 0) keeps y = 0
      const Fq ny = const_minus_dev<FqCfg, false>(q.y);
      const bool negy = (v >> 31) && !q.y.is_zero();
#pragma unroll
      for (int l = 0; l < 8; l++) q.y.v[l] = negy ? ny.v[l] : q.y.v[l];
      acc = xyzz_madd_lazy(acc, q);
    }
    }
    // k_fix_level's level-1 test for the group of chunks t .. t + 7 (t a multiple of 8: lane 8k):
    // the first chunk's first bucket is the last chunk's last (every lane of the wave shuffles)
    const uint32_t lb7 = __shfl_down(lb, 7, FIX_FAN);
    grouped |= (threadIdx.x & (FIX_FAN - 1)) == 0 && t + FIX_FAN - 1 < nchunks && fb == lb7;
  }
  // two flags per MSM: no run crossed a chunk (the 22-bit address commitment at C4: every bucket's
  // four entries inside one chunk) -> nothing to fix up; no 8-chunk group inside one bucket (any
  // uniform scalars: the openings, C2) -> no fix level has a group to sum
  const uint32_t f = (__any(crossed) ? 1u : 0u) | (__any(grouped) ? 2u : 0u);  // (every lane votes)
  if (f && (threadIdx.x & 63) == 0) atomicOr(spans, f);
}

// Heavy buckets (skewed scalars: repeated values, small ranges) span many chunks; their
// chunk heads are summed through a FIX_FAN-ary hierarchy so no thread walks a long run.
// Level l >= 1, group g covers chunks [g F^l, (g+1) F^l) (F = FIX_FAN); its sum is formed only when
// every sorted entry of those chunks has one key (then every head in it is a full-chunk
// sum of that bucket); other groups are never read.  (n and len: fix_level_sizes, msm_plan.hpp)
struct FixLevels {
  G1Xyzz *lv[FIX_LEVELS + 1];  // lv[l] for l >= 1 (the level-0 heads live in ht)
  size_t len[FIX_LEVELS + 1];
  int n;                        // levels built (0: none)
};

// FIX_FAN consecutive lanes per group: lane j loads item j and the group's sum is an xor butterfly
// over those lanes (3 dependent additions instead of one thread's chain of 7: the narrow value
// commitment's heavy buckets fill thousands of groups and this level ran at half a wave per SIMD)
static_assert(FIX_FAN == 8, "k_fix_level's butterfly assumes 8 lanes per group");
// one MSM's level-l groups (blockIdx.y picks the MSM: a pair's two tails run as one launch)
struct FixLevelSet {
  const uint32_t *valid;
  const HeadTail *ht;
  const G1Xyzz *below;
  G1Xyzz *out;
  const uint2 *cbk;
  size_t n_groups;  // 0: this MSM has no level l
  int acc_k;
};
struct FixLevelArgs {
  FixLevelSet s[2];
};
__global__ void __launch_bounds__(256) k_fix_level(FixLevelArgs A, int level) {
  const FixLevelSet &S = A.s[blockIdx.y];
  const size_t n_groups = S.n_groups;
  // (valid[1] bit 1: some 8-chunk group lies inside one bucket, k_accumulate; a group of any
  // higher level is made of such groups)
  if (!n_groups || !(S.valid[1] & 2u)) return;
  const size_t valid = *S.valid;
  const int acc_k = S.acc_k;
  const int j = threadIdx.x & (FIX_FAN - 1);
  const size_t stride = (size_t)gridDim.x * blockDim.x / FIX_FAN;
  // group-uniform trip count (blockDim.x is a multiple of FIX_FAN): the 8 lanes of a group stay together
  for (size_t g = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) / FIX_FAN; g < n_groups; g += stride) {
    size_t span = (size_t)acc_k;
    for (int l = 0; l < level; l++) span *= FIX_FAN;
    const size_t a = g * span, b = a + span;  // entries covered
    // every entry of [a, b) in one bucket: the bucket of entry a (that chunk's first) is the bucket
    // of entry b - 1 (the last chunk's last), as k_accumulate recorded them
    const bool uniform = b <= valid && S.cbk[a / acc_k].x == S.cbk[(b - 1) / acc_k].y;
    // a wave whose 8 groups all span several buckets has nothing to sum (those sums are never
    // read): skip its butterfly -- most of a narrow commitment's groups (the 22-bit address MSM:
    // ~4 entries a bucket) are such
    if (!__any(uniform)) continue;
    G1Xyzz acc = G1Xyzz::inf();
    if (uniform) acc = level == 1 ? S.ht[g * FIX_FAN + j].head : S.below[g * FIX_FAN + j];
    for (int off = FIX_FAN / 2; off > 0; off >>= 1) {  // every lane of the wave takes part
      G1Xyzz o;
      const uint32_t *pa = reinterpret_cast<const uint32_t *>(&acc);
      uint32_t *po = reinterpret_cast<uint32_t *>(&o);
#pragma unroll
      for (int q = 0; q < (int)(sizeof(G1Xyzz) / 4); q++) po[q] = __shfl_xor(pa[q], off);
      if (uniform) acc = xyzz_add_lazy(acc, o);
    }
    if (uniform && j == 0) S.out[g] = acc;
  }
}

// bucket values: empty -> identity; a run inside one chunk is already in buckets[bk];
// a run across chunks tf < tl -> tail(tf) + heads of (tf, tl) (via the levels) + head(tl)
// Runs over more than FIX_WAVE_SPAN chunks are summed by the whole wave that meets them in
// k_bucket_fixup: a single thread's chain over their ~50+ items would be the tail of the whole
// MSM (a skewed input puts every entry in one bucket: Shout's identity lookups, 5.8 instead of
// 6.4 ms at 2^20).  Shorter runs stay one thread each -- thousands of moderately heavy buckets
// (the top window's narrow digits crowd the low ones) are cheaper so than as thousands of
// mostly idle wave passes next to the other lane's accumulation.  (FIX_WAVE_SPAN: msm_plan.hpp)

// the items of a run across chunks tf < tl, in order: tail(tf), head(tl), then the inner heads
// (tf, tl), peeled to FIX_FAN-aligned ranges and climbing a level whenever both ends are aligned
struct FixItems {
  size_t tf, tl, lo, hi;
  int l, k;  // level, items produced so far
  __device__ FixItems(size_t f, size_t t) : tf(f), tl(t), lo(f + 1), hi(t), l(0), k(0) {}
  __device__ const G1Xyzz *next(const HeadTail *ht, const FixLevels &F) {
    if (k == 0) {
      k++;
      return &ht[tf].tail;
    }
    if (k == 1) {
      k++;
      return &ht[tl].head;
    }
    for (;;) {
      if (lo >= hi) return nullptr;
      const bool climb = l < F.n && hi - lo >= 2 * FIX_FAN;
      if (climb && lo % FIX_FAN == 0 && hi % FIX_FAN == 0) {
        lo /= FIX_FAN;
        hi /= FIX_FAN;
        l++;
        continue;
      }
      size_t i;
      if (!climb || lo % FIX_FAN) i = lo++;
      else i = --hi;  // lo aligned, hi not
      k++;
      return l == 0 ? &ht[i].head : &F.lv[l][i];
    }
  }
};

// the sum over the wave of every lane's acc, in every lane (xor butterfly: 6 dependent additions)
__device__ __forceinline__ G1Xyzz wave_sum_xyzz(G1Xyzz acc) {
  for (int off = 32; off > 0; off >>= 1) {
    G1Xyzz o;
    const uint32_t *pa = reinterpret_cast<const uint32_t *>(&acc);
    uint32_t *po = reinterpret_cast<uint32_t *>(&o);
#pragma unroll
    for (int q = 0; q < (int)(sizeof(G1Xyzz) / 4); q++) po[q] = __shfl_xor(pa[q], off);
    acc = xyzz_add_lazy(acc, o);
  }
  return acc;
}

// one MSM's buckets (blockIdx.y picks the MSM: a pair's two tails run as one launch)
struct FixupSet {
  const uint32_t *start, *end;
  const uint32_t *valid;  // [1]: some run crossed a chunk (else only the empty buckets need writing)
  const HeadTail *ht;
  FixLevels F;
  G1Xyzz *buckets;
  size_t nb;
  int acc_k;
};
struct FixupArgs {
  FixupSet s[2];
};
__global__ void __launch_bounds__(256) k_bucket_fixup(FixupArgs A) {
  const FixupSet &S = A.s[blockIdx.y];
  const uint32_t *__restrict__ start = S.start;
  const uint32_t *__restrict__ end = S.end;
  const HeadTail *__restrict__ ht = S.ht;
  const FixLevels &F = S.F;
  G1Xyzz *__restrict__ buckets = S.buckets;
  const size_t nb = S.nb;
  const int acc_k = S.acc_k;
  const int lane = threadIdx.x & 63;
  if (!S.valid[1]) {  // every run inside one chunk: k_accumulate wrote every non-empty bucket
    for (size_t bk = blockIdx.x * (size_t)blockDim.x + threadIdx.x; bk < nb; bk += (size_t)gridDim.x * blockDim.x)
      if (start[bk] == end[bk]) buckets[bk] = G1Xyzz::inf();
    return;
  }
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  // wave-uniform trip count: a wave meets its lanes' heavy runs together
  for (size_t base = blockIdx.x * (size_t)blockDim.x + (threadIdx.x & ~63u); base < nb; base += stride) {
    const size_t bk = base + lane;
    uint32_t s = 0, e = 0;
    if (bk < nb) {
      s = start[bk];
      e = end[bk];
    }
    const size_t tf = s / acc_k, tl = e > s ? (e - 1) / acc_k : tf;
    const bool heavy = bk < nb && tl - tf > FIX_WAVE_SPAN;
    // the wave's heavy runs, one at a time: lane j adds items j, j + 64, ..., then a butterfly
    for (uint64_t hm = __ballot(heavy); hm; hm &= hm - 1) {
      const int src = __ffsll((unsigned long long)hm) - 1;
      const size_t hf = __shfl((unsigned)tf, src), hl = __shfl((unsigned)tl, src);
      FixItems it(hf, hl);
      G1Xyzz acc = G1Xyzz::inf();
      const G1Xyzz *mine = nullptr;
      for (int k = 0;; k++) {  // the item sequence is the same in every lane: uniform control flow
        const G1Xyzz *item = it.next(ht, F);
        if (item && (k & 63) == lane) mine = item;
        if (!item || (k & 63) == 63) {  // a round of 64 items: every lane adds its own at once
          if (mine) acc = xyzz_add_lazy(acc, *mine);
          mine = nullptr;
          if (!item) break;
        }
      }
      acc = wave_sum_xyzz(acc);
      if (lane == src) buckets[bk] = acc;
    }
    if (bk >= nb || heavy) continue;
    if (s == e) {
      buckets[bk] = G1Xyzz::inf();
      continue;
    }
    if (tf == tl) continue;
    // one addition site: the items are head(tl), then the inner heads (tf, tl), peeled
    // to FIX_FAN-aligned ranges and climbing a level whenever both ends are aligned
    G1Xyzz acc = ht[tf].tail;
    size_t lo = tf + 1, hi = tl;
    int l = 0;
    bool pending_head = true;
    for (;;) {
      const G1Xyzz *item;
      if (pending_head) {
        item = &ht[tl].head;
        pending_head = false;
      } else {
        if (lo >= hi) break;
        const bool climb = l < F.n && hi - lo >= 2 * FIX_FAN;
        if (climb && lo % FIX_FAN == 0 && hi % FIX_FAN == 0) {
          lo /= FIX_FAN;
          hi /= FIX_FAN;
          l++;
          continue;
        }
        size_t i;
        if (!climb || lo % FIX_FAN) i = lo++;
        else i = --hi;  // lo aligned, hi not
        item = l == 0 ? &ht[i].head : &F.lv[l][i];
      }
      acc = xyzz_add_lazy(acc, *item);
    }
    buckets[bk] = acc;
  }
}

// one level over X (sets x n): groups of L; T = sum (j - a + 1) X_j, S = sum X_j
__global__ void __launch_bounds__(64) k_reduce_level(const G1Xyzz *__restrict__ X, int sets, size_t n, int L,
                                                     G1Xyzz *__restrict__ T, G1Xyzz *__restrict__ S) {
  const size_t groups = n / L;
  for (size_t id = blockIdx.x * (size_t)blockDim.x + threadIdx.x; id < (size_t)sets * groups;
       id += (size_t)gridDim.x * blockDim.x) {
    const size_t r = id / groups, g = id % groups;
    const G1Xyzz *x = X + r * n + g * L;
    G1Xyzz run = G1Xyzz::inf(), acc = G1Xyzz::inf();
    for (int j = L - 1; j >= 0; j--) {
      run = xyzz_add_lazy(run, x[j]);
      acc = xyzz_add_lazy(acc, run);
    }
    T[id] = acc;
    S[id] = run;
  }
}

// second level over the first level's (T, S) (sets x g1, groups of L1): per group h
//   u_h = sum T_g,  S2_h = sum S_g,  W_h = sum_j j S_{h L1 + j}  (the running sum added BEFORE
//   each element: no negation), and V_h = u_h + 2^lg0 W_h (lg0 doublings: L0 = 2^lg0).
// Then sum_g T_g + L0 sum_g g S_g = sum_h V_h + L0 L1 sum_h h S2_h, so the masked sums run over
// g1 / L1 groups with weight L0 L1.  Short chains (3 L1 additions + lg0 doublings) instead of the
// masked sums' ~nbits/2-fold re-reading of every S_g: C2's masked sums took 0.32 of its 2.3 ms.
__global__ void __launch_bounds__(64) k_reduce_level2(const G1Xyzz *__restrict__ T, const G1Xyzz *__restrict__ S,
                                                      int sets, size_t g1, int L1, int lg0,
                                                      G1Xyzz *__restrict__ V, G1Xyzz *__restrict__ S2) {
  const size_t groups = g1 / L1;
  for (size_t id = blockIdx.x * (size_t)blockDim.x + threadIdx.x; id < (size_t)sets * groups;
       id += (size_t)gridDim.x * blockDim.x) {
    const size_t r = id / groups, h = id % groups;
    const size_t base = r * g1 + h * L1;
    G1Xyzz run = G1Xyzz::inf(), w = G1Xyzz::inf(), u = G1Xyzz::inf();
    for (int j = L1 - 1; j >= 0; j--) {
      w = xyzz_add_lazy(w, run);  // + sum_{k > j} S_k: S_k counted k times in the end
      run = xyzz_add_lazy(run, S[base + j]);
      u = xyzz_add_lazy(u, T[base + j]);
    }
    w = xyzz_canon(w);
    for (int q = 0; q < lg0; q++) w = xyzz_dbl(w);
    V[id] = xyzz_add_lazy(u, w);
    S2[id] = run;
  }
}

// parts[(r specs + s) nch + ch], nch = g / (2 CH) chunks of CH items per spec s of set r:
//   s < nbits: the groups gi with bit s set, enumerated directly (the k-th is k with a one
//   inserted at bit s: every lane of a wave adds, no masked-off lanes);
//   s == nbits, nbits + 1: T over the lower / upper half of the groups
// wave_tree (nch a multiple of 64): the wave's 64 chunk sums are added in registers and only
// parts[id / 64] is written -- the two 8-way k_sum_chunks passes after it (each a chain of 8
// additions at low occupancy) become one 6-step butterfly
__global__ void __launch_bounds__(64) k_masked_sums(const G1Xyzz *__restrict__ T, const G1Xyzz *__restrict__ S,
                                                    int sets, size_t g, int nbits, int CH,
                                                    G1Xyzz *__restrict__ parts, bool wave_tree) {
  const int specs = nbits + 2;
  const size_t nch = g / (2 * (size_t)CH);
  for (size_t id = blockIdx.x * (size_t)blockDim.x + threadIdx.x; id < (size_t)sets * specs * nch;
       id += (size_t)gridDim.x * blockDim.x) {
    const size_t r = id / (specs * nch), rem = id % (specs * nch);
    const int sp = (int)(rem / nch);
    const size_t ch = rem % nch;
    G1Xyzz acc = G1Xyzz::inf();
    if (sp >= nbits) {
      const G1Xyzz *src = T + r * g + (size_t)(sp - nbits) * (g / 2);
      for (size_t k = ch * CH; k < ch * CH + CH; k++) acc = xyzz_add_lazy(acc, src[k]);
    } else {
      const G1Xyzz *src = S + r * g;
      const size_t lo_mask = ((size_t)1 << sp) - 1;
      for (size_t k = ch * CH; k < ch * CH + CH; k++)
        acc = xyzz_add_lazy(acc, src[((k & ~lo_mask) << 1) | ((size_t)1 << sp) | (k & lo_mask)]);
    }
    if (wave_tree) {  // the id range is a multiple of 64: every lane of the wave is here
      acc = wave_sum_xyzz(acc);
      if ((threadIdx.x & 63) == 0) parts[id >> 6] = acc;
    } else {
      parts[id] = acc;
    }
  }
}

// out[t] = sum of in[t*chunk .. (t+1)*chunk)
__global__ void __launch_bounds__(64) k_sum_chunks(const G1Xyzz *__restrict__ in, size_t n_out, int chunk,
                                                   G1Xyzz *__restrict__ out) {
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < n_out; t += (size_t)gridDim.x * blockDim.x) {
    G1Xyzz acc = in[t * chunk];
    for (int i = 1; i < chunk; i++) acc = xyzz_add_lazy(acc, in[t * chunk + i]);
    out[t] = acc;
  }
}

// out[r] = sum of parts[r*groups .. (r+1)*groups), one block per set
__global__ void __launch_bounds__(256) k_set_sum(const G1Xyzz *__restrict__ parts, size_t groups,
                                                 G1Xyzz *__restrict__ out) {
  __shared__ G1Xyzz lds[256];
  const size_t r = blockIdx.x;
  G1Xyzz acc = G1Xyzz::inf();
  for (size_t g = threadIdx.x; g < groups; g += blockDim.x) acc = xyzz_add_lazy(acc, parts[r * groups + g]);
  lds[threadIdx.x] = acc;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] = xyzz_add_lazy(lds[threadIdx.x], lds[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[r] = xyzz_canon(lds[0]);  // the host reads canonical coordinates
}

// Naive path for tiny inputs: one thread per point, double-and-add, then a tree.
__global__ void __launch_bounds__(64) k_msm_tiny(const G1Affine *__restrict__ pts,
                                                 const Fr *__restrict__ scalars, int n,
                                                 G1Xyzz *__restrict__ out) {
  __shared__ G1Xyzz lds[64];
  G1Xyzz acc = G1Xyzz::inf();
  for (int i = threadIdx.x; i < n; i += 64) {
    Fr k = from_mont(scalars[i]);
    G1Xyzz r = G1Xyzz::inf();
    for (int b = 253; b >= 0; b--) {
      r = xyzz_dbl(r);
      if ((k.v[b >> 5] >> (b & 31)) & 1) r = xyzz_madd(r, pts[i]);
    }
    acc = xyzz_add(acc, r);
  }
  lds[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 32; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] = xyzz_add(lds[threadIdx.x], lds[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = lds[0];
}

// ---------------------------------------------------------------- fixed-base tables
__global__ void __launch_bounds__(256) k_affine_to_xyzz(const G1Affine *__restrict__ in, size_t n,
                                                        G1Xyzz *__restrict__ out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = xyzz_from_affine(in[i]);
}

__global__ void __launch_bounds__(256) k_dbl_times(G1Xyzz *__restrict__ x, size_t n, int times) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    G1Xyzz p = x[i];
    for (int k = 0; k < times; k++) p = xyzz_dbl(p);
    x[i] = p;
  }
}

std::unique_ptr<FixedBase> fixed_base_build_dev(Ctx *c, const G1Affine *points, size_t n) {
  auto fb = std::make_unique<FixedBase>();
  fb->n = n;
  fb->c = table_window(n);
  fb->W = windows_for(254, fb->c);
  G1Affine *T = (G1Affine *)fb->table.ensure(sizeof(G1Affine) * n * fb->W);
  TNS_HIP(hipMemcpyAsync(T, points, sizeof(G1Affine) * n, hipMemcpyDeviceToDevice, c->stream));
  const size_t slab = std::min(n, (size_t)1 << 22);
  DevBuf xb, pb;
  G1Xyzz *X = (G1Xyzz *)xb.ensure(sizeof(G1Xyzz) * slab);
  Fq *pre = (Fq *)pb.ensure(sizeof(Fq) * slab);
  for (size_t off = 0; off < n; off += slab) {
    const size_t m = std::min(slab, n - off);
    k_affine_to_xyzz<<<grid_for(m, 256), 256, 0, c->stream>>>(points + off, m, X);
    TNS_LAUNCH_CHECK();
    for (int j = 1; j < fb->W; j++) {
      k_dbl_times<<<grid_for(m, 256), 256, 0, c->stream>>>(X, m, fb->c);
      TNS_LAUNCH_CHECK();
      xyzz_to_affine_batch_dev(c, X, m, T + (size_t)j * n + off, pre);
    }
  }
  TNS_HIP(hipStreamSynchronize(c->stream));
  return fb;
}

// the window table if the device has room for it: on an allocation failure the MSMs over these
// points run without one (per-window buckets, same results) and nothing is cached
std::unique_ptr<FixedBase> fixed_base_try_build(Ctx *c, const G1Affine *points, size_t n) {
  try {
    return fixed_base_build_dev(c, points, n);
  } catch (const Error &e) {
    if (e.code != TNS_ERR_OOM) throw;
    (void)hipGetLastError();  // clear the failed allocation's sticky status
    return nullptr;
  }
}

const FixedBase *srs_fixed_base(Ctx *c, const Srs &srs, size_t n) {
  if (n < ((size_t)1 << 16) || !c->msm_tables) return nullptr;
  if (srs.held < n) return nullptr;  // a shard's table covers its held points (tns_msm_sharded)
  if (!srs.fb) srs.fb = fixed_base_try_build(c, srs.points.as<G1Affine>(), srs.held);
  return srs.fb.get();
}

// ---------------------------------------------------------------- driver
// sum over each set of the sets x n array X (device) -> out (sets, device)
static void sum_sets(hipStream_t st, G1Xyzz *X, int sets, size_t n, G1Xyzz *tmp, G1Xyzz *out) {
  G1Xyzz *src = X, *dst = tmp;
  while (sum_sets_splits(n)) {  // short chains: these passes are latency-bound
    const size_t n_out = (size_t)sets * (n / 8);
    k_sum_chunks<<<grid_for(n_out, 64, 1u << 30), 64, 0, st>>>(src, n_out, 8, dst);
    TNS_LAUNCH_CHECK();
    std::swap(src, dst);
    n /= 8;
  }
  k_set_sum<<<sets, 256, 0, st>>>(src, n, out);
  TNS_LAUNCH_CHECK();
}

// How far an MSM has got.  msm_launch_sort leaves Immediate (n == 0, all scalars zero: the result is
// known), Tiny (k_msm_tiny: one point in the lane's pinned buffer) or Pass1Queued; msm_sort_passes:
// -> PassesQueued (up to the last pass's readback); msm_finish_sort: -> Sorted (the bucket order exists).
enum class MsmStage { None, Immediate, Tiny, Pass1Queued, PassesQueued, Sorted };
// One MSM in flight on a lane: launched by msm_launch_sort, completed by msm_complete.
struct MsmJob {
  MsmLane *lane = nullptr;
  MsmStage stage = MsmStage::None;
  bool sorted() const { return stage == MsmStage::Sorted; }
  void expect(MsmStage s, const char *what) const { if (stage != s) throw Error(TNS_ERR_DEVICE, what); }
  MsmPlan P;
  int L0 = 0, nbits = 0, specs = 0;
  TailGeom tail;       // what msm_launch_tails ran with, and the fix levels it built
  int fix_levels = 0;
  BucketSortJob bs;
  hipEvent_t sorted_ev = nullptr;   // recorded on the lane once the bucket order exists
  std::unique_ptr<ProfScope> sort_prof;  // "msm_sort" timing from pass 1 to the last pass
  Ctx *ctx = nullptr;
  const G1Affine *points = nullptr;
  uint32_t *keys2 = nullptr, *vals2 = nullptr, *bstart = nullptr, *bend = nullptr, *valid = nullptr;
  int ks = 0, acc_k = 0;
  size_t nchunks = 0, n = 0;
  G1Xyzz *buckets = nullptr;  // set before the accumulation (a two-set tail: the pair's buckets adjoin)
  const HeadTail *ht = nullptr;  // the accumulation's per-chunk partials and bucket bounds (the fixup reads them)
  const uint2 *cbk = nullptr;
  // where msm_complete finds the per-set sums: the slot of res_lane (this lane, or the lane that ran
  // a two-set tail), set res_set of res_sets
  MsmLane *res_lane = nullptr;
  int res_set = 0, res_sets = 1;
  // a batch (msm_batch_groups_dev): the per-set sums stay on the device for k_batch_finish --
  // msm_launch_tails publishes nothing and leaves them here (P.Wr x specs canonical points)
  bool device_finish = false;
  const G1Xyzz *sums = nullptr;
};

// ---------------------------------------------------------------- lane readbacks
struct PubArgs {
  const uint32_t *src[4];
  uint32_t words[4];
  int n;
};
constexpr size_t LANE_MAPPED_DATA[3] = {256, 512, 1024};  // slot data offsets; flags at 64 * slot
constexpr size_t LANE_MAPPED_BYTES = 1024 + 65536;

__global__ void __launch_bounds__(256) k_lane_publish(PubArgs a, uint32_t *dst, uint32_t *flag, uint32_t seq) {
  uint32_t off = 0;
  for (int k = 0; k < a.n; k++) {
    for (uint32_t i = threadIdx.x; i < a.words[k]; i += blockDim.x) dst[off + i] = a.src[k][i];
    off += a.words[k];
  }
  __threadfence_system();  // every thread's words reach host memory before the flag
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

void lane_publish(MsmLane &ln, int slot, int n, const void *const *src, const size_t *bytes) {
  char *m = (char *)ln.mapped.ensure(LANE_MAPPED_BYTES);
  (void)m;
  PubArgs a{};
  size_t total = 0;
  a.n = n;
  for (int k = 0; k < n; k++) {
    a.src[k] = (const uint32_t *)src[k];
    a.words[k] = (uint32_t)(bytes[k] / 4);
    total += bytes[k];
  }
  const size_t cap = (slot == 2 ? LANE_MAPPED_BYTES : LANE_MAPPED_DATA[slot + 1]) - LANE_MAPPED_DATA[slot];
  if (total > cap) throw Error(TNS_ERR_DEVICE, "lane readback larger than its slot");
  const uint32_t seq = ++ln.pub_seq;
  ln.slot_seq[slot] = seq;
  char *dev = (char *)ln.mapped.dev;
  k_lane_publish<<<1, 256, 0, ln.stream>>>(a, (uint32_t *)(dev + LANE_MAPPED_DATA[slot]), (uint32_t *)(dev + 64 * slot),
                                           seq);
  TNS_LAUNCH_CHECK();
}

void lane_publish_slot(MsmLane &ln, int slot, uint32_t **data, uint32_t **flag, uint32_t *seq) {
  ln.mapped.ensure(LANE_MAPPED_BYTES);
  *seq = ++ln.pub_seq;
  ln.slot_seq[slot] = *seq;
  char *dev = (char *)ln.mapped.dev;
  *data = (uint32_t *)(dev + LANE_MAPPED_DATA[slot]);
  *flag = (uint32_t *)(dev + 64 * slot);
}

// the slot's publish has landed (no wait)
static bool lane_ready(MsmLane &ln, int slot) {
  const uint32_t *flag = (const uint32_t *)((const char *)ln.mapped.p + 64 * slot);
  return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == ln.slot_seq[slot];
}

const void *lane_wait(MsmLane &ln, int slot) {
  const char *m = (const char *)ln.mapped.p;
  const uint32_t *flag = (const uint32_t *)(m + 64 * slot), seq = ln.slot_seq[slot];
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spin = 1; __atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq; spin++) {
    if ((spin & 4095) == 0) {  // a faulted stream reports here instead of leaving the flag unset
      const hipError_t e = hipStreamQuery(ln.stream);
      if (e != hipSuccess && e != hipErrorNotReady) TNS_HIP(e);
      if (e == hipSuccess && __atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq)
        throw Error(TNS_ERR_DEVICE, "lane readback: stream idle without its publish");
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 120.0)
        throw Error(TNS_ERR_DEVICE, "lane readback did not arrive within 120 s");
    }
  }
  return m + LANE_MAPPED_DATA[slot];
}

// the largest bit length of Montgomery scalars; the sort then reads them as they are
// (SortInput::mont: canonicalised in its digit pass instead of through a canonical copy)
// With a plan hint for n scalars (the lane's previous MSM of Montgomery scalars: a proof's value
// commitment is the same shape every call) pass 1's count kernel computes the bit length too and
// the sort keeps its histograms when the bit length confirms the plan (else it recounts): one read
// of the scalars and one launch less (C4's value commitment: k_scalar_bits 0.26 ms + the count).
static SortInput bits_launch(MsmLane &ln, const Fr *scalars, size_t n) {
  unsigned *d_bits = (unsigned *)ln.msm.words.ensure(2 * sizeof(unsigned));
  TNS_HIP(hipMemsetAsync(d_bits, 0, sizeof(unsigned), ln.stream));
  SortInput in;
  in.fr = scalars;
  in.mont = true;
  const MsmLane::PlanHint &h = ln.hint;
  // (narrow per-window plans -- the trace values -- also get their canonical low 64 bits written)
  const bool narrow = !h.plan.shared && h.plan.c * h.plan.W <= 64;
  if (!(h.n == n && h.plan.c > 0 && bucket_sort_precount_bits(ln, scalars, n, h.plan, d_bits, in, narrow))) {
    k_scalar_bits<<<grid_for(n, 256, 2048), 256, 0, ln.stream>>>(scalars, n, d_bits, nullptr);
    TNS_LAUNCH_CHECK();
  }
  const void *src[1] = {d_bits};
  const size_t by[1] = {sizeof(unsigned)};
  lane_publish(ln, LANE_SLOT_BITS, 1, src, by);
  return in;
}

static unsigned bits_result(MsmLane &ln) { return *(const unsigned *)lane_wait(ln, LANE_SLOT_BITS); }

// An MSM's first step on its lane: the scalars' prep, then their bit length on its way to the host
// (computed here for Montgomery scalars; canonical inputs -- the opening quotients -- and raw u64
// inputs -- trace addresses, lookup indices -- come with theirs).  Returns what the sort will read.
static SortInput msm_prepare_scalars(MsmLane &ln, const MsmArgs &x) {
  if (x.src.prep) x.src.prep(ln.stream);
  if (x.n <= 64) return SortInput();
  if (!x.src.canon_bits) return bits_launch(ln, x.scalars, x.n);
  if (x.plan_bits <= 0) {  // (plan_bits: nothing to read back)
    const void *src[1] = {x.src.canon_bits};
    const size_t by[1] = {sizeof(unsigned)};
    lane_publish(ln, LANE_SLOT_BITS, 1, src, by);
  }
  SortInput in;
  if (x.src.u64) {
    in.u64 = x.src.u64;
    in.n_u64 = x.src.n_u64;
  } else {
    in.fr = x.src.canon ? x.src.canon : x.scalars;
    in.precounted = x.precounted;
    in.pre = x.pre;
  }
  return in;
}
// the bit length msm_prepare_scalars put on its way (a host wait, unless the caller fixed it)
static unsigned msm_bits(MsmLane &ln, const MsmArgs &x) {
  return x.n <= 64 ? 254u : x.plan_bits > 0 ? (unsigned)x.plan_bits : bits_result(ln);
}

// Entries per accumulation thread.  Per-window plans (the narrow commitments: runs of a few
// entries, flush- and latency-bound): 128, halved down to 32 while the MSM gives fewer than
// ACC_THREADS_CU threads per CU -- short chunks shorten each thread's dependent chain.
// Table-window plans (full-width scalars) whose count the sort read back: the largest chunk
// <= 128 that fills whole rounds of the resident blocks (fewer chunks, fewer head/tail partials
// for the fixup: C2 2.17 -> 2.11 ms; the 2^24 openings keep 128, `profiles/r02_ab_acc_rounds.txt`).
constexpr int ACC_THREADS_CU = 1024;
static int acc_chunk(Ctx *ctx, size_t entries, bool table_plan) {
  if (!table_plan) {
    const size_t want = (size_t)ctx->num_cu * ACC_THREADS_CU;
    int k = 128;
    while (k > 32 && entries / k < want) k /= 2;
    return k;
  }
  static const int bpc = [] {  // resident blocks of 256 threads per CU (VGPR-bound: 3)
    int b = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_accumulate<false>, 256, 0) != hipSuccess || b < 1) b = 3;
    return b;
  }();
  const size_t slots = (size_t)ctx->num_cu * bpc * 256, kmax = 128;
  const size_t rounds = std::max<size_t>(1, (entries + kmax * slots - 1) / (kmax * slots));
  const size_t k = (entries + rounds * slots - 1) / (rounds * slots);
  return (int)std::max<size_t>(16, std::min<size_t>(kmax, k));
}

// Phase 1 on lane `ln` (asynchronous): plan, digits and the bucket order.  Trivial cases
// (all scalars zero, n <= 64) finish here.  `sorted` (optional) is recorded on the lane once
// the bucket order exists (or right away when there is none).
// in, bits: from msm_prepare_scalars and msm_bits.  defer: stop after pass 1; msm_sort_passes and
// msm_finish_sort (the sort's host wait) complete it, so a pair queues both lanes' passes before either waits.
struct SortOptions {
  hipEvent_t sorted = nullptr;
  bool defer = false;
};
static void msm_sort_passes(MsmJob &J);
static void msm_finish_sort(MsmJob &J);
static void msm_launch_sort(Ctx *ctx, MsmLane &ln, const MsmArgs &x, const SortInput &in, unsigned bits, MsmJob &J,
                            const SortOptions &opt = SortOptions()) {
  J.expect(MsmStage::None, "MSM job launched twice");
  const size_t n = x.n;
  J.lane = &ln;
  J.ctx = ctx;
  hipStream_t st = ln.stream;
  auto record_now = [&]() {  // (no bucket order to wait for)
    if (opt.sorted) TNS_HIP(hipEventRecord(opt.sorted, st));
  };
  if (n == 0 || bits == 0) {  // all scalars zero
    J.stage = MsmStage::Immediate;
    record_now();
    return;
  }
  if (n <= 64) {
    G1Xyzz *d = (G1Xyzz *)ln.msm.tiny_out.ensure(sizeof(G1Xyzz));
    k_msm_tiny<<<1, 64, 0, st>>>(x.points, x.scalars, (int)n, d);
    TNS_LAUNCH_CHECK();
    const void *src[1] = {d};
    const size_t by[1] = {sizeof(G1Xyzz)};
    lane_publish(ln, LANE_SLOT_SUMS, 1, src, by);
    J.stage = MsmStage::Tiny;
    record_now();
    return;
  }
  if (n >= ((size_t)1 << 31)) throw Error(TNS_ERR_COMMITMENT, "MSM larger than 2^31 points");

  const FixedBase *fb = x.fb;
  const TableShape table = fb ? TableShape{fb->n, fb->c, fb->W} : TableShape();
  const MsmPlan &P = J.P = plan_msm(n, (int)bits, table, x.fb_off, ctx->msm_tables);
  // (plan_msm: the shared layout when a fixed-base table covers the points -- T[w n + fb_off + i]: value w stride + i)
  J.points = P.shared ? fb->table.as<G1Affine>() + x.fb_off : x.points;
  if (in.mont && in.fr && !in.u64) ln.hint = MsmLane::PlanHint{n, P};
  const size_t total = (size_t)P.W * n;
  if (total >= ((size_t)1 << 31)) throw Error(TNS_ERR_COMMITMENT, "MSM too large for one sort");

  J.acc_k = acc_chunk(ctx, total, false);  // from the bound; table plans refine it from the sort's count
  J.nchunks = (total + J.acc_k - 1) / J.acc_k;
  J.n = n;
  J.sort_prof.reset(new ProfScope(ctx->prof, st, "msm_sort", 32.0 * n + 16.0 * total));
  J.valid = (uint32_t *)ln.msm.words.ensure(2 * sizeof(uint32_t));  // entries; [1]: a run crosses a chunk
  bucket_sort_begin(ln, sort_input_for_bits(in, n, bits), n, P, J.valid, J.bs);
  J.sorted_ev = opt.sorted;
  J.stage = MsmStage::Pass1Queued;
  if (opt.defer) return;
  msm_sort_passes(J);
  msm_finish_sort(J);
}

// the bucket sort's passes after pass 1, up to the last pass's readback (no host wait)
static void msm_sort_passes(MsmJob &J) {
  if (J.stage == MsmStage::Immediate || J.stage == MsmStage::Tiny) return;  // nothing to sort
  J.expect(MsmStage::Pass1Queued, "MSM sort passes without pass 1");
  bucket_sort_passes(J.bs);
  J.stage = MsmStage::PassesQueued;
}

// the bucket sort's last stage (waits for its last-pass readback), then the sorted state
static void msm_finish_sort(MsmJob &J) {
  if (J.stage == MsmStage::Immediate || J.stage == MsmStage::Tiny) return;
  J.expect(MsmStage::PassesQueued, "MSM sort finished before its passes");
  const BucketOrder o = bucket_sort_finish(J.bs);
  J.sort_prof.reset();  // the stage's end event, after the last pass on the lane
  if (o.entries != SIZE_MAX && J.P.shared) {  // table plans: chunks sized from the actual entry count
    J.acc_k = acc_chunk(J.ctx, o.entries, true);
    J.nchunks = std::max<size_t>(1, (o.entries + J.acc_k - 1) / J.acc_k);
  }
  J.keys2 = o.keys;
  J.vals2 = o.vals;
  J.bstart = o.bstart;
  J.bend = o.bstart + 1;
  J.ks = o.ks;
  J.stage = MsmStage::Sorted;
  if (J.sorted_ev) TNS_HIP(hipEventRecord(J.sorted_ev, J.lane->stream));
  J.sorted_ev = nullptr;
}

// Phase 2 (asynchronous): accumulation, bucket fixup, reduction and the per-set sums' readback.
// `accumulated` (optional) is recorded on the lane right after the accumulation kernel.
static void msm_launch_accumulate(Ctx *ctx, MsmJob &J, hipEvent_t accumulated, hipStream_t on = nullptr) {
  if (!J.sorted()) {  // immediate / tiny: done in phase 1
    if (accumulated) TNS_HIP(hipEventRecord(accumulated, on ? on : J.lane->stream));
    return;
  }
  MsmLane &ln = *J.lane;
  hipStream_t st = on ? on : ln.stream;
  if (!J.buckets) J.buckets = (G1Xyzz *)ln.msm.buckets.ensure(sizeof(G1Xyzz) * J.P.nb);
  HeadTail *ht = (HeadTail *)ln.msm.head_tail.ensure(sizeof(HeadTail) * J.nchunks);
  J.ht = ht;
  {
    TNS_PROF_ON(ctx, st, "msm_accumulate", 96.0 * J.n);  // 96 B per (scalar, point) pair
    uint2 *cbk = (uint2 *)ln.msm.chunk_bounds.ensure(sizeof(uint2) * J.nchunks);
    J.cbk = cbk;
    auto acc = J.keys2 ? k_accumulate<true> : k_accumulate<false>;
    acc<<<grid_for(J.nchunks, 256, 1u << 30), 256, 0, st>>>(J.keys2, J.vals2, J.valid, J.points, J.buckets, ht,
                                                            J.nchunks, J.ks, J.acc_k, J.bstart, J.P.nb, cbk,
                                                            J.valid + 1);
    TNS_LAUNCH_CHECK();
  }
  if (accumulated) TNS_HIP(hipEventRecord(accumulated, st));
}

// two sorted MSMs whose tails can run as one two-set launch sequence: the same bucket-set shape
static bool same_tail_shape(const MsmJob &a, const MsmJob &b) {
  return a.sorted() && b.sorted() && a.P.shared == b.P.shared && a.P.Wr == b.P.Wr && a.P.half == b.P.half;
}

// The accumulation's tail -- bucket fixup, reduction and the per-set sums' readback -- for nj = 1
// MSM, or nj = 2 of the same shape (same_tail_shape, buckets adjoining: J[1]->buckets ==
// J[0]->buckets + nb) as ONE sequence of launches on lane `run` whose grids cover both (a pair's two
// tails side by side on two lanes were short chains at low occupancy each, and the second lane's
// fixup took 0.97 ms against 0.38 ms for the same work on the first).
static void msm_launch_tails(Ctx *ctx, MsmJob *const *J, int nj, MsmLane &run) {
  for (int j = 0; j < nj; j++) {
    J[j]->res_lane = &run;
    J[j]->res_set = j;
    J[j]->res_sets = nj;
  }
  if (!J[0]->sorted()) return;
  hipStream_t st = run.stream;
  const MsmPlan &P = J[0]->P;
  if (nj == 2 && (!same_tail_shape(*J[0], *J[1]) || J[1]->buckets != J[0]->buckets + P.nb))
    throw Error(TNS_ERR_DEVICE, "two-set MSM tail over MSMs of different shapes");
  {
    TNS_PROF_ON(ctx, st, "msm_fixup", 0.0);
    FixupArgs FA{};
    int max_levels = 0;
    size_t max_nb = 0;
    for (int j = 0; j < nj; j++) {
      MsmJob &X = *J[j];
      FixLevels &F = FA.s[j].F;
      const FixLevelSizes sz = fix_level_sizes(X.nchunks);  // nchunks/F, /F^2, ...
      F.n = sz.n;
      for (int l = 1; l <= sz.n; l++) F.len[l] = sz.len[l];
      if (F.n) {
        G1Xyzz *base = (G1Xyzz *)X.lane->msm.fix.ensure(sizeof(G1Xyzz) * sz.total);
        size_t o = 0;
        for (int l = 1; l <= F.n; o += F.len[l], l++) F.lv[l] = base + o;
      }
      X.fix_levels = F.n;
      max_levels = std::max(max_levels, F.n);
      FA.s[j] = FixupSet{X.bstart, X.bend, X.valid, X.ht, F, X.buckets, X.P.nb, X.acc_k};
      max_nb = std::max(max_nb, X.P.nb);
    }
    for (int l = 1; l <= max_levels; l++) {
      FixLevelArgs LA{};
      size_t max_groups = 0;
      for (int j = 0; j < nj; j++) {
        const FixLevels &F = FA.s[j].F;
        const MsmJob &X = *J[j];
        LA.s[j] = FixLevelSet{X.valid, FA.s[j].ht, F.lv[l - 1], F.lv[l], X.cbk,
                              l <= F.n ? F.len[l] : 0, X.acc_k};
        if (l <= F.n) max_groups = std::max(max_groups, F.len[l]);
      }
      k_fix_level<<<dim3(grid_for(max_groups * FIX_FAN, 256, 1u << 30), nj), 256, 0, st>>>(LA, l);
      TNS_LAUNCH_CHECK();
    }
    k_bucket_fixup<<<dim3(grid_for(max_nb, 256), nj), 256, 0, st>>>(FA);
    TNS_LAUNCH_CHECK();
  }
  // bucket reduction (see the header; its group sizes, chunks and sums: tail_geom, msm_plan.hpp)
  const int sets = P.Wr * nj;
  const TailGeom G = tail_geom(P.half);
  const int L0 = G.L0, L1 = G.L1, nbits = G.nbits, specs = G.specs;
  const size_t g1 = G.g1, g = G.g;
  {
    TNS_PROF_ON(ctx, st, "msm_reduce", 128.0 * P.nb * nj);
    G1Xyzz *T = (G1Xyzz *)run.msm.level_sums.ensure(sizeof(G1Xyzz) * 2 * sets * (g1 + (L1 ? g : 0)));
    G1Xyzz *S = T + (size_t)sets * g1;
    k_reduce_level<<<grid_for((size_t)sets * g1, 64, 1u << 30), 64, 0, st>>>(J[0]->buckets, sets, P.half, L0, T, S);
    TNS_LAUNCH_CHECK();
    if (L1) {
      G1Xyzz *V = S + (size_t)sets * g1, *S2 = V + (size_t)sets * g;
      k_reduce_level2<<<grid_for((size_t)sets * g, 64, 1u << 30), 64, 0, st>>>(T, S, sets, g1, L1, G.lg0, V, S2);
      TNS_LAUNCH_CHECK();
      T = V;
      S = S2;
    }
    const size_t nparts = (size_t)sets * specs * G.nch;
    G1Xyzz *parts = (G1Xyzz *)run.msm.parts.ensure(sizeof(G1Xyzz) * (2 * nparts + (size_t)sets * specs));
    G1Xyzz *tmp = parts + nparts, *out = tmp + nparts;
    // (G.tree: each wave adds its 64 chunk sums by a butterfly)
    k_masked_sums<<<grid_for(nparts, 64, 1u << 30), 64, 0, st>>>(T, S, sets, g, nbits, G.CH, parts, G.tree);
    TNS_LAUNCH_CHECK();
    sum_sets(st, parts, sets * specs, G.sum_n, tmp, out);
    // the per-set sums, then each MSM's number of sorted non-zero digits (= mixed additions of
    // k_accumulate, profiling)
    const void *src[3] = {out, J[0]->valid, nj == 2 ? J[1]->valid : nullptr};
    const size_t by[3] = {sizeof(G1Xyzz) * sets * specs, sizeof(uint32_t), sizeof(uint32_t)};
    if (J[0]->device_finish) J[0]->sums = out;  // (thousands of sets: not through the lane's slot)
    else lane_publish(run, LANE_SLOT_SUMS, 1 + nj, src, by);
  }
  for (int j = 0; j < nj; j++) {
    J[j]->L0 = G.weight;  // the masked sums' weight (msm_window_sums' doublings)
    J[j]->nbits = nbits;
    J[j]->specs = specs;
    J[j]->tail = G;
  }
}

// The host finish of a sorted MSM, first half: wait for the tail's readback, then per bucket set
// R = sum_g T_g + L0 * sum_b 2^b M_b -- the window sums (per-window layout) or the result (shared).
static std::vector<G1Xyzz> msm_window_sums(Ctx *ctx, MsmJob &J) {
  J.expect(MsmStage::Sorted, "window sums of an MSM without a bucket order");
  const MsmPlan &P = J.P;
  const G1Xyzz *all = (const G1Xyzz *)lane_wait(J.res_lane ? *J.res_lane : *J.lane, LANE_SLOT_SUMS);
  const G1Xyzz *fin = all + (size_t)J.res_set * P.Wr * J.specs;
  const uint32_t *cnt = (const uint32_t *)(all + (size_t)J.res_sets * P.Wr * J.specs);
  ctx->prof.add_ops("msm_accumulate", (double)cnt[J.res_set]);
  std::vector<G1Xyzz> Rw(P.Wr);
  for (int r = 0; r < P.Wr; r++) {
    const G1Xyzz *f = &fin[(size_t)r * J.specs];
    G1Xyzz acc = G1Xyzz::inf();
    for (int b = J.nbits - 1; b >= 0; b--) acc = xyzz_add(xyzz_dbl(acc), f[b]);
    for (int L = J.L0; L > 1; L >>= 1) acc = xyzz_dbl(acc);
    Rw[r] = xyzz_add(xyzz_add(f[J.nbits], f[J.nbits + 1]), acc);
  }
  return Rw;
}

// ... second half: Horner over the windows (per-window layout) or nothing (shared layout)
static G1Xyzz msm_horner(const MsmPlan &P, const std::vector<G1Xyzz> &Rw) {
  if (P.shared) return Rw[0];
  G1Xyzz acc = Rw[P.W - 1];
  for (int w = P.W - 2; w >= 0; w--) {
    for (int k = 0; k < P.c; k++) acc = xyzz_dbl(acc);
    acc = xyzz_add(acc, Rw[w]);
  }
  return acc;
}

// Wait for the tail's readback and finish on the host
static G1Xyzz msm_complete(Ctx *ctx, MsmJob &J) {
  if (J.stage == MsmStage::Immediate) return G1Xyzz::inf();
  if (J.stage == MsmStage::Tiny) return *(const G1Xyzz *)lane_wait(J.res_lane ? *J.res_lane : *J.lane, LANE_SLOT_SUMS);
  return msm_horner(J.P, msm_window_sums(ctx, J));
}

// a whole MSM queued on a lane (one host wait for the bit length, one inside the sort) for msm_complete
static void msm_queue_whole(Ctx *ctx, MsmLane &ln, const MsmArgs &x, MsmJob &J) {
  const SortInput in = msm_prepare_scalars(ln, x);
  const unsigned bits = msm_bits(ln, x);
  msm_launch_sort(ctx, ln, x, in, bits, J);
  msm_launch_accumulate(ctx, J, nullptr);
  MsmJob *one[1] = {&J};
  msm_launch_tails(ctx, one, 1, ln);
}

G1Xyzz msm_dev(Ctx *ctx, const G1Affine *points, const Fr *scalars, size_t n, const FixedBase *fb, size_t fb_off) {
  if (n == 0) return G1Xyzz::inf();
  MsmJob J;
  msm_queue_whole(ctx, ctx->lanes[0], MsmArgs{points, scalars, n, fb, fb_off}, J);
  return msm_complete(ctx, J);
}

// The stages after the sort alone (msm.hpp): jobs filled at stage Sorted, then the same
// msm_launch_accumulate, msm_launch_tails and host finish as msm_dev / msm_pair_dev -- no launch
// sequence of its own.  Set j takes lane j's workspaces, as a pair's MSMs do, and everything is
// queued on lane 0's stream; two sets' buckets adjoin in lane 0's buffer, as msm_pair_queue arranges.
void msm_from_order_dev(Ctx *ctx, const MsmPlan &P, const OrderedSet *sets, int nj, OrderedMsm &out) {
  if (nj < 1 || nj > 2 || P.nb == 0 || P.nb != (size_t)P.Wr * P.half || (nj == 2 && !P.shared))
    throw Error(TNS_ERR_INVALID_PARAMETERS, "MSM from a bucket order: one set, or two of the shared layout");
  MsmLane &run = ctx->lanes[0];
  MsmJob J[2];
  try {
    for (int j = 0; j < nj; j++) {
      const OrderedSet &s = sets[j];
      if (!s.order.vals || !s.order.bstart || !s.valid || !s.points || s.acc_k < 1 || s.nchunks < 1)
        throw Error(TNS_ERR_INVALID_PARAMETERS, "MSM from a bucket order: a set without its order");
      MsmJob &X = J[j];
      X.lane = &ctx->lanes[j];
      X.ctx = ctx;
      X.P = P;
      X.points = s.points;
      X.keys2 = s.order.keys;
      X.vals2 = s.order.vals;
      X.bstart = s.order.bstart;
      X.bend = s.order.bstart + 1;
      X.ks = s.order.ks;
      X.valid = s.valid;
      X.acc_k = s.acc_k;
      X.nchunks = s.nchunks;
      X.n = s.order.entries == SIZE_MAX ? 0 : s.order.entries;  // (profiling's byte count only)
      X.stage = MsmStage::Sorted;
    }
    if (nj == 2) {
      J[0].buckets = (G1Xyzz *)run.msm.buckets.ensure(sizeof(G1Xyzz) * 2 * P.nb);
      J[1].buckets = J[0].buckets + P.nb;
    }
    for (int j = 0; j < nj; j++) msm_launch_accumulate(ctx, J[j], nullptr, run.stream);
    MsmJob *both[2] = {&J[0], &J[1]};
    msm_launch_tails(ctx, both, nj, run);
    for (int j = 0; j < nj; j++) {
      out.window_sums[j] = msm_window_sums(ctx, J[j]);
      out.result[j] = msm_horner(P, out.window_sums[j]);
      out.buckets[j] = J[j].buckets;
      out.fix_levels[j] = J[j].fix_levels;
    }
    out.tail = J[0].tail;
  } catch (...) {  // nothing queued here still runs on the caller's buffers
    (void)hipStreamSynchronize(run.stream);
    throw;
  }
}

// ---------------------------------------------------------------- a batch over one base
// The finish of a batch on the device (msm_complete's host arithmetic), in two kernels:
//  * k_batch_set_sums, per group: thread per bucket set forms window w of row b's sum
//    R = sum_g T_g + L0 sum_s 2^s M_s from the set's specs (fin: sets x specs canonical points) into
//    R[b W + w] -- a dozen dependent doublings and additions, every set in parallel;
//  * k_batch_horner, ONCE for all groups: thread per row runs Horner over the row's W windows -- a
//    chain of ~254 dependent doublings whatever the batch, so a fixed latency of the call (about
//    2 ms) that no group repeats.  Only the rows' points leave the device.
__global__ void __launch_bounds__(64) k_batch_set_sums(const G1Xyzz *__restrict__ fin, size_t sets, int specs, int nbits,
                                                       int lgL0, G1Xyzz *__restrict__ R) {
  const size_t set = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (set >= sets) return;
  const G1Xyzz *f = fin + set * (size_t)specs;
  G1Xyzz acc = G1Xyzz::inf();
  for (int s = nbits - 1; s >= 0; s--) acc = xyzz_add(xyzz_dbl(acc), f[s]);
  for (int k = 0; k < lgL0; k++) acc = xyzz_dbl(acc);
  R[set] = xyzz_add(xyzz_add(f[nbits], f[nbits + 1]), acc);
}

__global__ void __launch_bounds__(64) k_batch_horner(const G1Xyzz *__restrict__ R, size_t rows, int W, int c,
                                                     G1Xyzz *__restrict__ out) {
  const size_t row = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const G1Xyzz *r = R + row * (size_t)W;
  G1Xyzz acc = r[W - 1];
  for (int j = W - 2; j >= 0; j--) {
    for (int k = 0; k < c; k++) acc = xyzz_dbl(acc);
    acc = xyzz_add(acc, r[j]);
  }
  out[row] = acc;
}

unsigned msm_batch_bits_dev(Ctx *ctx, const Fr *scalars, size_t total) {
  if (!total) return 0;
  MsmLane &ln = ctx->lanes[0];
  unsigned *d_bits = (unsigned *)ln.msm.words.ensure(2 * sizeof(unsigned));
  TNS_HIP(hipMemsetAsync(d_bits, 0, sizeof(unsigned), ln.stream));
  {
    TNS_PROF_ON(ctx, ln.stream, "msm_batch_bits", 32.0 * total);
    k_scalar_bits<<<grid_for(total, 256, 2048), 256, 0, ln.stream>>>(scalars, total, d_bits, nullptr);
    TNS_LAUNCH_CHECK();
  }
  const void *src[1] = {d_bits};
  const size_t by[1] = {sizeof(unsigned)};
  lane_publish(ln, LANE_SLOT_BITS, 1, src, by);
  return bits_result(ln);
}

// One group after the other on lane 0: per group one sort (host wait: its last pass's tile totals),
// one accumulation, one tail and the finish kernel -- no host work or readback per row.  The lane's
// plan hint is left as the last single MSM wrote it.
void msm_batch_groups_dev(Ctx *ctx, const G1Affine *points, const Fr *scalars, size_t n, size_t rows, unsigned bits,
                          const BatchPlan &B, G1Affine *out, BatchReport *rep) {
  if (B.route != BATCH_ROUTE_BATCHED || B.group_rows == 0 || bits == 0 || n == 0)
    throw Error(TNS_ERR_DEVICE, "batched MSM without a batched plan");
  MsmLane &ln = ctx->lanes[0];
  hipStream_t st = ln.stream;
  DevBuf rs, pre, wb;
  G1Xyzz *rowsum = (G1Xyzz *)rs.ensure(sizeof(G1Xyzz) * rows);
  const int W = B.P.W, c = B.P.c;  // (every group's: the window depends on n and the bits alone)
  G1Xyzz *winsum = (G1Xyzz *)wb.ensure(sizeof(G1Xyzz) * rows * (size_t)W);  // R[b W + w]
  Fq *prefix = (Fq *)pre.ensure(sizeof(Fq) * rows);
  try {
    for (size_t r0 = 0; r0 < rows; r0 += B.group_rows) {
      const size_t g = std::min(B.group_rows, rows - r0);
      // a group of zero rows among others has no digit entry to sort (a single MSM never sorts
      // such scalars either: bits == 0 ends it): its window sums are identities
      if (B.groups > 1 && msm_batch_bits_dev(ctx, scalars + r0 * n, g * n) == 0) {
        TNS_HIP(hipMemsetAsync(winsum + r0 * (size_t)W, 0, sizeof(G1Xyzz) * g * (size_t)W, st));
        continue;
      }
      MsmJob J;
      J.lane = &ln;
      J.ctx = ctx;
      const MsmPlan &P = J.P = plan_batch_group(n, g, (int)bits);
      if (P.W != W || P.c != c) throw Error(TNS_ERR_DEVICE, "batched MSM: a group with another window plan");
      const size_t total = (size_t)P.W * g * n;
      if (total >= ((size_t)1 << 31)) throw Error(TNS_ERR_COMMITMENT, "MSM batch group too large for one sort");
      J.points = points;
      J.n = g * n;
      J.acc_k = acc_chunk(ctx, total, false);
      J.nchunks = (total + J.acc_k - 1) / J.acc_k;
      J.valid = (uint32_t *)ln.msm.words.ensure(2 * sizeof(uint32_t));
      J.sort_prof.reset(new ProfScope(ctx->prof, st, "msm_sort", 32.0 * J.n + 16.0 * total));
      SortInput in;
      in.fr = scalars + r0 * n;
      in.mont = true;
      bucket_sort_begin(ln, in, g * n, P, J.valid, J.bs);
      J.stage = MsmStage::Pass1Queued;
      msm_sort_passes(J);
      msm_finish_sort(J);
      msm_launch_accumulate(ctx, J, nullptr);
      J.device_finish = true;
      MsmJob *one[1] = {&J};
      msm_launch_tails(ctx, one, 1, ln);
      int lgL0 = 0;
      while ((1 << lgL0) < J.L0) lgL0++;
      {
        TNS_PROF_ON(ctx, st, "msm_batch_finish", 128.0 * P.Wr * J.specs);
        k_batch_set_sums<<<grid_for((size_t)P.Wr, 64, 1u << 30), 64, 0, st>>>(J.sums, (size_t)P.Wr, J.specs, J.nbits, lgL0,
                                                                              winsum + r0 * (size_t)W);
        TNS_LAUNCH_CHECK();
      }
      if (rep) {
        rep->c = P.c;
        rep->W = P.W;
        rep->npass = J.bs.g.npass;
      }
    }
    {
      TNS_PROF_ON(ctx, st, "msm_batch_finish", 128.0 * rows * W);
      k_batch_horner<<<grid_for(rows, 64, 1u << 30), 64, 0, st>>>(winsum, rows, W, c, rowsum);
      TNS_LAUNCH_CHECK();
    }
    xyzz_to_affine_batch_dev(ctx, rowsum, rows, out, prefix);
    TNS_HIP(hipStreamSynchronize(st));  // the scratch dies here
  } catch (...) {  // nothing queued here still runs on buffers that are then freed
    (void)hipStreamSynchronize(st);
    throw;
  }
}

static void msm_pair_queue(Ctx *ctx, const MsmArgs &a, const MsmArgs &b, G1Xyzz out[2]) {
  if (a.src.late && !b.src.late) {  // the late vector goes second (lane 1)
    G1Xyzz o[2];
    msm_pair_queue(ctx, b, a, o);
    out[0] = o[1];
    out[1] = o[0];
    return;
  }
  MsmLane &l0 = ctx->lanes[0], &l1 = ctx->lanes[1];
  // lane 1 starts after everything already queued on the context stream (its inputs)
  stream_wait(l1.stream, ctx->stream);
  MsmJob ja, jb;
  if (b.src.late) {
    // b's scalars are still being uploaded (HostUpload, a helper thread): a's MSM is queued whole
    // first -- sort, accumulation, tail -- so it runs under the upload; b's prep then waits for
    // the upload and b's MSM follows on lane 1
    msm_queue_whole(ctx, l0, a, ja);
    if (b.src.chunks > 1) {  // one MSM per uploaded chunk, each as soon as it lands
      const ScalarSource &bs = b.src;
      if ((int)bs.chunk_off.size() != bs.chunks + 1 || bs.chunk_off.back() != b.n)
        throw Error(TNS_ERR_INVALID_PARAMETERS, "chunk offsets do not cover the scalars");
      G1Xyzz acc = G1Xyzz::inf();
      for (int k = 0; k < bs.chunks; k++) {
        const size_t off = bs.chunk_off[k], cnt = bs.chunk_off[k + 1] - off;
        if (!cnt) continue;
        MsmArgs bk{b.points + off, b.scalars + off, cnt, b.fb, off};  // (Montgomery scalars: no canon_bits)
        bk.src.prep = [&bs, k](hipStream_t s) { bs.chunk_prep(k, s); };
        MsmJob jk;
        msm_queue_whole(ctx, l1, bk, jk);
        acc = xyzz_add(acc, msm_complete(ctx, jk));  // the lane's host buffer serves the next chunk
      }
      out[0] = msm_complete(ctx, ja);
      out[1] = acc;
      return;
    }
    msm_queue_whole(ctx, l1, b, jb);
    out[0] = msm_complete(ctx, ja);
    out[1] = msm_complete(ctx, jb);
    return;
  }
  const SortInput ca = msm_prepare_scalars(l0, a), cb = msm_prepare_scalars(l1, b);
  const unsigned ba = msm_bits(l0, a), bb = msm_bits(l1, b);
  Event sa, sb;
  // both lanes' passes are queued before either lane's host wait (the last pass's readback), and
  // each lane's last pass follows its own readback: the two sorts run side by side and neither
  // waits for the other's first passes (profiles/r02_ab_sort_overlap.txt, r05_ab_sort_overlap.txt)
  msm_launch_sort(ctx, l0, a, ca, ba, ja, SortOptions{sa, true});
  msm_sort_passes(ja);
  msm_launch_sort(ctx, l1, b, cb, bb, jb, SortOptions{sb, true});
  msm_sort_passes(jb);
  // Both accumulations go on the context's accumulation stream (ctx->acc, at the least priority:
  // api.hip's create_streams), one after the other (each is VALU-bound on the whole chip: run together
  // they take as long), each as soon as its own sort is done: the first runs beside the rest of lane 1's
  // sort, which then finishes in the first accumulation's tail-off.  Waiting for both sorts first
  // left the chip to lane 1's last passes alone for ~1.2 ms; this is 0.4 ms faster per C4 step
  // (profiles/r06_ab_acc_stream.txt) -- lane 1's sort stage then spans the first accumulation.
  // A pair of table-window MSMs (the openings: full-width scalars, ~16 ms accumulations) runs both
  // tails after the second accumulation as ONE two-set launch sequence on lane 0 (tails under the
  // second accumulation took wave slots from it, profiles/r02_ab_tails_last.txt); the commitments
  // keep lane 0's tail under lane 1's accumulation (the 22-bit address MSM's 2^22-bucket reduction
  // is longer than the value accumulation).
  hipStream_t as = ctx->acc;
  msm_finish_sort(ja);
  Event acc_a, acc_b;
  // a two-set tail needs the pair's buckets adjoining: room for both before acc a writes the first
  if (ja.sorted() && ja.P.shared) ja.buckets = (G1Xyzz *)l0.msm.buckets.ensure(sizeof(G1Xyzz) * 2 * ja.P.nb);
  TNS_HIP(hipStreamWaitEvent(as, sa, 0));
  msm_launch_accumulate(ctx, ja, acc_a, as);
  msm_finish_sort(jb);
  const bool tails_last = ja.sorted() && jb.sorted() && ja.P.shared && jb.P.shared;
  const bool two_set = tails_last && same_tail_shape(ja, jb);
  if (two_set) jb.buckets = ja.buckets + ja.P.nb;
  TNS_HIP(hipStreamWaitEvent(as, sb, 0));
  msm_launch_accumulate(ctx, jb, acc_b, as);
  TNS_HIP(hipStreamWaitEvent(l0.stream, tails_last ? acc_b : acc_a, 0));
  if (two_set) {
    MsmJob *both[2] = {&ja, &jb};
    msm_launch_tails(ctx, both, 2, l0);
  } else {
    TNS_HIP(hipStreamWaitEvent(l1.stream, acc_b, 0));
    MsmJob *one_a[1] = {&ja}, *one_b[1] = {&jb};
    msm_launch_tails(ctx, one_a, 1, l0);
    msm_launch_tails(ctx, one_b, 1, l1);
  }
  // two tails on two lanes: the host's part (bucket-sum Horner, ~20-45 us) of whichever lands
  // first runs while the other lane's tail still runs on the device
  if (!two_set && jb.res_lane && jb.res_lane != ja.res_lane && jb.sorted() && ja.sorted()) {
    // (bounded: past it the plain order below, whose waits report a faulted stream)
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spin = 1; !lane_ready(*ja.res_lane, LANE_SLOT_SUMS) && !lane_ready(*jb.res_lane, LANE_SLOT_SUMS);
         spin++)
      if ((spin & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(500)) break;
    if (!lane_ready(*ja.res_lane, LANE_SLOT_SUMS) && lane_ready(*jb.res_lane, LANE_SLOT_SUMS)) {
      out[1] = msm_complete(ctx, jb);
      out[0] = msm_complete(ctx, ja);
      return;
    }
  }
  out[0] = msm_complete(ctx, ja);
  out[1] = msm_complete(ctx, jb);
}

// When a pair fails part-way (a lane's wait, a HIP call, the chunk-offset check), nothing it queued
// is still running once the error leaves: an accumulation left on ctx->acc would write lane 0's
// buckets and fix-up flags under the context's next proof.  A pair that succeeds pays nothing.
void msm_pair_dev(Ctx *ctx, const MsmArgs &a, const MsmArgs &b, G1Xyzz out[2]) {
  try {
    msm_pair_queue(ctx, a, b, out);
  } catch (...) {
    (void)hipStreamSynchronize(ctx->acc);
    for (MsmLane &ln : ctx->lanes) (void)hipStreamSynchronize(ln.stream);
    throw;
  }
}

}  // namespace tns
