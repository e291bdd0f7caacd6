// msm_plan.hpp -- where an MSM's window plan (plan_msm, for msm.hip) and its bucket sort's geometry
// (sort_geom, for bucket_sort.hip) are decided, once: host arithmetic alone (plain C++17, no HIP),
// so it is tested without a device (tests/test_msm_plan_cpu.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace tns {

// ---------------------------------------------------------------- the sort's constants
#ifndef TNS_BS_BLOCK
#define TNS_BS_BLOCK 256
#endif
constexpr int BS_BLOCK = TNS_BS_BLOCK;  // 4 waves: fits the slots k_accumulate leaves free
constexpr int BS_MAXBITS = 9;  // key bits per pass
constexpr int BS_MAXBINS = 1 << BS_MAXBITS;
#ifndef TNS_BS_TILE_MAX
#define TNS_BS_TILE_MAX 8192
#endif
constexpr int BS_TILE = TNS_BS_TILE_MAX;  // entries per tile at most (LDS staging: 8 B each, 64 KiB at 8192)
// up to SCAN_SMALL counts are scanned in ONE launch (bucket_sort.hip k_scan_single, k_bs_geom)
#ifndef TNS_SCAN_SMALL_LOG  // (build-time A/B only)
#define TNS_SCAN_SMALL_LOG 15
#endif
constexpr size_t SCAN_SMALL = (size_t)1 << TNS_SCAN_SMALL_LOG;
// key formats between passes (bucket_sort.hip): 4-byte keys, or 2-byte keys (<= 16 key bits left)
enum { KF_U32 = 0, KF_U16 = 1 };

// ---------------------------------------------------------------- the window plan
// One MSM's W signed windows of c bits; shared: all in ONE set of 2^(c-1) buckets over a fixed-base
// table of `stride` points a window (else W sets); bucket_bits: of a bucket index (window bits included).
struct WindowPlan {
  int c = 0, W = 0;
  bool shared = false;
  int bucket_bits = 0;
  uint32_t stride = 0;
  // a batch of `rows` MSMs over the same n_row points sorted as one (per-window layout only): scalar
  // e = b n_row + i of the rows x n_row array is row b's scalar of point i, and row b's window w is
  // bucket set b W + w (msm_batch_plan.hpp).  rows == 1: one MSM, n_row unused.
  uint32_t rows = 1;
  size_t n_row = 0;
};
// pass-1 histograms counted for `a` serve a sort of the same scalars with `b` (the stride: values only)
inline bool same_counts(const WindowPlan &a, const WindowPlan &b) {
  return a.c == b.c && a.W == b.W && a.shared == b.shared && a.bucket_bits == b.bucket_bits && a.rows == b.rows &&
         (a.rows == 1 || a.n_row == b.n_row);
}
// the plan with what the reduction needs
struct MsmPlan : WindowPlan {
  int Wr = 0;       // bucket sets (windows) to reduce: W (per-window) or 1 (shared)
  size_t half = 0;  // buckets per set, 2^(c-1)
  size_t nb = 0;    // buckets in total
};

// signed-digit windows of c bits for `bits`-bit scalars: the top window's raw value
// < 2^(bits - c(W-1)) must stay <= 2^(c-1) so that it never carries out
inline int windows_for(int bits, int c) {
  int W = (bits + c - 1) / c;
  if (bits - c * (W - 1) > c - 1) W++;
  return W;
}

// bucket additions + ~3 additions per bucket in the reduction
inline double plan_cost(size_t n, int W, int c, int sets) {
  return (double)W * (double)n + 3.0 * sets * (double)((size_t)1 << (c - 1));
}

// w1max > cmax: scalars of up to w1max - 1 bits may also take one window of bits + 1 (no
// second window for the signed digits' carry, e.g. 22-bit trace addresses: n additions
// instead of 2n, and no thousands-deep buckets)
// tie: a window must cost below tie x the best smaller one to be taken (0.98: near-ties go to the
// smaller window, less bucket memory)
inline int best_window(size_t n, int bits, int cmax, bool shared, int w1max = 0, double tie = 0.98) {
  int lg = 0;
  while (((size_t)1 << lg) < n) lg++;
  double best = 1e300;
  int bc = 4;
  for (int c = 4; c <= cmax && c <= lg + 2; c++) {
    const int W = windows_for(bits, c);
    const double cost = plan_cost(n, W, c, shared ? 1 : W);
    if (cost < best * tie) {
      best = cost;
      bc = c;
    }
  }
  const int c1 = bits + 1;
  if (c1 > cmax && c1 <= w1max && c1 <= lg + 2 && plan_cost(n, 1, c1, 1) < best * tie) bc = c1;
  return bc;
}

// the window a table for n points uses: the shared-layout optimum for full-width scalars
inline int table_window(size_t n) {
  // no near-tie preference for the shared tables: at 2^20 + 1 points c = 19 (W = 14) was taken
  // over c = 20 (W = 13, 2 % cheaper in plan_cost) and the 2^20 MSM over it ran 2.42 vs 2.01 ms
  // (deeper buckets: 56 vs 26 entries each, k_bucket_fixup 0.28 vs 0.07 ms)
  return best_window(n, 254, 22, true, 0, 1.0);
}

inline void finish_plan(MsmPlan &p) {
  p.half = (size_t)1 << (p.c - 1);
  p.Wr = p.shared ? 1 : p.W;
  int wbits = 0;  // per-window layout: the window index is part of the bucket index
  while ((1 << wbits) < p.Wr) wbits++;
  p.bucket_bits = wbits + p.c - 1;
  p.nb = (size_t)p.Wr * p.half;
}

// a fixed-base window table's shape (msm.hpp FixedBase); n == 0: there is none
struct TableShape { size_t n = 0; int c = 0, W = 0; };
// The plan of an MSM of n points (64 < n < 2^31) by scalars of `bits` bits: the per-window layout,
// or the shared layout when a table covers the points -- entries [fb_off, fb_off + n) of the set
// it was built for -- its values fit 31 bits, its windows reach `bits` and it costs less (-> shared).
inline MsmPlan plan_msm(size_t n, int bits, const TableShape &t, size_t fb_off, bool tables) {
  MsmPlan P;
  P.c = best_window(n, bits, 20, false, 23);
  P.W = windows_for(bits, P.c);
  if (t.n && tables && t.n >= fb_off + n && (uint64_t)t.n * t.W < ((uint64_t)1 << 31)) {
    const int Ws = windows_for(bits, t.c);
    if (Ws <= t.W && plan_cost(n, Ws, t.c, 1) < plan_cost(n, P.W, P.c, P.W)) {
      P.shared = true;
      P.c = t.c;
      P.W = Ws;
      P.stride = (uint32_t)t.n;
    }
  }
  finish_plan(P);
  return P;
}

// ---------------------------------------------------------------- the sort's geometry
// The (c, W, scalars per thread) that pass 1 has compile-time kernels for: the fixed-base table
// windows (n = 2^20..2^26) and the narrow trace commitments' per-window plans; anything else takes
// the runtime kernels.  bucket_sort.hip's kPass1Kernels holds the kernels IN THIS ORDER.
struct Pass1Shape { int c, W, spt; };
constexpr Pass1Shape kPass1Shapes[] = {{22, 12, 3}, {20, 13, 3}, {19, 14, 3}, {17, 15, 3}, {16, 2, 16}, {12, 2, 16}};
constexpr int kPass1ShapeCount = (int)(sizeof(kPass1Shapes) / sizeof(kPass1Shapes[0]));

// Everything a sort of the W n digit entries of n scalars derives from numbers alone (a batch,
// plan.rows > 1: n = rows x n_row scalars in all).
struct SortGeom {
  size_t E = 0;  // entry slots (W n)
  WindowPlan plan;
  int wb = 0;           // window-index bits appended to the key (shared layout)
  int keybits = 0, npass = 0;
  int bits[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // key bits per pass
  int kf[8] = {0, 0, 0, 0, 0, 0, 0, 0};    // key format pass p writes (KF_*)
  // packed tail (pk): the second-to-last pass writes one u32 per entry -- the last pass's key
  // bits, the sign and the point index i (ibits bits) -- and the last pass reads that word and
  // writes the accumulation's values only (no keys: runs come from the bucket starts)
  bool pk = false, vo = false;  // vo: the last pass writes values only
  int ibits = 0;
  // pass 1: its shape (index into kPass1Shapes, -1: the runtime kernels), scalars per tile, tiles, bins, shift
  int ct = -1;
  size_t spb = 0, T1 = 0;
  int nb = 0, shift = 0;
  size_t max_seg = 0, max_tiles = 0, cnt_len = 0;  // segments, tiles of a later pass, count words at most
  // passes 1 .. npass - 1: the tile size; S + 1 <= SCAN_SMALL segment counts (k_bs_geom, else k_bs_tiles + scans)
  int tile[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool one_launch[8] = {false, false, false, false, false, false, false, false};
};
// (1 <= W <= BS_TILE and W n < 2^32 are the caller's to check; an MSM's keys have at most 31 bits)
inline SortGeom sort_geom(size_t n, const WindowPlan &plan) {
  SortGeom g;
  g.plan = plan;
  g.E = (size_t)plan.W * n;
  if (plan.shared)
    while ((1 << g.wb) < plan.W) g.wb++;
  const int keybits = g.keybits = plan.bucket_bits + g.wb;
  const int npass = g.npass = std::max(1, (keybits + BS_MAXBITS - 1) / BS_MAXBITS);
  int *bits = g.bits;
  // the last pass sorts LDS-sized segments by BS_MAXBITS bits; the passes before it split the
  // remaining bits evenly (25-bit keys: 8, 8, 9 -- pass 2 with 256 instead of 512 bins writes
  // 128-byte runs: 1.21 -> 1.02 ms at 2^24)
  const int last = bits[npass - 1] = std::min(keybits, BS_MAXBITS);
  for (int p = 0, rest = keybits - last; p < npass - 1; p++) {
    bits[p] = (rest + (npass - 2 - p)) / (npass - 1 - p);
    rest -= bits[p];
  }
  // packed tail: the second-to-last pass writes (last-pass key bits, sign, point index) as one
  // word when they fit (n <= 2^22 with a 9-bit last pass).  (A 7-bit last pass for 2^24 points,
  // 9, 9, 7, measured slower: it moved the cost into 512-bin passes, +3.3 ms of sort per C4 step
  // against -0.8 ms of reads.)  Values-only last pass (vo): whenever there is more than one pass --
  // the accumulation reads no keys (C4: k_accumulate 9.10 -> 8.8 ms).
  g.ibits = 1;  // (a batch's values are point indices of one row)
  while (((size_t)1 << g.ibits) < (plan.rows > 1 ? plan.n_row : n)) g.ibits++;
  g.vo = npass >= 2;
  // (unpack_value reads the window index from the low wb bits of the last pass's L key bits: L >= wb)
  g.pk = g.vo && npass >= 3 && last + g.ibits + 1 <= 32 && last >= g.wb;
  // key formats between passes: 2-byte keys into the last pass (its <= 9 key bits; C4 openings:
  // pass 2 -> 3, sort kernels -0.6 ms per step, profiles/r03_ab_sort_k16.txt), 4-byte keys elsewhere
  for (int p = 0, rest = keybits; p < npass - 1; p++) {
    rest -= bits[p];
    g.kf[p] = g.vo && p == npass - 2 && rest <= 16 ? KF_U16 : KF_U32;
  }
  if (g.pk) g.kf[npass - 2] = KF_U32;  // the packed words (pack_entry) are 4-byte

  // pass 1: scalars -> bins of the top bits[0] key bits
  g.nb = 1 << bits[0];
  g.shift = keybits - bits[0];
  for (int k = 0; k < kPass1ShapeCount && plan.rows == 1; k++)  // (a batch: the runtime kernels)
    if (kPass1Shapes[k].c == plan.c && kPass1Shapes[k].W == plan.W) g.ct = k;
  g.spb = (size_t)BS_TILE / plan.W;
  if (g.ct >= 0) g.spb = std::min(g.spb, (size_t)BS_BLOCK * kPass1Shapes[g.ct].spt);
  g.T1 = (n + g.spb - 1) / g.spb;
  g.max_seg = (size_t)1 << keybits;
  const size_t tmin = 4096;  // the smallest pass tile
  g.max_tiles = (g.E + tmin - 1) / tmin + (g.max_seg >> last) + 1;
  g.cnt_len = std::max((size_t)g.nb * g.T1, (size_t)BS_MAXBINS * g.max_tiles) + 1;

  size_t S = g.nb;  // segments before pass p
  for (int p = 1; p < npass; S <<= bits[p], p++) {
    // 8192-entry tiles, except a last pass whose segments average <= 3584 entries (4096: the
    // one-tile segments fill it, and half the LDS doubles the blocks per CU -- pass 3 of a 2^24
    // opening MSM 1.02 -> 0.61 ms, profiles/r02_ab_sort_tiles.txt)
    g.tile[p] = (p == npass - 1 && (g.E >> (keybits - bits[p])) <= 3584) ? 4096 : BS_TILE;
    g.one_launch[p] = S + 1 <= SCAN_SMALL;
  }
  return g;
}

// ---------------------------------------------------------------- the accumulation's tail
// What msm.hip's fix-up and bucket reduction derive from numbers alone (tests/test_accref_cpu.py
// walks every legal plan through it; DESIGN 2.16 has the table of what occurs).
constexpr int RED_L = 16;   // running-sum group size of the bucket reduction (sets of more than 2^19 buckets)
constexpr int FIX_FAN = 8;  // short peel chains: single-thread add chains are latency-bound
constexpr int FIX_LEVELS = 8;
// runs over more chunks than this are summed by a whole wave in k_bucket_fixup, shorter ones by one thread
constexpr size_t FIX_WAVE_SPAN = 512;

// The fix-up's level sizes for an accumulation of nchunks chunks: level l >= 1 has len[l] =
// nchunks / FIX_FAN^l groups and exists while that is >= 2 (a run climbs to a level only over two
// aligned groups of it); total: the groups of all levels, one allocation.
struct FixLevelSizes {
  int n = 0;  // levels built (0: none)
  size_t len[FIX_LEVELS + 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  size_t total = 0;
};
inline FixLevelSizes fix_level_sizes(size_t nchunks) {
  FixLevelSizes F;
  for (size_t groups = nchunks / FIX_FAN; F.n < FIX_LEVELS && groups >= 2; groups /= FIX_FAN) {
    F.len[++F.n] = groups;
    F.total += groups;
  }
  return F;
}

// The bucket reduction of sets of `half` buckets (msm.hip's header, steps 5 and 6): running sums
// over groups of L0 buckets, then the weighted group sum  sum_g g S_g = sum_b 2^b M_b,
// M_b = sum_{g: bit b of g} S_g,  as nbits + 2 plain sums (the M_b and sum_g T_g in two halves) --
// short dependency chains only.  Up to 2^19 buckets per set the chains are the latency: groups of 4
// and masked-sum chunks of 8 (C2, 2^20 points: 2.73 -> 2.65 ms); from 2^21 buckets groups of 16 stay
// the fastest (2^22, 2^24; 8: +0.19 ms, 32: +0.63 ms per C4 step, r05 A/B).  c >= 4: half >= 8, so g >= 2.
struct TailGeom {
  int L0 = 0;      // k_reduce_level's group
  int L1 = 0;      // k_reduce_level2's group (0: no second level)
  size_t g1 = 0;   // first-level groups per set
  size_t g = 0;    // groups the masked sums run over
  int nbits = 0, specs = 0;  // bits of a group index; sums per set (nbits masked + 2 halves of T)
  int CH = 0;      // items per masked-sum chunk
  size_t nch = 0;  // chunks per spec
  bool tree = false;  // k_masked_sums adds each wave's 64 chunk sums by a butterfly
  int lg0 = 0;     // log2 L0 (k_reduce_level2's doublings)
  int weight = 0;  // of the masked sums: L0, or L0 L1 with a second level (the host finish's doublings)
  size_t sum_n = 0;  // parts per spec that sum_sets adds
};
inline TailGeom tail_geom(size_t half) {
  TailGeom t;
  const bool small_sets = half <= ((size_t)1 << 19);
  t.L0 = (int)std::min<size_t>(small_sets ? 4 : RED_L, half / 2);
  t.g1 = half / t.L0;
  // a second level (k_reduce_level2, groups of L1 = 4) when the first leaves many groups
  t.L1 = t.g1 >= ((size_t)1 << 13) ? 4 : 0;
  if (t.L1 && t.g1 / t.L1 < 2) t.L1 = 0;
  t.g = t.L1 ? t.g1 / t.L1 : t.g1;
  while (((size_t)1 << t.nbits) < t.g) t.nbits++;
  t.specs = t.nbits + 2;
  while ((1 << t.lg0) < t.L0) t.lg0++;
  t.weight = t.L1 ? t.L0 * t.L1 : t.L0;
  t.CH = (int)std::min<size_t>(small_sets || t.L1 ? 8 : 16, t.g / 2);
  t.nch = t.g / (2 * (size_t)t.CH);
  t.tree = t.nch % 64 == 0;
  t.sum_n = t.tree ? t.nch / 64 : t.nch;
  return t;
}
// sum_sets (msm.hip) adds n parts per set: 8-way k_sum_chunks passes while this holds, then k_set_sum
inline bool sum_sets_splits(size_t n) { return n > 128 && n % 8 == 0; }

}  // namespace tns
