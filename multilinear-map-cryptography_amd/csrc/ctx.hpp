// ctx.hpp -- the per-device context: its streams, its named device workspaces and caches, the lock
// every entry point takes, the host-input uploaders, and the entry points of the modules that work
// on the context alone (mle.hip, zero_folds.hip, poly.hip, interp.hip).  The generic sum-check
// family's are sumcheck.hpp's.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <tuple>
#include <vector>

#include "bn254.hpp"
#include "hip_util.hpp"
#include "msm.hpp"
#include "profiler.hpp"

namespace tns {

// Per-level tables for exact interpolation on nodes {0..N-1} (interp.hip).
struct InterpPlan {
  unsigned log_n = 0;   // N = 2^log_n
  DevBuf fact, inv_fact;            // k!, 1/k!   (k < max(N, 2))
  DevBuf newton_kernel_hat;         // NTT_{2N}((-1)^t / t!), scaled by 1/(2N)
  DevBuf level_tables;              // per level: Vhat (2m) | Phat (2m)
  std::vector<size_t> level_off;    // element offset of level l (m = 2^l) in level_tables
};

// The scratch the context's own modules share: six grow-only allocations, each lent to several
// users under the names below.  This is the one place that binds a name to a storage.
//
// Why every sharing here is safe: each user is one host call (synthetic_division_dev;
// srs_generate_dev / fixed_base_mul_dev; mle_evaluate_dev; sumcheck_prove_dev; a node sweep inside
// one lagrange_* call) made under the context lock (CtxScope).  It launches on Ctx::stream only,
// takes its pointers from ensure() when it starts and keeps none after it returns, and no call
// uses two names of one storage.  So two users of a storage are ordered by that one stream, and a
// user that grows it frees the old allocation only after the device has drained (hipFree waits).
// A new user must fit that description, or take a DevBuf of its own.
class SharedScratch {
 public:
  static constexpr int SCAN_LEVELS = 6;
  // suffix scan (poly.hip): level `depth` of the chunk carries, n / 64^(depth + 1) pairs
  DevBuf &scan_level(int depth) { return slot[depth]; }
  // SRS generation / fixed-base multiplication (poly.hip): the comb table of G, and per slab the
  // canonical powers, their XYZZ multiples and the batch inversion's prefix products
  DevBuf &srs_table() { return slot[0]; }
  DevBuf &srs_powers() { return slot[1]; }
  DevBuf &srs_xyzz() { return slot[2]; }
  DevBuf &srs_prefix() { return slot[3]; }
  // mle_evaluate_dev: the fold chain's two halves
  DevBuf &mle_ping() { return slot[0]; }
  DevBuf &mle_pong() { return slot[1]; }
  // sumcheck_prove_dev: table i's first fold buffer (n / 2 entries; the second is SumcheckWs::pong)
  DevBuf &sc_fold(int table) { return slot[2 + table]; }
  // the node sweep of the Lagrange-route openings (lagrange.hip): chain products, partial sums,
  // device scalars and chain inverses in one allocation
  DevBuf &sweep_chains() { return slot[5]; }

 private:
  // slot 0: scan level 0 | the comb table | the MLE ping
  // slot 1: scan level 1 | the slab's powers | the MLE pong
  // slot 2: scan level 2 | the slab's XYZZ points | table 0's fold buffer
  // slot 3: scan level 3 | the slab's prefix products | table 1's fold buffer
  // slot 4: scan level 4 | table 2's fold buffer
  // slot 5: scan level 5 | table 3's fold buffer | the node sweep's chains
  // (each: see the argument above -- all users on Ctx::stream, no pointer kept past the call)
  DevBuf slot[SCAN_LEVELS];
};

// The sum-check's workspaces.  The generic provers (sumcheck.hip: sumcheck_prove_dev,
// composition_sum_dev; sumcheck_batch.hip) run on Ctx::stream; the single zero-closure fold chain of Twist /
// Shout::prove (zero_folds.hip: sumcheck_zero_folds_async) on Ctx::side.
struct SumcheckWs {
  // second fold buffer per table (the input tables stay intact).  Both provers use it: the prove
  // cores drain the side stream before they start and before they return (prove.hip SideDrain),
  // and every entry point holds the context lock, so the two never run at once
  DevBuf pong[4];
  DevBuf half[4], chal, out;      // the zero-closure fold chain on the side stream
  DevBuf partials;                // the round kernels' per-block sums (bounded by their grids)
  DevBuf counter;                 // round kernel: last-workgroup counter
  DevBuf poly;                    // ... and its composition (ScPoly, sumcheck.hip)
  PinnedBuf poly_host;            // (its host staging copy)
  MappedHostBuf mapped;           // round results + flag, polled by the host
  MappedHostBuf htab;             // the folded tables of the host's last rounds
  uint32_t seq = 0;               // the flag value of the latest round launch
  MappedHostBuf handoff;          // challenges for pre-queued round kernels (host writes)
  DevBuf rdev;                    // ... each copied to device memory by the waiting kernel
  DevBuf tail_sync;               // ... and relayed between the blocks of the persistent tail
  uint32_t chal_seq = 0;          // the flag value of the latest published challenge
  PinnedBuf host;                 // the zero-closure chain's challenges (in) and bound table values (out)
  // the batched prover (sumcheck_batch.hip), on Ctx::stream, one group at a time:
  DevBuf batch_fold[2];           // every table of every instance folded once (ping) and twice (pong)
  DevBuf batch_state;             // per instance: the round's challenge, its four sums, the bound table values, the block counter
  DevBuf batch_partials;          // the cross-block rounds' per-block sums
  PinnedBuf batch_host;           // the group's sums and bound values (in) and challenges (out)
};

// The one-pass batched MLE evaluation (mle_eval.hip), on Ctx::stream, one call at a time (the
// context lock).  Together at most 1/128 of the tables' bytes plus a few words an instance.
struct MleEvalWs {
  DevBuf points;    // the call's points, batch x nv
  DevBuf eq_hi;     // per instance the eq table of the variables above the low 8: 2^(nv-8) entries
  DevBuf partials;  // the cross-block regime's per-block sums, n_tables a block
  DevBuf values;    // the results, batch x n_tables
  DevBuf counters;  // per instance the blocks that have finished; zero between calls
};

// The resident vectors of Twist / Shout::prove (prove.hip).  One proof runs at a time (the context
// lock), and both protocols use the same names: Twist's addresses and values are Shout's table and
// lookup indices.
struct ProveWs {
  DevBuf raw;        // host input: the u64 addresses / lookup indices as the commitment's sort reads them
  DevBuf narrow;     // ... and their 24- or 32-bit upload staging, widened into `raw` on the device
  DevBuf flags;      // Twist: the is_write bytes of a host trace; Shout: the bad-index word
  DevBuf eval[2];    // the two committed evaluation vectors (Twist: addresses, values; Shout: table, indices)
  DevBuf optype;     // Twist: the op-type table, when the folds do not read the flag bytes
  DevBuf coeff[2];   // their interpolated coefficients (coefficient route, unsharded)
  DevBuf open_s[2];  // the two openings' scratch vectors (inverses and quotients)
  DevBuf bits;       // the bit-length word of the u64 vector
};

struct Ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  // workspaces
  SharedScratch scratch;
  DevBuf interp_x2;                     // interpolation's working vector of 2n elements (interp.hip)
  DevBuf sweep_totals;                  // the node sweep's per-block totals (lagrange.hip)
  SumcheckWs sc;
  MleEvalWs mle_eval;
  MappedHostBuf inv_mapped;             // the batch inversion's grand product + flag (lagrange.hip)
  uint32_t inv_seq = 0;
  hipStream_t side = nullptr;  // the zero-closure folds
  hipStream_t copy = nullptr;  // host-buffer uploads that overlap a proof's first MSM (HostUpload)
  hipStream_t acc = nullptr;   // an MSM pair's accumulations (msm_pair_dev)
  PinnedBuf stage;             // their pinned staging ring (upload.cpp, built on first use)
  hipEvent_t stage_ev[32] = {};  // upload.cpp's staging ring: one event per slot
  DevBuf qbits;        // opening quotients' bit lengths (lagrange_quotient_finish2_dev)
  MsmLane lanes[2];     // lanes[0].stream == stream; lanes[1] has its own stream
  ProveWs prove;
  DevBuf twiddles;  // stage-major TW[h + k] = w_{2h}^k (ntt.hpp), 2^twiddle_log entries, for the largest size seen
  unsigned twiddle_log = 0;
  DevBuf glv_tw;    // the same table split for the group NTT (glv_twiddles), for the largest k vc_open.hip saw
  unsigned glv_tw_log = 0;
  std::vector<std::unique_ptr<InterpPlan>> plans;  // indexed by log_n
  std::map<uint32_t, DevBuf> pass_tw;  // four-step pass twiddles keyed by (lo << 8 | r)
  std::map<std::tuple<size_t, size_t, size_t>, DevBuf> bary_w;  // (N, first, count) -> weights
  bool lagrange_commit = true;           // prove via the Lagrange-basis SRS when available
  bool msm_tables = true;                // shared-bucket MSM on fixed bases with window tables
  int num_cu = 256;
  int upload_chunks = 4;  // drop-in provers: value-upload node ranges, each committed as it lands (tns_ctx_set_upload_chunks)
  KernelProfiler prof;
  ~Ctx();
};
// upload.cpp: host-to-device copies of the drop-in provers' inputs, in add() order on the
// context's copy stream from a helper thread (pinned staging ring, worker threads); wait(i, s)
// makes stream s wait for item i.  The destructor joins the thread and drains the copy stream.
class HostUpload {
 public:
  explicit HostUpload(Ctx *c);
  ~HostUpload();
  HostUpload(const HostUpload &) = delete;
  HostUpload &operator=(const HostUpload &) = delete;
  int add(void *dst, const void *src, size_t bytes);
  // n u64 values (trace addresses, lookup indices) sent packed into `small` (4 n bytes) as 24-bit
  // values (3 bytes each, four to three words) when every value is below 2^24, else as u32 when
  // every value fits 32 bits, else as they are into dst64; narrow_width(item) says which (3, 4 or
  // 8 bytes a value) once wait(item) has returned -- widen_dev expands the first two
  int add_narrow(uint32_t *small, uint64_t *dst64, const uint64_t *src, size_t n);
  int narrow_width(int item);
  void start();
  void wait(int item, hipStream_t s);
  void wait_all(hipStream_t s);

 private:
  struct Item {
    void *dst = nullptr;
    const void *src = nullptr;
    size_t bytes = 0;
    hipEvent_t ev = nullptr;
    bool narrow = false, done = false;
    int width = 8;  // bytes a value crossed PCIe as (narrow items)
    void *dst_wide = nullptr;
  };
  struct Job {  // one chunk of one item (or a whole small item: direct)
    int item;
    size_t off, cnt;  // source units: bytes, or u64 values for a narrow item
    bool direct;
  };
  struct ItemState {  // worker-side progress of an item
    std::atomic<size_t> left{0};
    std::atomic<bool> fits24{true}, fits32{true};
  };
  void run();
  void run_jobs();
  void work(int w, char *ring, std::atomic<size_t> &next, std::atomic<bool> &stop);
  hipError_t do_job(const Job &j, char *ring, int w, int &use);
  hipError_t finish_item(int k, char *ring, int w, int &use);
  hipError_t stage(char *ring, int w, int &use, void *dst, const void *src, size_t bytes);
  hipError_t stage_u32(char *ring, int w, int &use, uint32_t *dst, const uint64_t *src, size_t n);
  void mark_first();
  std::chrono::steady_clock::time_point t_start_, t_first_;
  std::atomic<bool> first_marked_{false};
  Ctx *c_;
  std::vector<Item> items_;
  std::vector<Job> jobs_;
  std::unique_ptr<ItemState[]> state_;
  std::thread th_;
  std::mutex mu_;
  std::condition_variable cv_;
  int queued_ = 0;
  bool done_ = false;
  hipError_t err_ = hipSuccess;
};

// RAII device guard + lock
struct CtxScope {
  Ctx *c;
  std::lock_guard<std::mutex> lk;
  explicit CtxScope(Ctx *ctx) : c(ctx), lk(ctx->mu) { TNS_HIP(hipSetDevice(ctx->device)); }
};

// `bytes` of a call's input on the device: resident input as it is, host input uploaded on
// c->stream into buf (the caller keeps buf until that stream has drained)
inline const void *on_device(Ctx *c, const void *in, size_t bytes, bool resident, DevBuf &buf) {
  if (resident) return in;
  void *p = buf.ensure(bytes ? bytes : 1);
  if (bytes) TNS_HIP(hipMemcpyAsync(p, in, bytes, hipMemcpyHostToDevice, c->stream));
  return p;
}

// ---- module entry points (device-resident pointers; all on ctx->stream) ----
// mle.hip
void mle_fold_dev(Ctx *c, const Fr *in, Fr *out, size_t half, const Fr &r);
Fr mle_evaluate_dev(Ctx *c, const Fr *evals, unsigned nv, const Fr *point_host);

// zero_folds.hip
// The single chain: binds the k tables at the challenges on stream st and writes their values to
// d_out.  flags (optional): the last table as 0/1 bytes (n_flags of them, zero beyond),
// tables[k - 1] unused -- only when sumcheck_folds_take_flag_bytes(nv).
bool sumcheck_folds_take_flag_bytes(unsigned nv);
void sumcheck_zero_folds_async(Ctx *c, hipStream_t st, Fr *const *tables, int k, unsigned nv, const Fr *chal_pinned,
                               Fr *d_out, const uint8_t *flags = nullptr, size_t n_flags = 0);
// The batched chain's inputs: up to two Fr tables of `rows` x N entries and, last, the op-type
// table as 0/1 bytes (n_flags a row, zero beyond).
struct FoldIn {
  const Fr *tab[2];
  const uint8_t *flags;
  size_t n_flags;
  int n_fr;  // Fr tables; the flag table (if any) is table n_fr
};
constexpr size_t FOLD_TAIL = 512;  // entries a block of the chain's last kernel binds in LDS
// all ntab tables of all `rows` proofs (2^nv = N entries each) bound at their proofs' challenges
// d_chal[b nv + k] into d_finals[b ntab + t]; f0 / f1: rows ntab N/2 and rows ntab N/4 entries of
// scratch (unused when N <= FOLD_TAIL)
void fold_batch(Ctx *c, const FoldIn &in, int ntab, size_t N, size_t rows, unsigned nv, const Fr *d_chal, Fr *f0, Fr *f1,
                Fr *d_finals);

// poly.hip
// q[i] = c[i+1] + z q[i+1] (synthetic division by x - z); returns P(z).  q may be null.
Fr synthetic_division_dev(Ctx *c, const Fr *coeffs, size_t n, const Fr &z, Fr *q);
// g1_powers[first .. first + n) = G * tau^i
void srs_generate_dev(Ctx *c, const Fr &tau, size_t first, size_t n, G1Affine *out);
void fr_fill_zero_dev(Ctx *c, Fr *p, size_t n);
// u64 entries [0, n_in) zero-padded to n: Montgomery form (mont), canonical form (canon,
// optional) and the largest bit length (*bits, zeroed here) in one pass on stream s
void u64_tables_dev(hipStream_t s, const uint64_t *in, size_t n_in, size_t n, Fr *mont, Fr *canon, unsigned *bits);
// out[i] = in[i] widened to u64 (addresses / indices that crossed PCIe as u32), on stream s
void widen_u32_dev(hipStream_t s, const uint32_t *in, size_t n, uint64_t *out);
// HostUpload narrow items: width 3 (packed 24-bit) or 4 (u32) -> u64 (width 8: nothing to do)
void widen_dev(hipStream_t s, const uint32_t *in, int width, size_t n, uint64_t *out);
// out[i] = G * s_i (affine), scalars canonical
void fixed_base_mul_dev(Ctx *c, const Fr *scalars_canon, size_t n, G1Affine *out);
void xyzz_to_affine_batch_dev(Ctx *c, const G1Xyzz *in, size_t n, G1Affine *out, Fq *prefix_scratch);

// interp.hip
void interpolate_consecutive_dev(Ctx *c, const Fr *y, size_t n, Fr *coeffs);
void factorial_tables_dev(Ctx *c, size_t nf, Fr *fact, Fr *ifact);

}  // namespace tns
