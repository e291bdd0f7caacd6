// nttprobe.hip -- the Fr transform engine (csrc/ntt.hip) and the factorial tables of
// csrc/interp.hip alone, for tests/test_gpu_ntt.py: each C entry point copies its input to the
// device, calls one shipped function (tns::ntt_twiddles, ntt_blocks, ntt_conv_blocks,
// factorial_tables_dev) on the context's stream, synchronises and copies the result out.  Nothing
// is re-implemented on the device: this file has no kernel, and libtns_nttprobe.so links libtns.so
// for every symbol it calls.  All data is (n, 4) u64 Montgomery limbs.
//
// Every entry point returns 0, a TNS_* status (every HIP error: TNS_ERR_DEVICE, the message in
// tns_last_error()), or -1 for arguments it does not take.
#include <hip/hip_runtime.h>

#include "abi.hpp"
#include "ntt.hpp"

namespace {

using namespace tns;

// the words of nttprobe_state's `info`, in order
enum { I_TWIDDLE_LOG, I_TWIDDLE_BYTES, I_PASS_TABLES, I_COUNT };

constexpr unsigned MAX_LOG = 24;  // the probe's own cap on a transform or a table: 2^24 elements

}  // namespace

extern "C" {

int nttprobe_info_words() { return I_COUNT; }

// out[0, 2^L) = the first 2^L entries of the table ntt_twiddles(c, L) returns (L <= 28 is the
// engine's limit: L = 29 is passed on, for its status)
int nttprobe_twiddles(tns_ctx *ctx, unsigned L, uint64_t *out) {
  if (!ctx || !out || (L > MAX_LOG && L <= 28)) return -1;
  return guarded([&]() {
    CtxScope g(&ctx->c);
    const Fr *tw = ntt_twiddles(&ctx->c, L);
    TNS_HIP(hipStreamSynchronize(ctx->c.stream));
    TNS_HIP(hipMemcpy(out, tw, sizeof(Fr) << L, hipMemcpyDeviceToHost));
    return TNS_OK;
  });
}

// out = ntt_blocks of x: nb contiguous transforms of size 2^s, forward or inverse
int nttprobe_blocks(tns_ctx *ctx, const uint64_t *x, unsigned s, uint64_t nb, int inverse, uint64_t *out) {
  if (!ctx || !x || !out || s > MAX_LOG || nb == 0 || nb > ((uint64_t)1 << (MAX_LOG - s))) return -1;
  return guarded([&]() {
    CtxScope g(&ctx->c);
    hipStream_t st = ctx->c.stream;
    const size_t total = (size_t)nb << s;
    DevBuf d_x;
    Fr *d = (Fr *)d_x.ensure(sizeof(Fr) * total);
    TNS_HIP(hipMemcpyAsync(d, x, sizeof(Fr) * total, hipMemcpyHostToDevice, st));
    ntt_blocks(&ctx->c, d, s, (size_t)nb, inverse != 0);
    TNS_HIP(hipStreamSynchronize(st));
    TNS_HIP(hipMemcpy(out, d, sizeof(Fr) * total, hipMemcpyDeviceToHost));
    return TNS_OK;
  });
}

// out = ntt_conv_blocks of x (nb blocks of 2^s) with the operand w (2^s entries)
int nttprobe_conv(tns_ctx *ctx, const uint64_t *x, unsigned s, uint64_t nb, const uint64_t *w, uint64_t *out) {
  if (!ctx || !x || !w || !out || s > MAX_LOG || nb == 0 || nb > ((uint64_t)1 << (MAX_LOG - s))) return -1;
  return guarded([&]() {
    CtxScope g(&ctx->c);
    hipStream_t st = ctx->c.stream;
    const size_t total = (size_t)nb << s, S = (size_t)1 << s;
    DevBuf d_x, d_w;
    Fr *d = (Fr *)d_x.ensure(sizeof(Fr) * total);
    Fr *dw = (Fr *)d_w.ensure(sizeof(Fr) * S);
    TNS_HIP(hipMemcpyAsync(d, x, sizeof(Fr) * total, hipMemcpyHostToDevice, st));
    TNS_HIP(hipMemcpyAsync(dw, w, sizeof(Fr) * S, hipMemcpyHostToDevice, st));
    ntt_conv_blocks(&ctx->c, d, s, (size_t)nb, dw);
    TNS_HIP(hipStreamSynchronize(st));
    TNS_HIP(hipMemcpy(out, d, sizeof(Fr) * total, hipMemcpyDeviceToHost));
    return TNS_OK;
  });
}

// fact[k] = k!, ifact[k] = 1 / k! for k < nf
int nttprobe_factorials(tns_ctx *ctx, uint64_t nf, uint64_t *fact, uint64_t *ifact) {
  if (!ctx || !fact || !ifact || nf == 0 || nf > ((uint64_t)1 << MAX_LOG)) return -1;
  return guarded([&]() {
    CtxScope g(&ctx->c);
    DevBuf d_f, d_i;
    Fr *f = (Fr *)d_f.ensure(sizeof(Fr) * nf);
    Fr *i = (Fr *)d_i.ensure(sizeof(Fr) * nf);
    factorial_tables_dev(&ctx->c, (size_t)nf, f, i);
    TNS_HIP(hipStreamSynchronize(ctx->c.stream));
    TNS_HIP(hipMemcpy(fact, f, sizeof(Fr) * nf, hipMemcpyDeviceToHost));
    TNS_HIP(hipMemcpy(ifact, i, sizeof(Fr) * nf, hipMemcpyDeviceToHost));
    return TNS_OK;
  });
}

// What the context holds of the engine's tables: info = Ctx::twiddle_log, the bytes of
// Ctx::twiddles, the number of entries in Ctx::pass_tw; keys = the first `cap` of their keys
// (lo << 8 | r), ascending.
int nttprobe_state(tns_ctx *ctx, int64_t *info, uint32_t *keys, uint64_t cap) {
  if (!ctx || !info || (cap && !keys)) return -1;
  return guarded([&]() {
    CtxScope g(&ctx->c);
    info[I_TWIDDLE_LOG] = ctx->c.twiddle_log;
    info[I_TWIDDLE_BYTES] = (int64_t)ctx->c.twiddles.bytes;
    info[I_PASS_TABLES] = (int64_t)ctx->c.pass_tw.size();
    uint64_t i = 0;
    for (const auto &kv : ctx->c.pass_tw) {
      if (i >= cap) break;
      keys[i++] = kv.first;
    }
    return TNS_OK;
  });
}

}  // extern "C"
