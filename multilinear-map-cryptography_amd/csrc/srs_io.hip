// srs_io.hip -- the two setup artefacts in ark-serialize 0.4 form, on the device: g1_powers and the
// Lagrange basis as `Vec<G1Affine>` (u64 LE count, then 32 bytes a point compressed or 64
// uncompressed; the point encoding of serialize.cpp).  A production SRS arrives as such a file and
// has no tau: decoding it costs one Fq square root a point, which is what runs here, one thread a
// point.  A stored Lagrange basis is attached to an SRS only after a randomised check against the
// SRS's powers (lagrange_basis_attach_dev).
#include <sys/random.h>

#include "abi.hpp"
#include "fq_sqrt.hpp"

namespace tns {

namespace {

constexpr uint32_t FLAG_NEG = 0x80000000u, FLAG_INF = 0x40000000u;  // in the encoding's last word

// why a point was refused (g1_deserialize's checks, in its order); 0 = fine
enum : unsigned { IO_FLAGS = 1, IO_X_RANGE = 2, IO_Y_RANGE = 3, IO_NO_ROOT = 4, IO_OFF_CURVE = 5 };
const char *const kReason[] = {"",
                               "invalid G1 flags",
                               "G1 x not below the field modulus",
                               "G1 y not below the field modulus",
                               "G1 x is not on the curve",
                               "G1 point not on the curve"};
// the status word: (index << 3 | reason) of the lowest refused index, all ones while none is
constexpr unsigned long long IO_OK = ~0ull;

__device__ __forceinline__ bool lt_modulus_dev(const Fq &x) {  // x < p as integers
  bool lt = false;
#pragma unroll
  for (int i = 0; i < 8; i++) lt = x.v[i] < FqCfg::M[i] || (x.v[i] == FqCfg::M[i] && lt);
  return lt;
}

// "y > -y as canonical integers" (ark-ec to_flags; serialize.cpp y_negative): yc > p - yc
__device__ __forceinline__ bool y_negative_dev(const Fq &y_mont) {
  const Fq yc = from_mont(y_mont);
  if (yc.is_zero()) return false;
  bool gt = false;
  u64 br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const u64 d = (u64)FqCfg::M[i] - yc.v[i] - br;
    br = (d >> 32) & 1;
    const u32 ny = (u32)d;
    gt = yc.v[i] > ny || (yc.v[i] == ny && gt);
  }
  return gt;
}

__device__ __forceinline__ void io_fail(unsigned long long *status, size_t index, unsigned reason) {
  atomicMin(status, ((unsigned long long)index << 3) | reason);
}

__device__ __forceinline__ Fq load_words(const uint4 *p) {
  const uint4 lo = p[0], hi = p[1];
  Fq r;
  r.v[0] = lo.x, r.v[1] = lo.y, r.v[2] = lo.z, r.v[3] = lo.w;
  r.v[4] = hi.x, r.v[5] = hi.y, r.v[6] = hi.z, r.v[7] = hi.w;
  return r;
}
__device__ __forceinline__ void store_words(uint4 *p, const Fq &a) {
  p[0] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
  p[1] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
}

// Wire bytes -> G1Affine (Montgomery), one thread a point, with exactly g1_deserialize's checks
// (serialize.cpp): flags in the top two bits of the encoding's last byte, both set refused,
// infinity = the all-zero pair, x (and y) below the modulus, compressed y = (x^3 + 3)^((p+1)/4)
// accepted only if it squares back and negated when its sign disagrees with the flag,
// uncompressed points checked against the curve equation.  A refused point leaves zeros and
// records (base + i, reason) in *status, the lowest index winning.  `in` is 16-byte aligned.
template <bool COMPRESSED>
__global__ void __launch_bounds__(256) k_g1_decode(const uint4 *__restrict__ in, size_t n, size_t base,
                                                   G1Affine *__restrict__ out, unsigned long long *status) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  constexpr int Q = COMPRESSED ? 2 : 4;  // uint4 a point
  Fq x = load_words(in + Q * i), y = Fq::zero();
  if (!COMPRESSED) y = load_words(in + Q * i + 2);
  u32 &last = COMPRESSED ? x.v[7] : y.v[7];
  const u32 flags = last & (FLAG_NEG | FLAG_INF);
  last &= ~(FLAG_NEG | FLAG_INF);
  G1Affine P;
  P.x = Fq::zero();
  P.y = Fq::zero();
  unsigned bad = 0;
  if (flags == (FLAG_NEG | FLAG_INF)) {
    bad = IO_FLAGS;
  } else if (flags & FLAG_INF) {
    // identity: the coordinates are not read (as on the host)
  } else if (!lt_modulus_dev(x)) {
    bad = IO_X_RANGE;
  } else if (COMPRESSED) {
    const Fq xm = to_mont(x);
    const Fq rhs = add(mul(sqr(xm), xm), from_u64<FqCfg>(3));
    Fq r = fq_sqrt_candidate_dev(rhs);
    if (!(sqr(r) == rhs)) {
      bad = IO_NO_ROOT;
    } else {
      if (y_negative_dev(r) != ((flags & FLAG_NEG) != 0)) r = neg(r);
      P.x = xm;
      P.y = r;
    }
  } else if (!lt_modulus_dev(y)) {
    bad = IO_Y_RANGE;
  } else {
    G1Affine t;
    t.x = to_mont(x);
    t.y = to_mont(y);
    if (!g1_on_curve(t)) bad = IO_OFF_CURVE;
    else P = t;
  }
  if (bad) io_fail(status, base + i, bad);
  uint4 *o = reinterpret_cast<uint4 *>(out + i);
  store_words(o, P.x);
  store_words(o + 2, P.y);
}

// G1Affine (Montgomery) -> wire bytes, g1_serialize (serialize.cpp) one thread a point.
template <bool COMPRESSED>
__global__ void __launch_bounds__(256) k_g1_encode(const G1Affine *__restrict__ in, size_t n, uint4 *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  constexpr int Q = COMPRESSED ? 2 : 4;
  const uint4 *p = reinterpret_cast<const uint4 *>(in + i);
  G1Affine P;
  P.x = load_words(p);
  P.y = load_words(p + 2);
  Fq x = Fq::zero(), y = Fq::zero();
  u32 flags = FLAG_INF;
  if (!P.is_inf()) {
    x = from_mont(P.x);
    y = from_mont(P.y);
    flags = y_negative_dev(P.y) ? FLAG_NEG : 0;
  }
  (COMPRESSED ? x : y).v[7] |= flags;
  store_words(out + Q * i, x);
  if (!COMPRESSED) store_words(out + Q * i + 2, y);
}

// points a chunk: the wire bytes cross in pieces of at most 128 MiB through one device buffer, so
// neither side holds a second copy of a 0.5 GB file
constexpr size_t IO_CHUNK = (size_t)1 << 21;

}  // namespace

size_t g1_vec_serialized_size(size_t n, bool compressed) { return 8 + n * (compressed ? 32 : 64); }

// n points of wire bytes (host) -> out (device); throws naming the lowest refused index
void g1_decode_dev(Ctx *c, const uint8_t *bytes, size_t n, bool compressed, G1Affine *out) {
  if (n == 0) return;
  hipStream_t st = c->stream;
  const size_t sz = compressed ? 32 : 64, chunk = std::min(n, IO_CHUNK);
  DevBuf wire, stat;
  uint8_t *dw = (uint8_t *)wire.ensure(chunk * sz);
  unsigned long long *ds = (unsigned long long *)stat.ensure(sizeof(unsigned long long));
  TNS_HIP(hipMemsetAsync(ds, 0xff, sizeof(unsigned long long), st));
  for (size_t off = 0; off < n; off += chunk) {
    const size_t m = std::min(chunk, n - off);
    TNS_HIP(hipMemcpyAsync(dw, bytes + off * sz, m * sz, hipMemcpyHostToDevice, st));
    TNS_PROF(c, "g1_decode", (double)(m * (sz + sizeof(G1Affine))));
    const unsigned grid = (unsigned)((m + 255) / 256);
    if (compressed)
      k_g1_decode<true><<<grid, 256, 0, st>>>((const uint4 *)dw, m, off, out + off, ds);
    else
      k_g1_decode<false><<<grid, 256, 0, st>>>((const uint4 *)dw, m, off, out + off, ds);
    TNS_LAUNCH_CHECK();
  }
  unsigned long long s = IO_OK;
  TNS_HIP(hipMemcpyAsync(&s, ds, sizeof s, hipMemcpyDeviceToHost, st));
  TNS_HIP(hipStreamSynchronize(st));
  if (s != IO_OK) {
    const unsigned reason = (unsigned)(s & 7);
    throw Error(TNS_ERR_INVALID_PARAMETERS,
                "G1 point " + std::to_string(s >> 3) + ": " + kReason[reason < 6 ? reason : 0]);
  }
}

// n points (device) -> wire bytes (host)
void g1_encode_dev(Ctx *c, const G1Affine *pts, size_t n, bool compressed, uint8_t *bytes) {
  if (n == 0) return;
  hipStream_t st = c->stream;
  const size_t sz = compressed ? 32 : 64, chunk = std::min(n, IO_CHUNK);
  DevBuf wire;
  uint8_t *dw = (uint8_t *)wire.ensure(chunk * sz);
  for (size_t off = 0; off < n; off += chunk) {
    const size_t m = std::min(chunk, n - off);
    {
      TNS_PROF(c, "g1_encode", (double)(m * (sz + sizeof(G1Affine))));
      const unsigned grid = (unsigned)((m + 255) / 256);
      if (compressed)
        k_g1_encode<true><<<grid, 256, 0, st>>>(pts + off, m, (uint4 *)dw);
      else
        k_g1_encode<false><<<grid, 256, 0, st>>>(pts + off, m, (uint4 *)dw);
      TNS_LAUNCH_CHECK();
    }
    TNS_HIP(hipMemcpyAsync(bytes + off * sz, dw, m * sz, hipMemcpyDeviceToHost, st));
    TNS_HIP(hipStreamSynchronize(st));  // the buffer is rewritten by the next chunk
  }
}

// The header of a Vec<G1Affine> file: its count, with len required to be exactly the size the
// count implies (truncated and trailing bytes both refused).
size_t g1_vec_header(const uint8_t *in, size_t len, bool compressed) {
  if (!in || len < 8) throw Error(TNS_ERR_INVALID_PARAMETERS, "truncated G1 vector bytes (no length header)");
  uint64_t n = 0;
  for (int i = 0; i < 8; i++) n |= (uint64_t)in[i] << (8 * i);
  const size_t sz = compressed ? 32 : 64;
  if (n > (len - 8) / sz || len != 8 + (size_t)n * sz)
    throw Error(TNS_ERR_INVALID_PARAMETERS, "G1 vector bytes: " + std::to_string(len) + " bytes do not match the header's " +
                                                std::to_string(n) + " points");
  return (size_t)n;
}

void g1_vec_put_header(size_t n, uint8_t *out) {
  for (int i = 0; i < 8; i++) out[i] = (uint8_t)((uint64_t)n >> (8 * i));
}

// Attach a stored Lagrange basis ([L_j(tau)]G, j < N, wire bytes) to an SRS that holds
// g1_powers[0..N) -- without tau, so the basis is checked against the powers first: for N scalars
// r from the seed (tns_fr_rand_batch's stream) and the coefficients c of r's interpolant on the
// nodes 0..N-1, sum_j r_j B_j must equal sum_i c_i g1_powers[i].  Both are [sum_j r_j L_j(tau)]G
// for the true basis; points B with B_j != [L_j(tau)]G for some j make the difference
// sum_j r_j (B_j - [L_j(tau)]G) a non-zero linear form in r, which vanishes for a fraction 1/|Fr|
// of the r -- so r must not be known to whoever wrote the file (seed == NULL: 32 bytes from the
// OS).  On success the basis enters srs.lagrange under (N, 0, N), where
// lagrange_basis_from_powers_dev puts its own, with its window table from N = 2^12; a basis
// already cached there is kept (the file is still decoded and checked).
void lagrange_basis_attach_dev(Ctx *c, const Srs &srs, const uint8_t *bytes, size_t N, bool compressed,
                               const uint8_t seed_in[32]) {
  if (N == 0 || (N & (N - 1))) throw Error(TNS_ERR_INVALID_PARAMETERS, "Lagrange basis size must be a power of two");
  if (N > ((size_t)1 << 28)) throw Error(TNS_ERR_INVALID_PARAMETERS, "Lagrange basis larger than 2^28");
  if (srs.first != 0 || srs.held < N)
    throw Error(TNS_ERR_INVALID_PARAMETERS, "the basis of N nodes needs g1_powers[0..N) (an unsharded SRS)");
  uint8_t seed[32];
  if (seed_in) {
    std::memcpy(seed, seed_in, 32);
  } else if (getrandom(seed, 32, 0) != 32) {
    throw Error(TNS_ERR_DEVICE, "no randomness from the OS for the Lagrange basis check");
  }
  hipStream_t st = c->stream;
  auto basis = std::make_unique<LagrangeBasis>();
  try {
    G1Affine *pts = (G1Affine *)basis->points.ensure(sizeof(G1Affine) * N);
    g1_decode_dev(c, bytes, N, compressed, pts);
    std::vector<Fr> r(N);
    host_fr_rand_stream(seed, N, r.data());
    DevBuf rb, cb;
    Fr *dr = (Fr *)rb.ensure(sizeof(Fr) * N), *dc = (Fr *)cb.ensure(sizeof(Fr) * N);
    TNS_HIP(hipMemcpyAsync(dr, r.data(), sizeof(Fr) * N, hipMemcpyHostToDevice, st));
    interpolate_consecutive_dev(c, dr, N, dc);
    const G1Affine lhs = xyzz_to_affine(msm_dev(c, pts, dr, N));
    const G1Affine rhs = commit_dev(c, srs, dc, N);
    if (!(lhs.x == rhs.x) || !(lhs.y == rhs.y))
      throw Error(TNS_ERR_INVALID_PARAMETERS, "Lagrange basis does not match g1_powers");
    const auto key = std::make_tuple(N, (size_t)0, N);
    if (srs.lagrange.count(key)) return;
    if (N >= ((size_t)1 << 12)) basis->fb = fixed_base_try_build(c, pts, N);
    TNS_HIP(hipStreamSynchronize(st));
    srs.lagrange[key] = std::move(basis);
  } catch (...) {
    (void)hipStreamSynchronize(st);  // nothing queued may outlive the buffers freed here
    throw;
  }
}

}  // namespace tns
