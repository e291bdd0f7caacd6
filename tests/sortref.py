"""Plain-integer reference of the MSM's bucket sort (csrc/bucket_sort.hip), restating the contract in
scalar_digits' comment, vectorised over the scalars with numpy on four u64 limbs (the carry is
sequential in the window index only):

  signed c-bit digits   val = raw + carry; the digit is val - 2^c with a carry out iff val > 2^(c-1),
                        else val; zero digits are dropped
  per-window layout     key = w << (c-1) | (|d| - 1),  value = i | sign << 31,  bucket = key
  shared layout         key = (|d| - 1) << wb | w,     value = (w stride + i) | sign << 31,
                        bucket = |d| - 1; inside a bucket the entries come window by window

The device order is compared as one sorted u64 word per entry, bucket << 32 | value: equal arrays
mean every bucket holds the same multiset of values.  test_sortref_cpu.py proves this file on its
own; test_gpu_bucket_sort.py compares the device with it.  PLANS and families() are the cases both
use."""
import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
SIGN = 1 << 31
# the compile-time pass-1 shapes of msm_plan.hpp (kPass1Shapes): (c, W) -> scalars per thread
CT_PLANS = {(22, 12): 3, (20, 13): 3, (19, 14): 3, (17, 15): 3, (16, 2): 16, (12, 2): 16}


def to_limbs(vals):
    """ints < 2^256 -> (n, 4) u64, little-endian limbs"""
    raw = b"".join(int(v).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype=np.uint64).reshape(len(vals), 4).copy()


def from_limbs(limbs):
    raw = np.ascontiguousarray(limbs, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(limbs))]


def u64_to_limbs(u):
    out = np.zeros((len(u), 4), dtype=np.uint64)
    out[:, 0] = u
    return out


def raw_window(limbs, bit, c):
    """bits [bit, bit + c) of every scalar (zero above bit 255), as int64"""
    n = limbs.shape[0]
    l, sh = bit >> 6, bit & 63
    if l >= 4:
        return np.zeros(n, dtype=np.int64)
    x = limbs[:, l] >> np.uint64(sh)
    if sh + c > 64 and l + 1 < 4:
        x = x | (limbs[:, l + 1] << np.uint64(64 - sh))
    return (x & np.uint64((1 << c) - 1)).astype(np.int64)


def digits(limbs, c, W):
    """signed digits d[w][i] (int64, W rows) and the carry out of the top window"""
    half = 1 << (c - 1)
    carry = np.zeros(limbs.shape[0], dtype=np.int64)
    out = []
    for w in range(W):
        val = raw_window(limbs, w * c, c) + carry
        neg = val > half
        out.append(np.where(neg, val - (1 << c), val))
        carry = neg.astype(np.int64)
    return out, carry


def wb_of(W, shared):
    wb = 0
    if shared:
        while (1 << wb) < W:
            wb += 1
    return wb


def bucket_bits_of(c, W, shared):
    """what msm_plan.hpp's finish_plan hands the sort: wbits + c - 1 (shared: one bucket set)"""
    wbits = 0
    if not shared:
        while (1 << wbits) < W:
            wbits += 1
    return wbits + c - 1


def entries(limbs, c, W, shared, stride):
    """(bucket << 32 | value) of every non-zero digit, sorted: the order's contract as one array"""
    n = limbs.shape[0]
    d, _ = digits(limbs, c, W)
    idx = np.arange(n, dtype=np.uint64)
    parts = []
    for w in range(W):
        nz = np.nonzero(d[w])[0]
        dw = d[w][nz]
        mag1 = (np.abs(dw) - 1).astype(np.uint64)
        sign = np.where(dw < 0, np.uint64(SIGN), np.uint64(0))
        if shared:
            bucket = mag1
            value = (np.uint64(w * stride) + idx[nz]) | sign
        else:
            bucket = np.uint64(w << (c - 1)) | mag1
            value = idx[nz] | sign
        parts.append((bucket << np.uint64(32)) | value)
    out = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)
    out.sort()
    return out


# ---------------------------------------------------------------- the window planner
# csrc/msm_plan.hpp's cost model restated (test_msm_plan_cpu.py compares the header with it,
# test_gpu_msm_plan_grid.py the plans the device took).  The costs are integers below 2^53, so
# the products with `tie` are the doubles the header computes.
def windows_for(bits, c):
    """signed c-bit windows of `bits`-bit scalars: the top window's raw value must stay <= 2^(c-1)"""
    W = -(-bits // c)
    return W + 1 if bits - c * (W - 1) > c - 1 else W


def plan_cost(n, W, c, sets):
    return W * n + 3 * sets * (1 << (c - 1))


def best_window(n, bits, cmax, shared, w1max=0, tie=0.98):
    lg, best, bc = (n - 1).bit_length(), 1e300, 4
    for c in range(4, min(cmax, lg + 2) + 1):
        W = windows_for(bits, c)
        cost = plan_cost(n, W, c, 1 if shared else W)
        if cost < best * tie:
            best, bc = cost, c
    c1 = bits + 1
    return c1 if cmax < c1 <= min(w1max, lg + 2) and plan_cost(n, 1, c1, 1) < best * tie else bc


def table_shape(n):
    """(n, c, W) of the fixed-base window table over n points"""
    c = best_window(n, 254, 22, True, 0, 1.0)
    return n, c, windows_for(254, c)


def plan_msm(n, bits, table=None, fb_off=0, tables=True):
    """(c, W, bucket_bits, shared) of an MSM of n points by `bits`-bit scalars, and the stride"""
    c = best_window(n, bits, 20, False, 23)
    W, shared, stride = windows_for(bits, c), False, 0
    if table and tables and table[0] >= fb_off + n and table[0] * table[2] < 1 << 31:
        Ws = windows_for(bits, table[1])
        if Ws <= table[2] and plan_cost(n, Ws, table[1], 1) < plan_cost(n, W, c, W):
            c, W, shared, stride = table[1], Ws, True, table[0]
    return (c, W, bucket_bits_of(c, W, shared), shared), stride


# ---------------------------------------------------------------- the cases
class Plan:
    """One sort geometry of the MSM planner: (c, W, layout) at n scalars of up to `bits` bits."""

    def __init__(self, name, c, W, n, bits, shared=False, stride=0, route=None):
        self.name, self.c, self.W, self.n, self.bits = name, c, W, n, bits
        self.shared, self.stride = shared, stride if shared else 0
        self.route = route or {}
        self.bucket_bits = bucket_bits_of(c, W, shared)
        self.wb = wb_of(W, shared)

    def __repr__(self):
        return self.name

    @property
    def spb(self):
        """scalars per pass-1 tile"""
        spb = 8192 // self.W
        if (self.c, self.W) in CT_PLANS:
            spb = min(spb, 256 * CT_PLANS[(self.c, self.W)])
        return spb


# `bits`: the widest scalars whose window count for c is W (windows_for; test_sortref_cpu.py checks it).
# route: what the probe must report for the plan (test_gpu_bucket_sort.py asserts it).
PLANS = [
    Plan("pw_c4_W1_n65", 4, 1, 65, 3, route=dict(npass=1, bits=[3], keys=1, ct=0)),
    Plan("pw_c4_W1_n300", 4, 1, 300, 3, route=dict(npass=1, bits=[3], keys=1, ct=0)),
    Plan("pw_c6_W3_n65", 6, 3, 65, 17, route=dict(npass=1, bits=[7], keys=1, ct=0)),
    Plan("pw_c6_W3_n300", 6, 3, 300, 17, route=dict(npass=1, bits=[7], keys=1, ct=0)),
    # (51 windows need 6 window bits: 10-bit keys, which one 9-bit pass cannot sort -- a 2-bin pass 1)
    Plan("pw_c5_W51_n65", 5, 51, 65, 254, route=dict(npass=2, bits=[1, 9], kf=[1], pk=0, vo=1, keys=0, ct=0)),
    Plan("pw_c5_W51_n300", 5, 51, 300, 254, route=dict(npass=2, bits=[1, 9], kf=[1], pk=0, vo=1, keys=0, ct=0)),
    Plan("pw_c7_W37_n1000", 7, 37, 1000, 254, route=dict(npass=2, bits=[3, 9], kf=[1], pk=0, vo=1, keys=0, ct=0)),
    Plan("pw_c12_W22_n5000", 12, 22, 5000, 254, route=dict(npass=2, bits=[7, 9], kf=[1], pk=0, vo=1, keys=0, ct=0)),
    Plan("sh_c17_W4_n5000", 17, 4, 5000, 67, shared=True, stride=7001,
         route=dict(npass=2, bits=[9, 9], kf=[1], pk=0, vo=1, keys=0, ct=0, big=0)),
    Plan("pw_c16_W2_n12289", 16, 2, 12289, 31, route=dict(npass=2, bits=[7, 9], kf=[1], pk=0, vo=1, keys=0, ct=1)),
    Plan("pw_c12_W2_n12289", 12, 2, 12289, 23, route=dict(npass=2, bits=[3, 9], kf=[1], pk=0, vo=1, keys=0, ct=1)),
    Plan("pw_c15_W17_n16385", 15, 17, (1 << 14) + 1, 254,
         route=dict(npass=3, bits=[5, 5, 9], kf=[0, 0], pk=1, vo=1, keys=0, ct=0, big=0)),
    Plan("sh_c20_W13_n3000", 20, 13, 3000, 254, shared=True, stride=4099,
         route=dict(npass=3, bits=[7, 7, 9], kf=[0, 0], pk=1, vo=1, keys=0, ct=1, big=0)),
    Plan("sh_c19_W14_n3000", 19, 14, 3000, 254, shared=True, stride=4099,
         route=dict(npass=3, bits=[7, 6, 9], kf=[0, 0], pk=1, vo=1, keys=0, ct=1, big=0)),
    Plan("sh_c17_W15_n3000", 17, 15, 3000, 254, shared=True, stride=4099,
         route=dict(npass=3, bits=[6, 5, 9], kf=[0, 0], pk=1, vo=1, keys=0, ct=1, big=0)),
    # 25-bit keys: the pass over 2^16 segments takes the multi-level geometry route (k_bs_tiles + two
    # exclusive_scans).  bucket_sort_begin sizes its buffers by the key width, not by n: about 1 GB
    # of segment, tile and count workspaces for these 6000 scalars
    Plan("sh_c22_W12_n6000", 22, 12, 6000, 254, shared=True, stride=6151,
         route=dict(npass=3, bits=[8, 8, 9], kf=[0, 0], pk=1, vo=1, keys=0, ct=1, big=1)),
]
# n > 2^22: the point index needs 23 bits, which leaves no room for the packed tail.  The table's
# full-width plan over scalars of at most 40 bits (MsmArgs::plan_bits: the windows above carry no
# digits), read as u64
BIG_PLAN = Plan("sh_c22_W12_n4194305", 22, 12, (1 << 22) + 1, 254, shared=True, stride=(1 << 22) + 1,
                route=dict(npass=3, bits=[8, 8, 9], kf=[0, 1], pk=0, vo=1, keys=0, ct=1, big=1, ibits=23))


def rand_exact(rng, bits, n):
    """n ints of exactly `bits` bits, below R"""
    lo = 1 << (bits - 1)
    hi = min(1 << bits, R)
    out = []
    for row in rng.integers(0, 1 << 63, size=(n, 5), dtype=np.uint64):
        x = 0
        for v in row:
            x = (x << 63) | int(v)
        out.append(lo + x % (hi - lo))
    return out


def families(plan, rng, n=None):
    """name -> n ints (canonical scalars, < 2^256) for every scalar family of the plan"""
    c, W, bits = plan.c, plan.W, plan.bits
    n = n or plan.n
    half = 1 << (c - 1)
    top_bits = bits - c * (W - 1)  # the top window's raw width
    rnd = rand_exact(rng, bits, n)
    fam = {"random": rnd}
    fam["last_only"] = [0] * (n - 1) + [rnd[-1]]
    if W >= 2:  # (a one-window plan has c = bits + 1: its raw window stays below 2^(c-1))
        fam["top_bucket"] = [sum(half << (c * w) for w in range(W - 1))] * n
        fam["neg_carry"] = [sum((half + 1) << (c * w) for w in range(W - 1))] * n
    fam["all_ones"] = [(1 << bits) - 1] * n
    fam["top_only"] = [(1 + (7919 * i) % ((1 << top_bits) - 1 or 1)) << (c * (W - 1)) for i in range(n)]
    if bits == 254:
        fam["r_minus_1"] = [R - 1] * n
        fam["r_minus_12345"] = [R - 12345] * n
    fam["repeated"] = [rnd[0]] * n
    a, b = rnd[1 % n], rnd[2 % n]
    fam["two_heavy"] = [a if i % 3 == 0 else b if i % 3 == 1 else rnd[i] for i in range(n)]
    return fam
