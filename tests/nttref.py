"""A plain-integer reference for the Fr transform engine (csrc/ntt.hip, ntt.hpp) and the factorial
tables of csrc/interp.hip, for tests/test_gpu_ntt.py.  Everything is Python big integers mod r:
nothing here calls the library or does arithmetic in numpy.  oracle.pyoracle gives r, and
oracle.coracle the Montgomery limb conversions of the arrays that cross to the device.

Conventions (ntt.hpp): the forward transform is decimation in frequency, natural order in,
bit-reversed out; the inverse is decimation in time, bit-reversed in, natural order out, unscaled.
The twiddle table is stage-major: TW[h + k] = w_{2h}^k for h = 2^lh, k < h, and TW[0] = 1.
tests/test_nttref_cpu.py proves this module against an O(n^2) DFT and schoolbook products."""
import numpy as np

from oracle import coracle as co
from oracle import pyoracle as po

R = po.R_MOD
TWO_ADICITY = 28
ROOT_2_28 = pow(5, (R - 1) >> TWO_ADICITY, R)  # of exact order 2^28
EDGES = (0, 1, R - 1, R - 2, (R - 1) // 2)

TILE_LOG = 10   # ntt.hip: the contiguous LDS tile runs the 10 smallest strides
PASS_RMAX = 5   # ... and one strided pass at most 5 stages


def root(log_order):
    """the primitive 2^log_order-th root of unity the engine uses"""
    assert 0 <= log_order <= TWO_ADICITY
    x = ROOT_2_28
    for _ in range(TWO_ADICITY - log_order):
        x = x * x % R
    return x


def twiddle_table(L):
    tw = [1] * (1 << L)
    for lh in range(L):
        h, w, p = 1 << lh, root(lh + 1), 1
        for k in range(h):
            tw[h + k] = p
            p = p * w % R
    return tw


def log2_exact(n):
    s = n.bit_length() - 1
    assert n == 1 << s, "a power of two"
    return s


def bitrev(i, s):
    return int(format(i, "0%db" % s)[::-1], 2) if s else 0


def bitrev_permute(x):
    s = log2_exact(len(x))
    return [x[bitrev(i, s)] for i in range(len(x))]


def dft_naive(x):
    """X[k] = sum_j x[j] w^(j k), natural order, O(n^2)"""
    n = len(x)
    w = root(log2_exact(n))
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * w % R
    return [sum(x[j] * pw[j * k % n] for j in range(n)) % R for k in range(n)]


def forward(x):
    """the textbook in-place DIF: stage h = n/2 .. 1 with the root w_{2h}; natural in, bit-reversed out"""
    x = list(x)
    n = len(x)
    h = n >> 1
    while h >= 1:
        w = root(log2_exact(2 * h))
        tw = [1] * h
        for k in range(1, h):
            tw[k] = tw[k - 1] * w % R
        for i in range(0, n, 2 * h):
            for k in range(h):
                a, b = x[i + k], x[i + k + h]
                x[i + k] = (a + b) % R
                x[i + k + h] = (a - b) * tw[k] % R
        h >>= 1
    return x


def _dft_recursive(x, w):
    """natural in, natural out, by the even / odd split: X[j] = E[j] + w^j O[j], X[j + n/2] = E[j] - w^j O[j]"""
    n = len(x)
    if n == 1:
        return list(x)
    w2 = w * w % R
    E, O = _dft_recursive(x[0::2], w2), _dft_recursive(x[1::2], w2)
    out = [0] * n
    p, half = 1, n >> 1
    for j in range(half):
        t = p * O[j] % R
        out[j] = (E[j] + t) % R
        out[j + half] = (E[j] - t) % R
        p = p * w % R
    return out


def inverse(x):
    """bit-reversed in, natural out, unscaled: x[j] = sum_k X[k] w^(-j k).  Not `forward` run
    backwards: the input is put into natural order and transformed by the recursive even / odd
    split with the inverse root."""
    n = len(x)
    w_inv = pow(root(log2_exact(n)), R - 2, R)
    return _dft_recursive(bitrev_permute(list(x)), w_inv)


def schoolbook_cyclic(x, k):
    n = len(x)
    assert len(k) == n
    out = [0] * n
    for i, a in enumerate(x):
        if a:
            for j, b in enumerate(k):
                out[(i + j) % n] += a * b
    return [v % R for v in out]


def cyclic_conv(x, k):
    n = len(x)
    assert len(k) == n
    if n <= 64:
        return schoolbook_cyclic(x, k)
    X, K = forward(x), forward(k)
    n_inv = pow(n, R - 2, R)
    return [v * n_inv % R for v in inverse([a * b % R for a, b in zip(X, K)])]


def conv_operand(k, s):
    """what ntt_conv_blocks takes as w: the forward transform of k zero-padded to 2^s (bit-reversed
    order), scaled by 2^-s"""
    n = 1 << s
    assert len(k) <= n
    scale = pow(n, R - 2, R)
    return [v * scale % R for v in forward(list(k) + [0] * (n - len(k)))]


def factorials(nf):
    """(fact, inv_fact): k! and 1 / k! mod r for k < nf"""
    fact = [1] * nf
    for k in range(1, nf):
        fact[k] = fact[k - 1] * k % R
    return fact, [pow(f, R - 2, R) for f in fact]


def pass_split(s):
    """The strided passes of a size-2^s transform as (lo, r), low to high: the stages [10, s) in
    ceil((s - 10) / 5) passes, as even as possible, the larger ones at the low end."""
    stages = s - TILE_LOG
    if stages <= 0:
        return []
    count = -(-stages // PASS_RMAX)
    small, larger = divmod(stages, count)
    out, lo = [], TILE_LOG
    for p in range(count):
        r = small + 1 if p < larger else small
        out.append((lo, r))
        lo += r
    assert lo == s
    return out


def pass_key(lo, r):
    return lo << 8 | r


def rand_vec(rng, n):
    """n random residues with the edge values 0, 1, r-1, r-2 and (r-1)/2 at random places (as many as fit)"""
    v = [rng.randrange(R) for _ in range(n)]
    for e, i in zip(EDGES, rng.sample(range(n), min(n, len(EDGES)))):
        v[i] = e
    return v


def to_limbs(vals):
    return co.fr_array(vals)


def from_limbs(arr):
    return co.fr_ints(np.asarray(arr))
