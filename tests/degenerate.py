"""Inputs of the degenerate-base MSM tests (test_gpu_degenerate.py, test_degenerate_cpu.py) and their
closed-form reference.  No GPU and no libtns here: integers, numpy and the C oracle's one scalar
multiplication.

Bases are B_i = k_i G with the multiplier k_i of row i drawn from a small set, so the points repeat,
negate each other and include the identity; the MSM of scalars c_i over them is
(sum_i c_i k_i mod r) G -- one integer sum and one double-and-add, independent of any Pippenger
structure.  Scalars are drawn over all of [0, r).
"""
import numpy as np

from oracle import coracle as co
from oracle import pyoracle as po

R = po.R_MOD

BASES = ("same", "pm", "small", "holes", "few")
SCALARS = ("uniform", "equal", "cancel", "narrow22", "flags", "one_hot", "edge")
# 2, 64: the one-thread-per-point kernel and its LDS tree; 65: the smallest sorted MSM; 777: several
# accumulation chunks, below the window-table threshold; 2^16: the smallest MSM over a window table
SIZES = (2, 64, 65, 777, 1 << 16)

EDGE = (0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 2**253 - 1, 2**253, 2**128 - 1, 2**128, 2**64 - 1, 2**64,
        2**22 - 1, 2**22, 2**21)


def _rand_fr(rng, n):
    raw = rng.bytes(32 * n)
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") % R for i in range(n)]


def _few_multipliers():
    a = _rand_fr(np.random.default_rng(0xFE3), 64)
    for j in range(8):
        a[2 * j + 1] = R - a[2 * j]
    return a


_BASES = {}


def base_family(name, n):
    """(multipliers, index): the distinct multipliers (ints mod r) of a family and, for each of the
    n rows, which of them it takes (numpy intp array)."""
    i = np.arange(n)
    if name == "same":
        return [1], np.zeros(n, dtype=np.intp)
    if name == "pm":
        return [1, R - 1], np.where(i % 3 == 0, 0, 1).astype(np.intp)
    if name == "small":  # (i % 5) - 1
        return [R - 1, 0, 1, 2, 3], (i % 5).astype(np.intp)
    if name == "holes":  # identity where i % 3 == 1, else 1 + i % 3
        return [1, 0, 3], (i % 3).astype(np.intp)
    if name == "few":
        if "few" not in _BASES:
            _BASES["few"] = _few_multipliers()
        return _BASES["few"], (i % 64).astype(np.intp)
    raise KeyError(name)


_POINTS = {}


def base_limbs(name, n):
    """The (n, 8) affine Montgomery limb rows of a family's first n points (identity = zeros): each
    distinct point by one oracle scalar multiplication, the rows by numpy indexing."""
    ks, idx = base_family(name, n)
    if name not in _POINTS:
        _POINTS[name] = np.stack([co.g1_to_limbs(co.g1_mul_gen(k)) for k in ks])
    return np.ascontiguousarray(_POINTS[name][idx])


_SCALARS = {}


def scalar_family(name, n):
    """n scalars as ints in [0, r); the same list for every base family (cached)."""
    key = (name, n)
    if key in _SCALARS:
        return _SCALARS[key]
    rng = np.random.default_rng([SCALARS.index(name), n])
    if name == "uniform":
        c = _rand_fr(rng, n)
    elif name == "equal":
        c = [R - 12345] * n
    elif name == "cancel":  # pairs s, r - s (an odd n leaves its last scalar unpaired)
        s = _rand_fr(rng, (n + 1) // 2)
        c = [s[i // 2] if i % 2 == 0 else (R - s[i // 2]) % R for i in range(n)]
    elif name == "narrow22":
        c = [int(x) for x in rng.integers(0, 1 << 22, size=n)]
    elif name == "flags":
        c = [int(x) for x in rng.integers(0, 2, size=n)]
    elif name == "one_hot":
        c = [0] * (n - 1) + [123456789]
    elif name == "edge":  # the signed-digit recoding's carry chains and window boundaries
        c = [EDGE[i % len(EDGE)] for i in range(n)]
    else:
        raise KeyError(name)
    _SCALARS[key] = c
    return c


def fr_mont(vals):
    """ints in [0, r) -> (n, 4) uint64 Montgomery limbs (arkworks' memory layout)."""
    raw = b"".join(((v << 256) % R).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype="<u8").reshape(-1, 4).astype(np.uint64)


_EXPECTED = {}


def expected_scalar(base, scalars, n):
    """sum_i c_i k_i mod r: the MSM is this multiple of G."""
    key = (base, scalars, n)
    if key not in _EXPECTED:
        ks, idx = base_family(base, n)
        acc = [0] * len(ks)
        for j, c in zip(idx.tolist(), scalar_family(scalars, n)):
            acc[j] += c
        _EXPECTED[key] = sum(a * k for a, k in zip(acc, ks)) % R
    return _EXPECTED[key]


def expected_point(base, scalars, n):
    return co.g1_mul_gen(expected_scalar(base, scalars, n))
