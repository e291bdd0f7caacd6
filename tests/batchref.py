"""Plain-integer restatement of the batched MSM's digit contract (csrc/bucket_sort.hip scalar_digits
with ROWS, csrc/msm_batch_plan.hpp), on top of sortref's single-MSM digits:

  a batch of B rows of n scalars is one array of B n scalars; entry e = b n + i is row b's scalar of
  point i.  With signed windows of c bits and W windows (sortref.digits), every non-zero digit d of
  window w gives
      key   = (b W + w) << (c - 1) | (|d| - 1)        bucket set b W + w, B W sets in all
      value = i | sign << 31                          the point index wraps per row

and the route rule / group split of plan_batch.  test_msm_batch_plan_cpu.py proves the digits
against big integers and the header against the rule; the GPU tests use the windows to build their
edge-case rows."""
import numpy as np

import sortref

SIGN = 1 << 31
ENTRY_LIMIT = 1 << 31
KEY_BITS = 31
WS_CAP = 1 << 30
MAX_SCALARS = 1 << 32
ROUTE_ROWS, ROUTE_BATCHED = 0, 1


def ceil_log2(x):
    return max(x - 1, 0).bit_length()


def batch_window(n, bits):
    """the window of ONE row's per-window optimum (plan_msm's), shared by the rows of a batch"""
    c = sortref.best_window(n, bits, 20, False, 23)
    return c, sortref.windows_for(bits, c)


def batch_entries(limbs, n, c, W):
    """limbs: (B n, 4) canonical scalars, row-major.  (key, value) of every non-zero digit, in entry
    order e then w, and the B W bucket-set populations."""
    total = limbs.shape[0]
    assert n > 0 and total % n == 0
    B = total // n
    d, carry = sortref.digits(limbs, c, W)
    assert not carry.any(), "the top window carried out: W too small for these scalars"
    e = np.arange(total, dtype=np.uint64)
    b, i = e // np.uint64(n), e % np.uint64(n)
    keys, vals = [], []
    for w in range(W):
        nz = np.nonzero(d[w])[0]
        dw = d[w][nz]
        mag1 = (np.abs(dw) - 1).astype(np.uint64)
        sets = b[nz] * np.uint64(W) + np.uint64(w)
        keys.append((sets << np.uint64(c - 1)) | mag1)
        vals.append(i[nz] | np.where(dw < 0, np.uint64(SIGN), np.uint64(0)))
    keys = np.concatenate(keys) if keys else np.zeros(0, dtype=np.uint64)
    vals = np.concatenate(vals) if vals else np.zeros(0, dtype=np.uint64)
    pop = np.bincount((keys >> np.uint64(c - 1)).astype(np.int64), minlength=B * W)
    return keys, vals, pop


def scalars_from_entries(keys, vals, B, n, c, W):
    """the scalars the entries spell: sum over a (row, point)'s digits of sign |d| 2^(c w), big integers"""
    out = [[0] * n for _ in range(B)]
    half_mask = (1 << (c - 1)) - 1
    for k, v in zip(keys.tolist(), vals.tolist()):
        s, mag = k >> (c - 1), (k & half_mask) + 1
        b, w = divmod(s, W)
        i = v & (SIGN - 1)
        out[b][i] += (-mag if v & SIGN else mag) << (c * w)
    return out


def ws_bytes(n, g, c, W):
    E, nb = W * g * n, (g * W) << (c - 1)
    return 28 * E + 320 * nb + 40 * (1 << (ceil_log2(g * W) + c - 1))


def group_fits(n, g, c, W, entries=ENTRY_LIMIT, ws=WS_CAP):
    return (1 <= g <= (1 << 24) // W and W * g * n < entries and ceil_log2(g * W) + c - 1 <= KEY_BITS
            and ws_bytes(n, g, c, W) <= ws)


def plan_batch(n, rows, bits, basis_ok=True, entries=ENTRY_LIMIT, ws=WS_CAP, crossover=None, force=-1):
    """(route, c, W, group_rows, groups): the route rule and the greedy split, by linear search"""
    rows_route = (ROUTE_ROWS, 0, 0, 1, rows)
    if n == 0 or rows == 0 or bits <= 0 or not basis_ok:
        return rows_route
    c, W = batch_window(n, bits)
    batched = rows > 1 and W * n < crossover
    if force >= 0:
        batched = force == ROUTE_BATCHED
    if not batched or not group_fits(n, 1, c, W, entries, ws):
        return rows_route
    g = 1
    while g < rows and group_fits(n, g + 1, c, W, entries, ws):
        g += 1
    return ROUTE_BATCHED, c, W, g, -(-rows // g)


def edge_row(n, c, W, plus):
    """n copies of the scalar whose every window's value is exactly 2^(c-1) (plus = 0: the largest
    positive digit everywhere, no carry) or 2^(c-1) + 1 in window 0 and 2^(c-1) above (a carry out of
    every window up to the top one), cut to the W - 1 windows below the top so that it stays below
    2^(c (W - 1)); returns ints"""
    half = 1 << (c - 1)
    x = sum(half << (c * w) for w in range(W - 1)) + (1 if plus else 0)
    return [x] * n
