"""Plain-integer reference of the MSM's stages after the sort (csrc/msm.hip: k_accumulate with
k_fix_level / k_bucket_fixup, the bucket reduction and the host finish), and the bucket orders that
tests/test_gpu_accumulate.py hands to the device through tests/device/accprobe.hip.

Every point is a known multiple of the generator, a_i G with the a_i in pool_scalars(), so the
reference works on scalars alone:

  bucket b   = sum of +-a_v mod r over the entries [bstart[b], bstart[b+1])  (value = index | sign << 31)
  set s      = sum_j (j + 1) bucket[s half + j]
  result     = sum_w 2^(c w) set_w  (per-window layout)  or  set 0  (shared layout)

and the expected points come from the C oracle's k G.  Beside that contract the file restates, in
integers, HOW the device is meant to get there -- the per-chunk heads and tails, the two flags of
valid[1], the FIX_FAN-ary level sums and the peel / climb item sequence of the fix-up (simulate), and
the reduction's geometry (tail_geom, fix_level_sizes: csrc/msm_plan.hpp) -- so that each case's
geometry (spans in chunks, (lo mod 8, hi mod 8), deepest level read, reduction regime) is computed,
not assumed.  test_accref_cpu.py proves this file on its own and asserts the coverage of the cases."""
import functools
import zlib

import numpy as np

import sortref

R = sortref.R
SIGN = 1 << 31
FIX_FAN, FIX_LEVELS, FIX_WAVE_SPAN = 8, 8, 512
ACC_KS = (16, 37, 32, 128)  # acc_chunk's floor, an arbitrary table-plan value, the per-window plans' bounds


# ---------------------------------------------------------------- csrc/msm_plan.hpp, restated
def fix_level_sizes(nchunks):
    """[len[1], len[2], ...]: level l has nchunks // 8^l groups and exists while that is >= 2"""
    out, groups = [], nchunks // FIX_FAN
    while len(out) < FIX_LEVELS and groups >= 2:
        out.append(groups)
        groups //= FIX_FAN
    return out


TAIL_FIELDS = ("L0", "L1", "g1", "g", "nbits", "specs", "CH", "nch", "tree", "lg0", "weight", "sum_n")


def tail_geom(half):
    """the bucket reduction of sets of `half` = 2^(c-1) buckets"""
    small = half <= 1 << 19
    L0 = min(4 if small else 16, half // 2)
    g1 = half // L0
    L1 = 4 if g1 >= 1 << 13 and g1 // 4 >= 2 else 0
    g = g1 // L1 if L1 else g1
    nbits = (g - 1).bit_length()
    CH = min(8 if small or L1 else 16, g // 2)
    nch = g // (2 * CH)
    tree = nch % 64 == 0
    return dict(L0=L0, L1=L1, g1=g1, g=g, nbits=nbits, specs=nbits + 2, CH=CH, nch=nch, tree=int(tree),
                lg0=L0.bit_length() - 1, weight=L0 * (L1 or 1), sum_n=nch // 64 if tree else nch)


def sum_passes(n):
    """8-way k_sum_chunks passes of sum_sets over n parts per set"""
    k = 0
    while n > 128 and n % 8 == 0:
        n //= 8
        k += 1
    return k


def regime(half):
    """what the reduction's launch sequence depends on: (L0, L1, CH, tree, k_sum_chunks passes)"""
    t = tail_geom(half)
    return (t["L0"], t["L1"], t["CH"], t["tree"], sum_passes(t["sum_n"]))


# ---------------------------------------------------------------- the point pool
POOL_RANDOM = 1 << 12
# pool indices: the identity, 1 G, the pairs (a, r - a) at I_PAIR + 2 i and + 2 i + 1, one value four
# times at I_REPEAT, random ones from I_RANDOM on
I_ZERO, I_ONE, I_PAIR, I_REPEAT, I_RANDOM = 0, 1, 9, 17, 21


@functools.lru_cache(maxsize=None)
def pool_scalars():
    rnd = sortref.rand_exact(np.random.default_rng(0xACC), 254, POOL_RANDOM + 8)
    a = [0, 1, 2, 3, R - 1, R - 2, 5, 7, 11]
    for x in rnd[:4]:
        a += [x, R - x]
    a += [rnd[4]] * 4
    assert len(a) == I_RANDOM and a[I_PAIR] + a[I_PAIR + 1] == R and a[I_REPEAT] == a[I_REPEAT + 3]
    return tuple(a + rnd[8:])


@functools.lru_cache(maxsize=None)
def scalar_array():
    return np.array(pool_scalars(), dtype=object)


@functools.lru_cache(maxsize=None)
def mul_gen(k):
    """k G as plain affine integers, None for the identity (the C oracle's double-and-add)"""
    from oracle import coracle as co
    return co.g1_mul_gen(k % R)


@functools.lru_cache(maxsize=None)
def pool_limbs():
    """(npool, 16) u32: the device's G1Affine (Montgomery x, y), the identity as (0, 0)"""
    from oracle import coracle as co
    a = pool_scalars()
    out = np.zeros((len(a), 8), dtype=np.uint64)
    for i, k in enumerate(a):
        out[i] = co.g1_to_limbs(mul_gen(k))
    assert not out[0].any() and out[1:].any(axis=1).all()
    return np.ascontiguousarray(out).view(np.uint32).reshape(len(a), 16)


# ---------------------------------------------------------------- orders
class Order:
    """One bucket order: nb run lengths, the values (pool index | sign << 31) and, with ks set, a key
    per entry: bucket << ks | low bits that the accumulation must shift out."""

    def __init__(self, lengths, vals, acc_k, nchunks=None, ks=None, scalars=None):
        self.scalars = scalar_array() if scalars is None else scalars  # a_v of the points the values index
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.bstart = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.uint32)
        self.vals = np.ascontiguousarray(vals, dtype=np.uint32)
        self.valid = int(self.bstart[-1])
        assert self.valid == len(self.vals) >= 1 and (self.lengths >= 0).all()
        self.acc_k = acc_k
        self.nchunks = nchunks if nchunks is not None else -(-self.valid // acc_k)
        assert self.nchunks * acc_k >= self.valid
        self.ks, self.keys = ks, None
        if ks is not None:
            bucket = np.repeat(np.arange(len(self.lengths), dtype=np.uint32), self.lengths)
            low = (np.arange(self.valid, dtype=np.uint32) * np.uint32(40503)) & np.uint32((1 << ks) - 1)
            self.keys = np.ascontiguousarray((bucket << np.uint32(ks)) | low, dtype=np.uint32)

    @property
    def nb(self):
        return len(self.lengths)

    # ---- the contract
    def prefix(self):
        """cs[p] = the signed scalars of the entries [0, p) added up, exact integers"""
        a = self.scalars[(self.vals & np.uint32(SIGN - 1)).astype(np.int64)]
        a = np.where((self.vals >> np.uint32(31)).astype(bool), -a, a)
        return np.concatenate([np.array([0], dtype=object), np.cumsum(a)])

    def sparse_buckets(self):
        """(indices of the non-empty buckets, their sums mod r)"""
        cs, b = self.prefix(), self.bstart.astype(np.int64)
        nz = np.nonzero(b[1:] > b[:-1])[0]
        return nz, (cs[b[nz + 1]] - cs[b[nz]]) % R

    def buckets(self, sparse=None):
        out = [0] * self.nb
        for i, v in zip(*(sparse or self.sparse_buckets())):
            out[int(i)] = int(v)
        return out

    def set_sums(self, Wr, half, sparse=None):
        """sum_j (j + 1) bucket[s half + j] for every set s"""
        nz, v = sparse or self.sparse_buckets()
        out = [0] * Wr
        for s in range(Wr):
            m = (nz // half) == s
            out[s] = int((v[m] * (nz[m] % half + 1).astype(object)).sum()) % R if m.any() else 0
        return out

    # ---- the geometry
    def runs(self):
        """(bucket, tf, tl) of every non-empty run: its first and last chunk"""
        b = self.bstart.astype(np.int64)
        nz = np.nonzero(b[1:] > b[:-1])[0]
        return [(int(k), int(b[k]) // self.acc_k, int(b[k + 1] - 1) // self.acc_k) for k in nz]

    def flags(self):
        """valid[1]: bit 0 iff some run has entries in two chunks; bit 1 iff some aligned group of 8
        chunks below valid (all eight inside nchunks, the eighth beginning below valid) lies in one
        bucket"""
        k = self.acc_k
        f = 1 if any(tf != tl for _, tf, tl in self.runs()) else 0
        t = np.arange(0, max(self.nchunks - 7, 0), 8, dtype=np.int64)
        t = t[(t + 7) * k < self.valid]
        if len(t):
            first = np.searchsorted(self.bstart, t * k, side="right")
            last = np.searchsorted(self.bstart, np.minimum((t + 8) * k, self.valid) - 1, side="right")
            if (first == last).any():
                f |= 2
        return f


def result_of(sums, c, shared):
    return sums[0] if shared else sum(s << (c * w) for w, s in enumerate(sums)) % R


def fix_items(tf, tl, nlevels):
    """the inner heads of a run over the chunks tf < tl as (level, index), in the fix-up's order:
    peeled to FIX_FAN-aligned ranges, climbing a level whenever both ends are aligned (msm.hip:
    FixItems::next and the thread path's loop)"""
    lo, hi, l, out = tf + 1, tl, 0, []
    while lo < hi:
        climb = l < nlevels and hi - lo >= 2 * FIX_FAN
        if climb and lo % FIX_FAN == 0 and hi % FIX_FAN == 0:
            lo //= FIX_FAN
            hi //= FIX_FAN
            l += 1
            continue
        if not climb or lo % FIX_FAN:
            i = lo
            lo += 1
        else:
            hi -= 1
            i = hi
        out.append((l, i))
    return out


def on_wave_path(tf, tl):
    return tl - tf > FIX_WAVE_SPAN


def run_geometry(o):
    """per run across chunks: dict(span, path, pair = (lo mod 8, hi mod 8), levels = those it reads,
    items = the points its sum adds: the tail, the head and the inner heads)"""
    nl = len(fix_level_sizes(o.nchunks))
    out = []
    for _, tf, tl in o.runs():
        if tf == tl:
            continue
        items = fix_items(tf, tl, nl)
        out.append(dict(span=tl - tf, path="wave" if on_wave_path(tf, tl) else "thread",
                        pair=((tf + 1) % FIX_FAN, tl % FIX_FAN), levels={l for l, _ in items}, items=len(items) + 2))
    return out


def simulate(o):
    """The device's route in integers: (buckets, flags).  Chunk heads and tails as k_accumulate leaves
    them, the level sums k_fix_level forms (uniform groups only, and only under flag bit 1), then every
    bucket as k_bucket_fixup adds it up.  An item that nobody wrote raises KeyError."""
    k, valid, cs = o.acc_k, o.valid, o.prefix()
    b = o.bstart.astype(np.int64)
    used = min(o.nchunks, -(-valid // k))  # chunks that begin below valid
    starts = np.arange(used, dtype=np.int64) * k
    ends = np.minimum(starts + k, valid)
    first = np.searchsorted(o.bstart, starts, side="right") - 1
    last = np.searchsorted(o.bstart, ends - 1, side="right") - 1
    head, tail, direct = {}, {}, {}
    crossed = False
    for t in range(used):
        lo, hi, fb, lb = int(starts[t]), int(ends[t]), int(first[t]), int(last[t])
        head_run, tail_run = b[fb] < lo, b[lb + 1] > hi
        crossed |= bool(head_run or tail_run)
        if fb == lb:  # one run: a head if it began before, else a tail if it goes on, else the bucket
            v = int(cs[hi] - cs[lo])
            if head_run:
                head[t] = v
            elif tail_run:
                tail[t] = v
            else:
                direct[fb] = v
            continue
        nzb = fb + np.nonzero(b[fb + 1:lb + 2] > b[fb:lb + 1])[0]
        for bk in nzb:
            s, e = max(int(b[bk]), lo), min(int(b[bk + 1]), hi)
            v = int(cs[e] - cs[s])
            if bk == fb and head_run:
                head[t] = v
            elif bk == lb and tail_run:
                tail[t] = v
            else:
                direct[int(bk)] = v
    grouped = any(t + 7 < used and first[t] == last[t + 7] for t in range(0, o.nchunks - 7, 8))
    flags = (1 if crossed else 0) | (2 if grouped else 0)
    sizes = fix_level_sizes(o.nchunks)
    lv = {0: head}
    for l, n in enumerate(sizes, 1):
        span, lv[l] = k * FIX_FAN ** l, {}
        for g in range(n if flags & 2 else 0):
            ea, eb = g * span, (g + 1) * span
            if eb <= valid and first[ea // k] == last[(eb - 1) // k]:
                # (a group that begins with its run's first chunk adds a head nobody wrote: the
                # device forms that sum too, and no run reads it -- poison here)
                part = [lv[l - 1].get(g * FIX_FAN + j) for j in range(FIX_FAN)]
                lv[l][g] = None if None in part else sum(part)
    out = [0] * o.nb
    for bk, tf, tl in o.runs():
        if tf == tl:
            out[bk] = direct[bk] % R
            continue
        acc = tail[tf] + head[tl]
        for l, i in fix_items(tf, tl, len(sizes)):
            if lv[l][i] is None:
                raise KeyError("run of bucket %d reads the poisoned level-%d sum %d" % (bk, l, i))
            acc += lv[l][i]
        out[bk] = acc % R
    return out, flags


# ---------------------------------------------------------------- cases
class Case:
    """One probe call: a plan (c, W, layout) and one or two orders; `buckets`: compared one by one;
    `prefill`: a case run first on the same plan, so that the bucket buffer holds its buckets."""

    def __init__(self, name, c, W, shared, orders, buckets=True, prefill=None):
        self.name, self.c, self.W, self.shared, self.orders = name, c, W, shared, orders
        self.half = 1 << (c - 1)
        self.Wr = 1 if shared else W
        self.nb = self.Wr * self.half
        self.buckets = buckets and self.nb <= 1 << 12
        self.prefill = prefill
        assert all(o.nb == self.nb for o in orders) and (len(orders) == 1 or shared)

    def __repr__(self):
        return self.name


def _rng(*tag):
    return np.random.default_rng(zlib.crc32("/".join(str(t) for t in tag).encode()))


def random_vals(rng, n, lo=I_RANDOM):
    idx = rng.integers(lo, len(pool_scalars()), size=n, dtype=np.uint32)
    return idx | (rng.integers(0, 2, size=n, dtype=np.uint32) << np.uint32(31))


def lattice_lengths(nb, k, empty_ends, until=None):
    """run lengths cycling through k-1, 1, k, k+1, 0, 0, 2k, 2k-1, 1, 3k+1, 0: runs end on, start on,
    straddle and contain chunk edges, with empty buckets on both sides; empty_ends: bucket 0 and the
    last bucket are empty; until: cut to that many entries"""
    units = [k - 1, 1, k, k + 1, 0, 0, 2 * k, 2 * k - 1, 1, 3 * k + 1, 0]
    out = [units[(i - 1 if empty_ends else i) % len(units)] for i in range(nb)]
    if empty_ends:
        out[0] = out[-1] = 0
    if until is not None:
        tot = 0
        for i, n in enumerate(out):
            out[i] = max(0, min(n, until - tot))
            tot += out[i]
        assert tot == until, (tot, until)
    return out


@functools.lru_cache(maxsize=None)
def lattice_cases(k):
    """the chunk-edge lattice at acc_k = k: both end variants, with and without keys, valid a multiple
    of k, one more than a multiple, as it comes, and nchunks sized from a bound of 1.5 valid"""
    out = []
    c = 8 if k <= 37 else 7
    nb = 1 << (c - 1)
    for empty_ends in (False, True):
        for keyed in (False, True):
            rng = _rng("lattice", k, empty_ends, keyed)
            full = sum(lattice_lengths(nb, k, empty_ends))
            for what, valid, slack in (("all", full, 1.0), ("multiple", full // k * k, 1.0),
                                       ("multiple+1", (full // k - 1) * k + 1, 1.0), ("bound", full, 1.5)):
                ln = lattice_lengths(nb, k, empty_ends, valid)
                o = Order(ln, random_vals(rng, valid), k, -(-int(valid * slack) // k), ks=3 if keyed else None)
                out.append(Case("lattice_k%d_%s_%s_%s" % (k, "empty-ends" if empty_ends else "full-ends",
                                                          "keys" if keyed else "nokeys", what), c, 1, True, [o]))
    if k == 16:  # per-window, nb = 2^12; and valid = 1 at either end and in the middle
        rng = _rng("lattice", "pw")
        ln = lattice_lengths(1 << 12, 16, True)
        out.append(Case("lattice_k16_pw_c12_W2", 12, 2, False, [Order(ln, random_vals(rng, sum(ln)), 16)]))
        for pos in (0, 1, 63, 127):
            ln = [0] * 128
            ln[pos] = 1
            for keyed in (False, True):
                out.append(Case("one_entry_b%d_%s" % (pos, "keys" if keyed else "nokeys"), 8, 1, True,
                                [Order(ln, random_vals(rng, 1), 16, ks=2 if keyed else None)]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def no_crossing_cases():
    """no run crosses a chunk (flag bit 0 stays 0): the fix-up writes the empty buckets only, over what
    a call with every bucket non-empty left in the bucket buffer"""
    out = []
    for k in (16, 37):
        rng = _rng("nocross", k)
        pre = Order([2] * 128, random_vals(rng, 256), k)
        ln = [0] + [(k // 2, 0, k - k // 2)[i % 3] for i in range(126)] + [0]  # every 3 buckets: one chunk
        o = Order(ln, random_vals(rng, sum(ln)), k)
        out.append(Case("no_crossing_k%d" % k, 8, 1, True, [o], prefill=Case("prefill_k%d" % k, 8, 1, True, [pre])))
    return tuple(out)


def heavy_order(nb, k, heavy, rng, same, ks=None):
    """heavy: [(bucket, first entry, last entry)], increasing; the buckets before each share the
    entries before it evenly, the buckets after the last get one entry each but for the last bucket
    (empty).  same: every entry of a heavy run is one point (equal chunk heads: the doubling branch of
    the level butterfly and of the chains), else random points."""
    ln = [0] * nb
    pos, prev = 0, 0
    for bk, s, e in heavy:
        gap, nfill = s - pos, bk - prev
        assert (gap == 0 or nfill > 0) and e >= s
        for i in range(nfill):
            ln[prev + i] = gap // nfill + (1 if i < gap % nfill else 0)
        ln[bk] = e - s + 1
        pos, prev = e + 1, bk + 1
    for bk in range(prev, nb - 1):
        ln[bk] = 1
    vals = random_vals(rng, sum(ln))
    if same:
        b = np.concatenate([[0], np.cumsum(ln)])
        for n, (bk, s, e) in enumerate(heavy):
            vals[b[bk]:b[bk + 1]] = np.uint32(I_RANDOM + 5 + n) | np.uint32(SIGN if n % 2 else 0)
    return Order(ln, vals, k, ks=ks)


def variant(same):
    return "same" if same else "rand"


@functools.lru_cache(maxsize=None)
def thread_cases(depth):
    """acc_k = 16, one heavy run a case, on the thread path: every (lo mod 8, hi mod 8) with an aligned
    range of two groups of level `depth` inside the run (depth 1: spans 20..32 chunks, 2: 130..144)"""
    k, out = 16, []
    A, need = (16, 16) if depth == 1 else (64, 128)
    for lo in range(8):
        for hi in range(8):
            tf = A - 1 - (8 - lo) % 8
            tl = A + need + hi
            if tl - tf < (20 if depth == 1 else 130):
                tl += 8
            s, e = tf * k + (lo * 5 + hi) % k, tl * k + (lo + hi * 3) % k
            for same in (True, False):
                o = heavy_order(64, k, [(5, s, e)], _rng("thread", depth, lo, hi, same), same,
                                ks=1 if (lo + hi) % 2 else None)
                out.append(Case("thread%d_lo%d_hi%d_%s" % (depth, lo, hi, variant(same)), 7, 1, True, [o]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def threshold_cases():
    """tl - tf = 512 (the last thread-path span) and 513 (the first wave-path one)"""
    k, out = 16, []
    for span in (FIX_WAVE_SPAN, FIX_WAVE_SPAN + 1):
        for same in (True, False):
            o = heavy_order(64, k, [(9, 3 * k + 7, (3 + span) * k + 2)], _rng("threshold", span, same), same)
            out.append(Case("threshold_span%d_%s" % (span, variant(same)), 7, 1, True, [o]))
    return tuple(out)


# (level, tf, span in chunks): an aligned range of two level-l groups lies inside (tf, tf + span);
# tf mod 512 takes 0, 1, 7, 63 and 511.  (4, 4680, 52663): lo = 0o11111 and hi = 0o157777 peel at every
# level, 66 items in all -- the one run whose items take a second round of 64 in the wave's loop
DEEP = ((3, 0, 1539), (3, 513, 2100), (3, 7, 2000), (3, 63, 1990), (3, 511, 1030), (4, 63, 12300), (4, 4095, 8198),
        (4, 4680, 52663), (5, 32767, 65538))


@functools.lru_cache(maxsize=None)
def deep_cases(level):
    """acc_k = 16, the wave path: heavy runs that read level `level`.  Level 5 needs an aligned range of
    2 x 8^5 chunks past chunk 8^5: 98305 chunks, 1.5 x 2^20 entries.  Levels 6..8 would need more than
    2^23 entries in one bucket and stay unexercised."""
    k, out = 16, []
    for l, tf, span in DEEP:
        if l != level:
            continue
        for same in (True, False):
            heavy = [(3, tf * k + 5, (tf + span) * k + 11)] if tf else [(0, 0, span * k + 11)]
            o = heavy_order(64, k, heavy, _rng("deep", l, tf, span, same), same)
            out.append(Case("deep_l%d_tf%d_span%d_%s" % (l, tf, span, variant(same)), 7, 1, True, [o]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def wave_edge_cases():
    """two heavy buckets in one wave of 64 buckets (the ballot loop runs twice) with a light one
    between them; and per-window c = 4, W = 9: nb = 72, so the second wave has 8 buckets and 56 lanes
    past nb, with a heavy run in its first and in its last bucket"""
    k, out = 16, []
    for same in (True, False):
        h = [(10, 40 * k + 3, 640 * k + 1), (12, 640 * k + 9, 1670 * k + 4)]
        out.append(Case("two_heavy_in_a_wave_" + variant(same), 7, 1, True,
                        [heavy_order(64, k, h, _rng("wave", "two", same), same)]))
        for bk in (64, 71):
            rng = _rng("wave", bk, same)
            ln = [3] * 72
            ln[bk] = 700 * k + 5
            vals = random_vals(rng, sum(ln))
            if same:
                vals[3 * bk:3 * bk + ln[bk]] = np.uint32(I_RANDOM + 3)
            out.append(Case("heavy_b%d_of_72_%s" % (bk, variant(same)), 4, 9, False, [Order(ln, vals, k)]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cancellation_cases():
    k, nb, out = 16, 64, []
    P, Q = I_PAIR, I_PAIR + 1  # a G and (r - a) G
    rng = _rng("cancel")

    def neg(i):
        return int(i) | SIGN

    def r(n):
        return [int(v) for v in random_vals(rng, n)]

    def case(name, ln, vals):
        ln = list(ln) + [0] * (nb - len(ln))
        out.append(Case("cancel_" + name, 7, 1, True, [Order(ln, np.array(vals, dtype=np.uint32), k)]))

    # P, -P adjacent inside a chunk, mid-run: by the sign bit, and as the pool's a and r - a
    case("adjacent_sign", [5, 9], r(5) + r(3) + [P, neg(P)] + r(4))
    case("adjacent_pair", [5, 9], r(5) + r(3) + [P, Q] + r(4))
    # a chunk whose whole partial is the identity, inside a run over four chunks
    case("identity_chunk", [8, 3 * k + 8], r(8) + r(8) + [P, neg(P)] * (k // 2) + r(2 * k))
    # a tail S met by a head -S: the bucket is the identity, reached in the fix-up
    t = r(8)
    case("tail_meets_head", [8, k + 16], r(8) + t + [P, neg(P)] * (k // 2) + [v ^ SIGN for v in t])
    # the identity point with the sign bit set; a bucket of identities alone, over a chunk edge
    case("signed_identity", [3, 4], r(3) + [neg(I_ZERO), I_ZERO] + r(2))
    case("only_identities", [10, 20, 3], r(10) + [neg(I_ZERO), I_ZERO] * 10 + r(3))
    # a heavy run whose every chunk cancels: 40 chunks of Q, -Q
    case("heavy_cancels", [4, 40 * k], r(4) + [Q, neg(Q)] * (20 * k))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def two_set_cases():
    """nj = 2 on one shared plan: a heavy set with the lattice, crossing with non-crossing sets (the
    flags differ), different acc_k and nchunks (the level counts differ)"""
    k, c, nb = 16, 9, 256
    rng = _rng("twoset")
    heavy = heavy_order(nb, k, [(40, 100 * k + 3, 1200 * k + 8)], rng, False)
    ln = lattice_lengths(nb, k, True)
    lattice = Order(ln, random_vals(rng, sum(ln)), k, ks=2)
    light = Order([1] * nb, random_vals(rng, nb), 37)
    two_level = heavy_order(nb, k, [(7, 9 * k + 1, 160 * k + 3)], rng, True)
    return (Case("two_heavy_lattice", c, 1, True, [heavy, lattice]), Case("two_lattice_heavy", c, 1, True, [lattice, heavy]),
            Case("two_crossing_light", c, 1, True, [two_level, light]), Case("two_light_heavy", c, 1, True, [light, heavy]))


SWEEP_SHAPES = [(c, 1, True) for c in range(4, 22)] + [(c, W, False) for W in (2, 3, 13) for c in (4, 8, 12, 16)]


def sweep_positions(half):
    """bucket positions that pin each weight: the ends of the first groups of both levels, the middle,
    the last, and the masked sums' group indices with a single bit and with all bits set"""
    t = tail_geom(half)
    w = t["weight"]
    pos = {0, 1, t["L0"] - 1, t["L0"], w - 1, w, w + 1, half // 2 - 1, half // 2, half - 1}
    pos |= {(1 << b) * w for b in range(t["nbits"])} | {(t["g"] - 1) * w, (t["g"] - 1) * w + w - 1}
    return sorted(p for p in pos if 0 <= p < half)


def sweep_cases(c, W, shared):
    """the reduction's patterns for one shape; every run is one entry (acc_k = 32: nothing crosses)"""
    half, Wr = 1 << (c - 1), 1 if shared else W
    nb, k, out = Wr * half, 32, []
    rng = _rng("sweep", c, W, shared)
    name = "%s_c%d_W%d_" % ("sh" if shared else "pw", c, W)

    def case(what, ln, vals):
        out.append(Case(name + what, c, W, shared, [Order(ln, vals, k)], buckets=False))

    for j in sweep_positions(half):  # one non-empty bucket at j of every set, another point in each
        ln = np.zeros(nb, dtype=np.int64)
        ln[np.arange(Wr) * half + j] = 1
        case("single_j%d" % j, ln, random_vals(rng, Wr))
    pt = np.uint32(I_RANDOM + c)
    case("all_same", np.ones(nb, dtype=np.int64), np.full(nb, pt, dtype=np.uint32))
    alt = np.full(nb, pt, dtype=np.uint32)
    alt[1::2] |= np.uint32(SIGN)
    case("alternating", np.ones(nb, dtype=np.int64), alt)
    ln = (rng.random(nb) < min(1.0, 300.0 / nb)).astype(np.int64)
    ln[int(rng.integers(0, nb))] = 1
    case("sparse", ln, random_vals(rng, int(ln.sum())))
    return out


def fixup_cases():
    """every case of the accumulation and the fix-up: what the coverage conditions are computed over"""
    out = ()
    for k in ACC_KS:
        out += lattice_cases(k)
    out += no_crossing_cases() + thread_cases(1) + thread_cases(2) + threshold_cases()
    for l in (3, 4, 5):
        out += deep_cases(l)
    return out + wave_edge_cases() + cancellation_cases() + two_set_cases()
