"""MultilinearExtension::evaluate of a batch of tables in one pass (tns_mle_evaluate_batch, its
_device form and tns_mle_evaluate_device; csrc/mle_eval.hip).  Every comparison is
exact equality of field elements against tests/mleref.py's big-integer fold.  (1) the grid
nv in {0..12, 14, 16, 18} x batch in {1, 3}, and batch 70 for nv <= 5 (a block holding many
instances, its last block partly filled), 1 to 4 tables spread over it, at five kinds of points --
random, all 0 (the first entry), all 1 (the last), the boolean point of a random index (that entry),
every coordinate r - 1 -- on random tables holding entries 0 and r - 1 and, where there are several,
one all-zero table; the regime, launches, blocks and rows tests/device/mleevalprobe.hip reports are
asserted for every case against the geometry's restatement (regime boundaries 2^6 and 2^8 entries an
instance, both sides of each in the grid), host and resident entries agree and the resident inputs
come back unchanged; (2) forced limits: several rows a thread, an instance one block behind the eq
launch, several blocks of several rows; (3) tns_mle_evaluate_device against tns_mle_evaluate;
(4) degenerate calls and errors."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from oracle import coracle as co
from oracle import pyoracle as po

import twist_and_shout as ts
from twist_and_shout import _native as N

import mleevalprobe as mp
import mleref as ref

pytestmark = pytest.mark.gpu
R = po.R_MOD
KINDS = ["random", "zeros", "ones", "boolean", "rminus1"]
GRID = [(nv, b) for nv in list(range(13)) + [14, 16, 18] for b in (1, 3)] + [(nv, 70) for nv in range(6)]
# tables a case: 1..4 spread over the grid; the largest sizes take the counts that keep the
# big-integer reference of a case at a couple of seconds
BIG_K = {(16, 1): 4, (16, 3): 2, (18, 1): 3, (18, 3): 1}


def n_tables(nv, batch):
    return BIG_K.get((nv, batch), 1 + (nv + batch) % 4)


@functools.lru_cache(maxsize=None)
def case(nv, batch):
    """k read-only tables of batch x 2^nv Montgomery Fr: random, with an entry 0 and an entry r - 1
    an instance; with several tables, the last one all zero when nv is a multiple of 3"""
    k = n_tables(nv, batch)
    rng = np.random.default_rng(7001 * nv + 13 * batch + k)
    pick = random.Random(31 * nv + batch)
    n = 1 << nv
    minus1 = co.fr_array([R - 1])[0]
    tabs = []
    for j in range(k):
        t = rng.integers(0, 2**63, size=(batch << nv, 4), dtype=np.uint64) * np.uint64(2)
        t += rng.integers(0, 2, size=(batch << nv, 4), dtype=np.uint64)
        t[:, 3] &= np.uint64((1 << 60) - 1)  # below r
        t = t.reshape(batch, n, 4)
        if k > 1 and j == k - 1 and nv % 3 == 0:
            t[:] = 0
        else:
            for b in range(batch):
                t[b, pick.randrange(n)] = 0
                t[b, pick.randrange(n)] = minus1
        t.setflags(write=False)
        tabs.append(t)
    return tabs


@functools.lru_cache(maxsize=None)
def points(nv, batch, kind):
    """(batch rows of nv canonical coordinates, per instance the entry index the value must equal or None)"""
    rng = random.Random(1000 * nv + 10 * batch + KINDS.index(kind))
    n = 1 << nv
    if kind == "random":
        return [[rng.randrange(R) for _ in range(nv)] for _ in range(batch)], [None] * batch
    if kind == "zeros":
        return [[0] * nv for _ in range(batch)], [0] * batch
    if kind == "ones":
        return [[1] * nv for _ in range(batch)], [n - 1] * batch
    if kind == "boolean":
        idx = [rng.randrange(n) for _ in range(batch)]
        return [[(i >> v) & 1 for v in range(nv)] for i in idx], idx
    return [[R - 1] * nv for _ in range(batch)], [None] * batch


@functools.lru_cache(maxsize=None)
def expected(nv, batch, kind):
    """per instance the list of its tables' values (canonical), by the big-integer fold -- or, at a
    boolean point, the entry itself"""
    tabs = case(nv, batch)
    pts, idx = points(nv, batch, kind)
    out = []
    for b in range(batch):
        if idx[b] is None:
            out.append([ref.mle_eval_mont(t[b], pts[b]) for t in tabs])
        else:
            out.append([ref.from_mont_int(ref.mont_ints(t[b, idx[b]])[0]) for t in tabs])
    return out


def ints(values):
    return [co.fr_ints(row) for row in values]


@functools.lru_cache(maxsize=None)
def resident(nv, batch):
    ctx = ts.Context.get(0)
    return [ts.DeviceBuffer(ctx, t) for t in case(nv, batch)]


# (1) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv,batch", GRID)
def test_grid_matches_the_fold(nv, batch):
    tabs = case(nv, batch)
    bufs = resident(nv, batch)
    want_info = mp.plan(nv, batch)
    assert want_info[1] <= 2 and want_info[1] == (1 if nv <= 8 else 2)
    for kind in KINDS:
        pts, _ = points(nv, batch, kind)
        want = expected(nv, batch, kind)
        arr = mp.points_array(pts)
        arr.setflags(write=False)
        st, vals, info = mp.evaluate(tabs, nv, batch, arr, bufs=bufs)
        assert st == 0, N.last_error()
        assert info == want_info, kind
        assert ints(vals) == want, ("resident", kind)
        if kind in ("random", "rminus1"):  # the host entry uploads the tables: the same values
            st, hv, info = mp.evaluate(tabs, nv, batch, arr)
            assert st == 0 and info == want_info
            assert np.array_equal(hv, vals), ("host", kind)
    # the public entries, host and resident
    pts, _ = points(nv, batch, "random")
    want = expected(nv, batch, "random")
    assert ts.MultilinearExtension.evaluate_batch(tabs, pts) == want
    assert ts.mle_evaluate_batch_resident(bufs, pts) == want
    for t, dt in zip(tabs, bufs):  # the inputs are only read
        back = np.empty_like(t)
        ts.buffer_download(dt, back)
        assert np.array_equal(back, t)
    resident.cache_clear()


def test_every_regime_and_the_launch_counts():
    """the reported regime is the restatement's for every case of the grid (asserted above); here:
    every regime appears, on both sides of each boundary, and the launch count does not move with
    nv or with the batch"""
    seen = {(nv, b): mp.plan(nv, b) for nv, b in GRID}
    assert {v[0] for v in seen.values()} == {mp.WAVE, mp.BLOCK, mp.BLOCKS}
    assert [seen[(nv, 1)][0] for nv in (6, 7, 8, 9)] == [mp.WAVE, mp.BLOCK, mp.BLOCK, mp.BLOCKS]
    got = {}
    for nv, b in ((9, 1), (9, 3), (16, 1), (16, 3)):
        arr = mp.points_array(points(nv, b, "random")[0])
        st, vals, info = mp.evaluate(case(nv, b), nv, b, arr)
        assert st == 0 and ints(vals) == expected(nv, b, "random")
        got[(nv, b)] = info
    assert {i[1] for i in got.values()} == {2} and {i[0] for i in got.values()} == {mp.BLOCKS}


# (2) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv,batch,min_blocks,max_log_rows,want", [
    (9, 3, 1, -1, (mp.BLOCK, 2, 3, 2)),       # the instance's two rows in one block, behind the eq launch
    (12, 3, 1, -1, (mp.BLOCK, 2, 3, 16)),
    (14, 1, 1, -1, (mp.BLOCK, 2, 1, 64)),     # the most rows a thread takes
    (16, 3, 1, -1, (mp.BLOCKS, 2, 12, 64)),   # four blocks an instance, 64 rows a thread
    (12, 3, 8, -1, (mp.BLOCKS, 2, 12, 4)),    # the rule's own stop: 48 rows, at least 8 blocks
    (12, 3, 1, 1, (mp.BLOCKS, 2, 24, 2)),     # the row cap
    (10, 1, 1, 0, (mp.BLOCKS, 2, 4, 1)),
])
def test_forced_limits(nv, batch, min_blocks, max_log_rows, want):
    assert mp.plan(nv, batch, min_blocks, 6 if max_log_rows < 0 else max_log_rows) == want
    tabs = case(nv, batch)
    for kind in ("random", "boolean"):
        arr = mp.points_array(points(nv, batch, kind)[0])
        st, vals, info = mp.evaluate(tabs, nv, batch, arr, min_blocks=min_blocks, max_log_rows=max_log_rows)
        assert st == 0, N.last_error()
        assert info == want
        assert ints(vals) == expected(nv, batch, kind), kind
    # the next call by the rule (the cross-block counters were left at zero)
    arr = mp.points_array(points(nv, batch, "random")[0])
    st, vals, info = mp.evaluate(tabs, nv, batch, arr)
    assert st == 0 and info == mp.plan(nv, batch) and ints(vals) == expected(nv, batch, "random")


# (3) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [0, 1, 5, 7, 8, 9, 12])
def test_single_resident_table_matches_tns_mle_evaluate(nv):
    t = case(nv, 1)[0][0]
    ctx = ts.Context.get(0)
    buf = ts.DeviceBuffer(ctx, t)
    evals = [ref.from_mont_int(x) for x in ref.mont_ints(t)]
    mle = ts.MultilinearExtension(nv, evals)
    for kind in ("random", "rminus1", "boolean"):
        pt = points(nv, 1, kind)[0][0]
        got = ts.mle_evaluate_resident(buf, nv, pt)
        assert got == mle.evaluate(pt) == ref.mle_eval(evals, pt)
    back = np.empty_like(t)
    ts.buffer_download(buf, back)
    assert np.array_equal(back, t)


# (4) ----------------------------------------------------------------------------------------------
def test_empty_calls_write_nothing():
    tabs = case(4, 3)
    arr = mp.points_array(points(4, 3, "random")[0])
    st, _, info = mp.evaluate(tabs, 4, 0, arr)
    assert st == 0 and info == (mp.NONE, 0, 0, 0)
    st, _, info = mp.evaluate([], 4, 3, arr)
    assert st == 0 and info == (mp.NONE, 0, 0, 0)
    assert ts.MultilinearExtension.evaluate_batch([], points(4, 3, "random")[0]) == [[], [], []]
    out = np.full((3, 4), 7, dtype=np.uint64)
    L, ctx = N.load(), ts.Context.get(0)
    ptrs = (N.U64P * 1)(N.p64(np.ascontiguousarray(tabs[0]).reshape(-1, 4)))
    assert L.tns_mle_evaluate_batch(ctx.handle, ptrs, 1, 4, 0, N.p64(arr.reshape(-1, 4)), N.p64(out)) == 0
    assert L.tns_mle_evaluate_batch(ctx.handle, ptrs, 0, 4, 3, N.p64(arr.reshape(-1, 4)), N.p64(out)) == 0
    assert (out == 7).all()


def test_invalid_calls():
    nv, batch = 4, 3
    tabs = case(nv, batch)
    pts = points(nv, batch, "random")[0]
    arr = mp.points_array(pts)
    L, ctx = N.load(), ts.Context.get(0)
    flat = [np.ascontiguousarray(t).reshape(-1, 4) for t in tabs]
    out = np.zeros((batch * 5, 4), dtype=np.uint64)
    five = (N.U64P * 5)(*[N.p64(flat[0])] * 5)
    p64 = N.p64(arr.reshape(-1, 4))
    assert L.tns_mle_evaluate_batch(ctx.handle, five, 5, nv, batch, p64, N.p64(out)) == 1  # more than 4 tables
    assert L.tns_mle_evaluate_batch(ctx.handle, five, -1, nv, batch, p64, N.p64(out)) == 1
    assert L.tns_mle_evaluate_batch(None, five, 1, nv, batch, p64, N.p64(out)) == 1  # NULL handle
    assert L.tns_mle_evaluate_batch(ctx.handle, None, 1, nv, batch, p64, N.p64(out)) == 1  # NULL arrays
    assert L.tns_mle_evaluate_batch(ctx.handle, five, 1, nv, batch, None, N.p64(out)) == 1
    assert L.tns_mle_evaluate_batch(ctx.handle, five, 1, nv, batch, p64, None) == 1
    hole = (N.U64P * 2)(N.p64(flat[0]), None)
    assert L.tns_mle_evaluate_batch(ctx.handle, hole, 2, nv, batch, p64, N.p64(out)) == 1
    # sizes: checked before anything is read
    assert L.tns_mle_evaluate_batch(ctx.handle, five, 1, 31, 1, p64, N.p64(out)) == 1
    assert L.tns_mle_evaluate_batch(ctx.handle, five, 1, 30, 5, p64, N.p64(out)) == 1
    assert "2^32" in N.last_error()
    assert L.tns_mle_evaluate_device(ctx.handle, None, nv, p64, N.p64(out)) == 1
    assert not out.any()
    # the Python mirror's own checks
    with pytest.raises(ts.InvalidParameters):
        ts.MultilinearExtension.evaluate_batch([flat[0][:-1]], pts)
    with pytest.raises(ts.InvalidParameters):
        ts.mle_evaluate_batch_resident([ts.DeviceBuffer(ctx, flat[0][:-1])], pts)
    with pytest.raises(ts.InvalidParameters):
        ts.mle_evaluate_resident(ts.DeviceBuffer(ctx, flat[0]), nv, pts[0])  # batch x 2^nv entries, not 2^nv
    # and the context evaluates correctly afterwards
    assert ts.MultilinearExtension.evaluate_batch(tabs, pts) == expected(nv, batch, "random")
