"""The batched MSM's internal entry points with forced limits (tests/device/batchprobe.hip over
csrc/kzg_batch.hip): the batched route forced at an n above the crossover and the row route below
it give the same points; a small entry limit runs 7 rows as groups of 3, 3 and 1; the route, the
groups, the window plan and the sort passes each call REPORTS are asserted, so a silent fallback to
the row loop cannot pass."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import batchref
import twist_and_shout as ts
from twist_and_shout import _native as N

from test_gpu_msm_batch import mont, params, points, rand_limbs, check_msm_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "multilinear-map-cryptography_amd", "libtns_batchprobe.so")
ROWS, BATCHED = batchref.ROUTE_ROWS, batchref.ROUTE_BATCHED
INFO = ["route", "groups", "group_rows", "c", "W", "npass"]


@functools.lru_cache(maxsize=None)
def probe():
    lib = C.CDLL(PROBE)
    lib.batchprobe_run.restype = C.c_int
    lib.batchprobe_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, N.U64P, C.c_uint64, C.c_uint64, N.U64P, C.c_int, C.c_int,
                                   C.c_uint64, C.c_uint64, C.c_uint64, N.U64P, N.U64P, C.POINTER(C.c_int64)]
    assert lib.batchprobe_info_words() == len(INFO)
    return lib


def run(cp, op, rows_mont, n, B, z=None, force=-1, entries=0, ws=0, crossover=0):
    out = np.zeros((B, 8), dtype=np.uint64)
    vals = np.zeros((B, 4), dtype=np.uint64)
    info = (C.c_int64 * len(INFO))()
    zz = ts.to_mont([z])[0] if z is not None else None
    st = probe().batchprobe_run(cp.srs.ctx.handle, cp.srs.handle, op, N.p64(np.ascontiguousarray(rows_mont)), n, B,
                                None if zz is None else N.p64(zz), 0, force, entries, ws, crossover, N.p64(vals), N.p64(out), info)
    assert st == 0, (st, N.last_error())
    return out, ts.from_mont(vals), dict(zip(INFO, list(info)))


def passes(n, g, c, W):
    return max(1, -(-(batchref.ceil_log2(g * W) + c - 1) // 9))


def test_rule_and_forced_routes_agree():
    cp, _, pows = params(11)
    n, B = 600, 7
    limbs = rand_limbs(n * B, seed=21)
    m = mont(limbs)
    c, W = batchref.batch_window(n, 253)
    a, _, ia = run(cp, 0, m, n, B)  # the rule: W n digit entries a row, below the shipped crossover
    assert ia == dict(route=BATCHED, groups=1, group_rows=B, c=c, W=W, npass=passes(n, B, c, W))
    check_msm_rows(cp, pows, limbs, n, B, a, seed=1, single=3)
    b, _, ib = run(cp, 0, m, n, B, crossover=W * n)  # at the crossover: the row route ...
    assert (ib["route"], ib["groups"], ib["group_rows"]) == (ROWS, B, 1)
    c2, _, ic = run(cp, 0, m, n, B, crossover=W * n, force=BATCHED)  # ... unless the batched route is forced
    assert ic == ia
    d, _, id_ = run(cp, 0, m, n, B, force=ROWS)  # and the row route forced below it
    assert id_["route"] == ROWS
    _, _, ij = run(cp, 0, m, n, B, crossover=W * n + 1)  # just below the crossover: batched
    assert ij == ia
    assert np.array_equal(a, b) and np.array_equal(a, c2) and np.array_equal(a, d)
    e, _, ie = run(cp, 0, m[:n], n, 1)  # one row: the row route; forced: one group of one row
    assert ie["route"] == ROWS
    f, _, if_ = run(cp, 0, m[:n], n, 1, force=BATCHED)
    assert (if_["route"], if_["groups"], if_["group_rows"]) == (BATCHED, 1, 1) and np.array_equal(e, f) and np.array_equal(e, a[:1])


def test_small_entry_limit_splits_into_groups():
    cp, _, pows = params(7)
    n, B = 300, 7
    limbs = rand_limbs(n * B, seed=22)
    m = mont(limbs)
    c, W = batchref.batch_window(n, 253)
    whole, _, iw = run(cp, 0, m, n, B)
    assert (iw["route"], iw["groups"], iw["group_rows"]) == (BATCHED, 1, 7)
    split, _, info = run(cp, 0, m, n, B, entries=3 * W * n + 1)  # 3 rows fit one sort, 4 do not: 3, 3, 1
    assert info == dict(route=BATCHED, groups=3, group_rows=3, c=c, W=W, npass=passes(n, 1, c, W))
    assert np.array_equal(split, whole)
    check_msm_rows(cp, pows, limbs, n, B, split, seed=2, single=7)
    two, _, i2 = run(cp, 0, m, n, B, ws=batchref.ws_bytes(n, 2, c, W))  # the workspace cap: 2, 2, 2, 1
    assert (i2["route"], i2["groups"], i2["group_rows"]) == (BATCHED, 4, 2) and np.array_equal(two, whole)
    # a group of zero rows between others (rows 3..5 of 3, 3, 1): identities, the other rows as before
    z = m.copy().reshape(B, n, 4)
    z[3:6] = 0
    zo, _, iz = run(cp, 0, z.reshape(-1, 4), n, B, entries=3 * W * n + 1)
    assert (iz["route"], iz["groups"], iz["group_rows"]) == (BATCHED, 3, 3)
    assert not zo[3:6].any() and np.array_equal(zo[:3], whole[:3]) and np.array_equal(zo[6:], whole[6:])
    none, _, i0 = run(cp, 0, m, n, B, entries=W * n)  # not one row fits: the row route
    assert i0["route"] == ROWS and np.array_equal(none, whole)


def test_narrow_batch_plans_few_windows():
    cp, _, pows = params(7)
    n, B = 300, 5
    limbs = rand_limbs(n * B, seed=23, bits=30)
    bits = max(int(x) for x in limbs[:, 0]).bit_length()
    c, W = batchref.batch_window(n, bits)
    out, _, info = run(cp, 0, mont(limbs), n, B)
    assert info == dict(route=BATCHED, groups=1, group_rows=B, c=c, W=W, npass=passes(n, B, c, W))
    assert W == -(-bits // c) + (1 if bits % c == 0 else 0) < batchref.batch_window(n, 254)[1] // 4  # 30 of 254 bits
    check_msm_rows(cp, pows, limbs, n, B, out, seed=3, single=2)


def test_evals_calls_report_their_route():
    cp, _, _ = params(7)
    n, B = 100, 6
    m = mont(rand_limbs(n * B, seed=24))
    rows = m.reshape(B, n, 4)
    cm, _, ic = run(cp, 1, m, n, B)
    assert ic["route"] == BATCHED and ic["groups"] == 1
    assert points(cm) == [ts.KZGVectorCommitment.commit(cp, rows[b]).commitment for b in range(B)]
    cm_rows, _, ir = run(cp, 1, m, n, B, force=ROWS)
    assert ir["route"] == ROWS and np.array_equal(cm, cm_rows)
    for z in (31, 555555555555):  # a node, and off the nodes
        pa, va, ia = run(cp, 2, m, n, B, z=z)
        pb, vb, ib = run(cp, 2, m, n, B, z=z, force=ROWS)
        assert (ia["route"], ib["route"]) == (BATCHED, ROWS) and va == vb and np.array_equal(pa, pb) and pa.any()
        ps, _, is_ = run(cp, 2, m, n, B, z=z, entries=2 * ia["W"] * n + 1)
        assert (is_["route"], is_["groups"], is_["group_rows"]) == (BATCHED, 3, 2) and np.array_equal(ps, pa)
    bare = ts.CommitmentParams.from_g1_limbs(cp.srs.download())  # no basis: rows, whatever is forced
    m64 = mont(rand_limbs(64 * B, seed=25))
    _, _, inb = run(bare, 1, m64, 64, B, force=BATCHED)
    assert inb["route"] == ROWS
