"""The MSM's accumulation with its fix-up (k_accumulate, k_fix_level, k_bucket_fixup), the bucket
reduction (k_reduce_level, k_reduce_level2, k_masked_sums, sum_sets) and the host finish alone,
against the plain-integer reference tests/accref.py.  tests/device/accprobe.hip uploads a bucket
order written here and hands it to the shipped msm_from_order_dev, which runs msm_launch_accumulate,
msm_launch_tails and the host finish as every MSM does; nothing is re-implemented on the device.

Every comparison is exact.  Points are known multiples a_i G of the generator, so the reference adds
scalars: each bucket after the fix-up (where the plan has at most 2^12 buckets), each set's window
sum before Horner, and the result are compared as points with k G from the C oracle -- a device XYZZ
(X, Y, ZZ, ZZZ) equals the affine (x, y) iff X = x ZZ, Y = y ZZZ, ZZ^3 = ZZZ^2 and ZZ != 0, the
identity iff ZZ = 0 -- and the two flags of valid[1], the reduction's geometry and the fix-level
count are compared as integers.  The geometry each case reaches (spans, peel pairs, levels, flags,
regimes) is asserted without a GPU in test_accref_cpu.py.

Fix levels 6..8 need more than 2^23 entries in one bucket and stay unexercised, like the two
branches no legal plan reaches (CH = 16 and sum_sets' 8-way passes: DESIGN 2.16).  Every test prints
the cases, buckets and sums it compared."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import accref as A
import fieldref
import twist_and_shout as ts
from twist_and_shout import _native as N

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "multilinear-map-cryptography_amd", "libtns_accprobe.so")
INFO = A.TAIL_FIELDS + ("Wr", "half", "nb", "inputs_intact")
HIP_ERRORS = []  # a failed call ends the file's GPU work: nothing more runs on a device that faulted
COUNT = {"cases": 0, "buckets": 0, "sums": 0}
M, RINV = fieldref.FQ.M, fieldref.FQ.RINV


class ProbeSet(C.Structure):
    _fields_ = [("vals", C.c_void_p), ("bstart", C.c_void_p), ("keys", C.c_void_p), ("ks", C.c_int32),
                ("acc_k", C.c_int32), ("entries", C.c_uint64), ("nchunks", C.c_uint64), ("buckets", C.c_void_p),
                ("sums", C.c_void_p), ("result", C.c_void_p), ("flags", C.c_uint32), ("fix_levels", C.c_int32)]


@functools.lru_cache(maxsize=None)
def probe():
    assert os.path.exists(PROBE), "build() builds libtns_accprobe.so"
    N.load()
    lib = C.CDLL(PROBE)
    lib.accprobe_run.restype = C.c_int
    lib.accprobe_run.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                 C.c_void_p]
    assert lib.accprobe_info_words() == len(INFO)
    return lib


def run(case, want_buckets=None):
    """-> (info, [per set: dict(flags, fix_levels, sums, result, buckets)])"""
    lib, pool = probe(), A.pool_limbs()
    want_buckets = case.buckets if want_buckets is None else want_buckets
    sets = (ProbeSet * len(case.orders))()
    keep = []
    for s, o in zip(sets, case.orders):
        out = dict(sums=np.zeros((case.Wr, 32), dtype=np.uint32), result=np.zeros(32, dtype=np.uint32),
                   buckets=np.full((case.nb, 32), 0xA5A5A5A5, dtype=np.uint32) if want_buckets else None)
        vals, bstart, keys = o.vals.copy(), o.bstart.copy(), None if o.keys is None else o.keys.copy()
        keep.append((out, vals, bstart, keys))
        s.vals, s.bstart, s.keys = vals.ctypes.data, bstart.ctypes.data, None if keys is None else keys.ctypes.data
        s.ks, s.acc_k, s.entries, s.nchunks = o.ks or 0, o.acc_k, o.valid, o.nchunks
        s.buckets = out["buckets"].ctypes.data if want_buckets else None
        s.sums, s.result = out["sums"].ctypes.data, out["result"].ctypes.data
    info = np.zeros(len(INFO), dtype=np.int64)
    assert not HIP_ERRORS, "an earlier probe call failed (%s): no further GPU work in this process" % HIP_ERRORS[0]
    st = lib.accprobe_run(ts.Context.get(0).handle, pool.ctypes.data, len(pool), case.c, case.W, 1 if case.shared else 0,
                          len(case.orders), C.addressof(sets), info.ctypes.data)
    if st > 0:  # (-1: the probe refused the arguments, nothing ran)
        HIP_ERRORS.append("%r: accprobe_run returned %d (%s)" % (case, st, N.last_error()))
    assert st == 0, HIP_ERRORS[-1] if st > 0 else "%r: the probe refused the order" % case
    for s, (out, vals, bstart, keys), o in zip(sets, keep, case.orders):
        out["flags"], out["fix_levels"] = int(s.flags), int(s.fix_levels)
        # the host arrays the probe read are the case's own, untouched
        assert np.array_equal(vals, o.vals) and np.array_equal(bstart, o.bstart), case
    return dict(zip(INFO, (int(x) for x in info))), [k[0] for k in keep]


def coords(words):
    """32 u32 words -> the four Montgomery coordinates mod M (the buckets come in the lazy domain [0, 2M))"""
    raw = np.ascontiguousarray(words, dtype=np.uint32).tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") % M for i in range(4)]


def point_error(words, k):
    """None if the XYZZ point equals k G exactly, else what differs"""
    X, Y, ZZ, ZZZ = coords(words)
    want = A.mul_gen(k)
    if want is None:
        return None if ZZ == 0 else "a finite point, want the identity"
    if ZZ == 0:
        return "the identity, want %d G" % k
    zz, zzz = ZZ * RINV % M, ZZZ * RINV % M
    if pow(zz, 3, M) != zzz * zzz % M:
        return "zz^3 != zzz^2"
    if X != want[0] * ZZ % M or Y != want[1] * ZZZ % M:
        return "another point than %d G" % k
    return None


def check(case, want_buckets=None):
    """one probe call against the reference: flags, geometry, level counts, buckets, window sums, result"""
    info, outs = run(case, want_buckets)
    t = A.tail_geom(case.half)
    assert {f: info[f] for f in A.TAIL_FIELDS} == t, case
    assert (info["Wr"], info["half"], info["nb"]) == (case.Wr, case.half, case.nb), case
    assert info["inputs_intact"] == 1, "%r: the kernels wrote the order, the points or valid[0]" % case
    for j, (o, out) in enumerate(zip(case.orders, outs)):
        what = "%r set %d" % (case, j)
        assert out["flags"] == o.flags(), "%s: valid[1] = %d, want %d" % (what, out["flags"], o.flags())
        assert out["fix_levels"] == len(A.fix_level_sizes(o.nchunks)), what
        sparse = o.sparse_buckets()  # (one pass over the entries for the buckets and the sums)
        if out["buckets"] is not None:
            for b, k in enumerate(o.buckets(sparse)):
                err = point_error(out["buckets"][b], k)
                assert err is None, "%s: bucket %d of %d (bucket, first chunk, last chunk %s; acc_k %d) is %s" % (
                    what, b, case.nb, [r for r in o.runs() if r[0] == b], o.acc_k, err)
            COUNT["buckets"] += case.nb
        sums = o.set_sums(case.Wr, case.half, sparse)
        for w, k in enumerate(sums):
            err = point_error(out["sums"][w], k)
            assert err is None, "%s: window sum %d is %s" % (what, w, err)
        COUNT["sums"] += case.Wr
        err = point_error(out["result"], A.result_of(sums, case.c, case.shared))
        assert err is None, "%s: the result is %s" % (what, err)
    COUNT["cases"] += 1
    return info, outs


def report(what, before):
    print("%s: %d cases, %d buckets, %d window sums compared" % (
        what, COUNT["cases"] - before["cases"], COUNT["buckets"] - before["buckets"], COUNT["sums"] - before["sums"]))


# ---------------------------------------------------------------- chunk edges
@pytest.mark.parametrize("k", A.ACC_KS)
def test_chunk_edge_lattice(k):
    """runs that end on, start on, straddle and contain chunk edges, empty buckets around them, valid on
    and one past a multiple of acc_k, valid = 1, chunks past valid; with and without keys"""
    before = dict(COUNT)
    for case in A.lattice_cases(k):
        check(case)
    report("lattice acc_k %d" % k, before)
    assert COUNT["cases"] - before["cases"] == len(A.lattice_cases(k)) >= 16


def test_no_run_crosses_a_chunk():
    """flag bit 0 stays 0 and the fix-up takes its "only empty buckets" path: every empty bucket is
    the identity although the bucket buffer held a previous call's non-empty buckets"""
    before = dict(COUNT)
    for case in A.no_crossing_cases():
        check(case.prefill)
        info, outs = check(case)
        assert outs[0]["flags"] == 0
    report("no crossing", before)


# ---------------------------------------------------------------- heavy runs
@pytest.mark.parametrize("depth", [1, 2])
def test_thread_path_peel_pairs(depth):
    """one heavy run a case on the thread path of k_bucket_fixup: all 64 (lo mod 8, hi mod 8), climbing
    `depth` levels; entries all one point (equal heads: the doubling branch of xyzz_add_lazy in the
    level butterfly and the chain) and random points"""
    before = dict(COUNT)
    for case in A.thread_cases(depth):
        check(case)
    report("thread path, %d level(s)" % depth, before)
    assert COUNT["cases"] - before["cases"] == 128


def test_wave_span_threshold():
    """tl - tf = 512 stays one thread's chain, 513 is the wave's"""
    before = dict(COUNT)
    for case in A.threshold_cases():
        check(case)
    report("threshold", before)
    assert COUNT["cases"] - before["cases"] == 4


@pytest.mark.parametrize("level", [3, 4, 5])
def test_wave_path_deep_runs(level):
    """runs that read fix level `level` at unaligned starts (level 5: 1.5 x 2^20 entries, the least
    that reaches it at acc_k = 16); one level-4 run has 66 items, a second round of the wave's loop"""
    before = dict(COUNT)
    for case in A.deep_cases(level):
        check(case)
    report("wave path, level %d" % level, before)
    assert COUNT["cases"] > before["cases"]


def test_wave_path_edges():
    """two heavy buckets in one wave of 64 (the ballot loop runs twice); a heavy bucket in the wave whose
    other lanes lie past nb"""
    before = dict(COUNT)
    for case in A.wave_edge_cases():
        check(case)
    report("wave edges", before)


def test_cancellation():
    """P, -P adjacent; a chunk whose partial is the identity; a tail met by its negative in the
    fix-up; the identity point with the sign bit set; buckets of identities; a heavy run that cancels"""
    before = dict(COUNT)
    for case in A.cancellation_cases():
        check(case)
    report("cancellation", before)
    assert COUNT["cases"] - before["cases"] == 7


# ---------------------------------------------------------------- two sets in one tail
def test_two_set_tail():
    """nj = 2 (blockIdx.y picks the MSM): each set's flags, level count, buckets, sums and result are
    those of the same order run alone"""
    before = dict(COUNT)
    for case in A.two_set_cases():
        info, both = check(case)
        for j, o in enumerate(case.orders):
            alone = A.Case("%s_alone%d" % (case.name, j), case.c, case.W, case.shared, [o])
            _, one = check(alone)
            # (both runs' buckets, sums and result equal the reference's points exactly: check)
            for f in ("flags", "fix_levels"):
                assert both[j][f] == one[0][f], (case, j, f)
    report("two-set tail", before)
    assert COUNT["cases"] - before["cases"] == 12


# ---------------------------------------------------------------- the reduction
@pytest.mark.parametrize("c,W,shared", A.SWEEP_SHAPES, ids=lambda v: str(int(v)))
def test_reduction_sweep(c, W, shared):
    """one non-empty bucket at each position that pins a weight ((j + 1) a G), every bucket the same
    point, buckets alternating P, -P, random sparse; the probe's TailGeom is the restatement's"""
    before = dict(COUNT)
    cases = A.sweep_cases(c, W, shared)
    for case in cases:
        info, outs = check(case)
        assert outs[0]["flags"] == 0
    report("reduction c=%d W=%d %s" % (c, W, "shared" if shared else "per-window"), before)
    # (half = 8 at c = 4 leaves six distinct positions; three patterns beside them)
    assert COUNT["cases"] - before["cases"] == len(cases) == len(A.sweep_positions(1 << (c - 1))) + 3 >= 9
