"""The MSM window planner's (n, scalar width) plane, end to end: ts.msm over one setup_params(16)
SRS of 2^18 + 1 points -- so every n below 2^18 also runs with a table wider than the MSM
(stride != n in the sort's values) -- each result against the trapdoor identity
C == (sum c_i tau^i) G, never against another HIP path.  After every MSM the plan it took is read
from the lane's hint through tests/device/sortprobe.hip; the last test asserts that the grid reached
the plan classes no other direct MSM test does.  One test is one size: all 15 widths, window tables
on and off over the same scalars (nothing is thinned).

Two of those classes lie outside the (n, width) grid as given, by best_window's cost model, and get
a case of their own: the (16, 2) plan needs 2 n + 3 * 2^16 < 3 n + 3 * 3 * 2^10, i.e. 30- or 31-bit
scalars at n = 2^18 (EXTRA_WIDTHS), and one window of bits + 1 > 20 bits beats two 12-bit windows
only above n = 3 * 2^22 - 3 * 2^12 scalars (test_single_window_plan_above_20_bits, n = 2^24)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from oracle import pyoracle as po

import sortref
import twist_and_shout as ts
from twist_and_shout import _native as N

pytestmark = pytest.mark.gpu
R = po.R_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "multilinear-map-cryptography_amd", "libtns_sortprobe.so")
SIZES = [65, 257, 1 << 11, 3000, (1 << 12) + 1, 1 << 13, 12289, (1 << 14) + 1, 1 << 15, 40000, (1 << 16) - 1, 1 << 16,
         (1 << 16) + 1, 100000, (1 << 17) + 1, 1 << 18]
WIDTHS = [1, 8, 14, 15, 16, 22, 23, 32, 33, 64, 65, 128, 160, 253, 254]
EXTRA_WIDTHS = {1 << 18: [30]}
SEQUENCE = [30, 30, 254, 30, 12, 22, 22, 64, 64]
R_LIMBS = np.array([(R >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)
PLANS = {}  # (n, width, tables) -> (c, W, bucket_bits, shared): the plan each grid MSM took
HIP_ERRORS = []


@functools.lru_cache(maxsize=None)
def setup():
    pp, _ = ts.setup_params(16)
    cp = pp.commitment_params
    tau, pows, t = cp.tau, [], 1
    for _ in range(1 << 18):
        pows.append(t)
        t = t * tau % R
    lib = C.CDLL(PROBE)
    lib.sortprobe_hint.restype, lib.sortprobe_hint.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    return cp, pows, lib


def reduce_mod_r(limbs):
    """x - R where x >= R, for x < 2^254 < 2 R (four u64 limbs)"""
    ge = np.ones(len(limbs), dtype=bool)  # x >= R, from the low limb up
    for l in range(4):
        ge = np.where(limbs[:, l] == R_LIMBS[l], ge, limbs[:, l] > R_LIMBS[l])
    out, borrow = limbs.copy(), np.zeros(len(limbs), dtype=np.uint64)
    for l in range(4):
        d = limbs[:, l] - R_LIMBS[l]
        b1 = limbs[:, l] < R_LIMBS[l]
        d2 = d - borrow
        b2 = d < borrow
        out[:, l] = np.where(ge, d2, limbs[:, l])
        borrow = (b1 | b2).astype(np.uint64)
    return out


def scalars(n, width, seed):
    """n random scalars below 2^width (mod R at 254 bits, with R - 1), one of exactly `width` bits"""
    rng = np.random.default_rng(seed)
    limbs = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64, endpoint=False)
    for l in range(4):
        keep = min(max(width - 64 * l, 0), 64)
        limbs[:, l] &= np.uint64((1 << keep) - 1)
    if width == 254:
        limbs = reduce_mod_r(limbs)
        limbs[n // 3] = R_LIMBS
        limbs[n // 3, 0] -= np.uint64(1)
    top = (1 << (width - 1)) | (0 if width < 3 else 5)  # exactly `width` bits, below R
    limbs[n // 2] = [(top >> (64 * l)) & (2**64 - 1) for l in range(4)]
    return limbs


def to_ints(limbs):
    if not limbs[:, 1:].any():
        return limbs[:, 0].tolist()
    raw = limbs.tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(limbs))]


def msm_checked(limbs, tables, what):
    """ts.msm of the canonical scalars against the trapdoor identity; returns the plan it left as hint"""
    cp, pows, lib = setup()
    vals = to_ints(limbs)
    assert max(vals).bit_length() <= 254 and max(vals) < R
    want = po.affine_mul(po.G1_GEN, sum(v * t for v, t in zip(vals, pows)) % R)
    mont = np.zeros_like(limbs)
    N.load().tns_fr_from_canonical(N.p64(np.ascontiguousarray(limbs)), len(limbs), N.p64(mont))
    ctx = cp.srs.ctx
    assert not HIP_ERRORS, "an earlier call failed (%s): no further GPU work in this process" % HIP_ERRORS[0]
    ctx.set_msm_tables(tables)
    try:
        got = ts.msm(cp, mont)
    except ts.DeviceError as e:
        HIP_ERRORS.append("%s: %s" % (what, e))
        raise
    finally:
        if not HIP_ERRORS:
            ctx.set_msm_tables(True)
    assert got == want, "%s: the MSM is not (sum c_i tau^i) G" % what
    hint = (C.c_int64 * 5)()
    assert lib.sortprobe_hint(ctx.handle, hint) == 0
    assert hint[0] == len(limbs), (what, list(hint))
    return hint[1], hint[2], hint[3], bool(hint[4])


def run_size(n):
    checked = 0
    for width in WIDTHS + EXTRA_WIDTHS.get(n, []):
        limbs = scalars(n, width, seed=n * 1000 + width)
        for tables in (True, False):
            PLANS[(n, width, tables)] = msm_checked(limbs, tables, "n=%d, %d bits, tables %s" % (n, width, tables))
            # the plan sortref's restatement of the cost model predicts: commits of >= 2^16 points come
            # with the window table over the SRS's 2^18 + 1 points (kzg.hip srs_fixed_base)
            table = sortref.table_shape((1 << 18) + 1) if tables and n >= 1 << 16 else None
            assert PLANS[(n, width, tables)] == sortref.plan_msm(n, width, table)[0], (n, width, tables)
            checked += 1
    assert checked == 2 * len(WIDTHS + EXTRA_WIDTHS.get(n, []))


def test_reduce_mod_r():
    xs = [0, 1, R - 1, R, R + 1, 2**254 - 1, R + 2**64, R - 2**64, (R & ~(2**128 - 1)) + 5, 2**253]
    raw = b"".join(x.to_bytes(32, "little") for x in xs)
    got = to_ints(reduce_mod_r(np.frombuffer(raw, dtype=np.uint64).reshape(len(xs), 4).copy()))
    assert got == [x % R for x in xs]


@pytest.mark.parametrize("n", SIZES)
def test_plan_grid(n):
    run_size(n)


@pytest.mark.parametrize("n", [12289, 1 << 16, 1 << 18])
def test_plan_sequence_on_one_lane(n):
    """The lane's plan hint (msm.hip bits_launch) across MSMs of one size, widths 30, 30, 254, 30,
    12, 22, 22, 64, 64 and then 254, 254 in a row: every MSM leaves its plan as the hint, and the
    next one counts pass 1 ahead for it when the hinted plan has a compile-time pass-1 kernel.  A
    repeated width then confirms the hint (the sort keeps the precounted histograms; with the
    scalars' low words when the plan's windows fit 64 bits), a new width rejects it (the sort
    recounts).  Which steps precount depends on n: at 2^18 the pairs 30, 30 -- (16, 2) -- and 22, 22
    -- (12, 2) -- confirm with low words and 254, 254 -- the shared (17, 15) -- without; each 254
    after a narrow width and each narrow width after 254 is a rejected hint.  2^18 is a size beyond
    the two the grid's plan asks for: at 12289 and 2^16 the planner gives 30-bit scalars three
    11-bit windows, which have no compile-time kernel."""
    checked, plans = 0, []
    widths = SEQUENCE + [254, 254]
    for k, width in enumerate(widths):
        limbs = scalars(n, width, seed=n + 31 * k)
        plans.append(msm_checked(limbs, True, "sequence n=%d step %d (%d bits)" % (n, k, width)))
        checked += 1
    assert checked == len(widths) == 11
    assert plans[0] == plans[1] == plans[3] and plans[5] == plans[6] and plans[7] == plans[8] and plans[9] == plans[10]
    assert plans[2] == plans[9] and plans[2] != plans[1]
    assert all(W == windows_for(width, c) for width, (c, W, _, _) in zip(widths, plans))
    if n == 1 << 18:
        assert plans[0][:2] == (16, 2) and plans[5][:2] == (12, 2) and plans[2] == (17, 15, 16, True), plans


def test_single_window_plan_above_20_bits():
    """2^24 scalars of at most 22 bits take ONE 23-bit window (best_window's w1max route: n additions
    instead of 2 n).  All but 2048 scalars are zero -- the plan depends on n and the widest scalar
    alone -- so the trapdoor sum stays small.  Per-window layout (no window table is built)."""
    n, width = 1 << 24, 22
    pp, _ = ts.setup_params(22)
    cp = pp.commitment_params
    rng = np.random.default_rng(24)
    pos = np.unique(np.concatenate([rng.integers(0, n, size=2045), [0, n // 2, n - 1]]))
    u = np.zeros(n, dtype=np.uint64)
    u[pos] = rng.integers(1, 1 << width, size=len(pos), dtype=np.uint64)
    u[n // 2] = (1 << (width - 1)) | 5
    want = po.affine_mul(po.G1_GEN, sum(int(u[i]) * pow(cp.tau, int(i), R) for i in pos) % R)
    ctx = cp.srs.ctx
    assert not HIP_ERRORS, "an earlier call failed (%s): no further GPU work in this process" % HIP_ERRORS[0]
    ctx.set_msm_tables(False)
    try:
        got = ts.msm(cp, ts.fr_from_u64_array(u))
    except ts.DeviceError as e:
        HIP_ERRORS.append("single window: %s" % e)
        raise
    finally:
        if not HIP_ERRORS:
            ctx.set_msm_tables(True)
    assert got == want
    hint = (C.c_int64 * 5)()
    assert setup()[2].sortprobe_hint(ctx.handle, hint) == 0
    assert list(hint) == [n, width + 1, 1, width, 0], list(hint)
    PLANS[(n, width, False)] = (hint[1], hint[2], hint[3], bool(hint[4]))


def windows_for(bits, c):
    """msm_plan.hpp's windows_for: the top window's raw value must stay <= 2^(c-1)"""
    W = -(-bits // c)
    return W + 1 if bits - c * (W - 1) > c - 1 else W


def passes_of(c, W, bucket_bits, shared):
    """the sort's pass count for a plan (bucket_sort_begin: 9 key bits a pass)"""
    wb = (W - 1).bit_length() if shared else 0
    return max(1, -(-(bucket_bits + wb) // 9))


def test_grid_reached_every_plan_class():
    """(runs whatever part of the grid has not run in this process, then looks at all of it)"""
    for n in SIZES:
        if (n, WIDTHS[0], True) not in PLANS:
            run_size(n)
    if (1 << 24, 22, False) not in PLANS:
        test_single_window_plan_above_20_bits()
    assert len(PLANS) == 2 * (len(SIZES) * len(WIDTHS) + sum(len(v) for v in EXTRA_WIDTHS.values())) + 1
    plans = set(PLANS.values())
    print("plans (c, W, bucket_bits, shared) the grid took:", sorted(plans))
    assert any(sh and passes_of(c, W, bb, sh) == 2 for c, W, bb, sh in plans), "no shared two-pass plan"
    assert any(sh and passes_of(c, W, bb, sh) == 3 for c, W, bb, sh in plans), "no shared three-pass plan"
    for cw in ((16, 2), (12, 2), (17, 15)):
        assert any((c, W) == cw for c, W, _, _ in plans), "compile-time plan %r not reached" % (cw,)
    assert any(W == 1 and c == width + 1 > 20 for (_, width, _), (c, W, _, _) in PLANS.items()), "no single-window plan"
    for (_, width, _), (c, W, _, _) in PLANS.items():  # and every plan has the planner's window count
        assert W == windows_for(width, c), (width, c, W)
