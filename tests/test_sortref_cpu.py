"""The bucket-sort reference (tests/sortref.py) proved on its own, without a device: for every
scalar family and every plan (c, W) that test_gpu_bucket_sort.py sorts, the signed digits add up to
the scalar, stay within 2^(c-1), never carry out of the top window, and the entry list holds one
entry per non-zero digit.  Every test counts what it checked."""
import numpy as np
import pytest

import sortref as ref

ALL_PLANS = ref.PLANS + [ref.BIG_PLAN]


def windows_for(bits, c):
    """msm_plan.hpp's windows_for, from its comment: signed-digit windows of c bits for `bits`-bit
    scalars -- the top window's raw value < 2^(bits - c (W-1)) must stay <= 2^(c-1) so that it
    never carries out."""
    W = -(-bits // c)
    if bits - c * (W - 1) > c - 1:
        W += 1
    return W


def small_n(plan):
    return min(plan.n, 700)  # the digit identities do not depend on n; every family at every plan


@pytest.mark.parametrize("plan", ALL_PLANS, ids=repr)
def test_plan_windows(plan):
    """each plan's W is the planner's for its widest scalars, and one bit more would need another"""
    assert windows_for(plan.bits, plan.c) == plan.W
    assert plan.bits == 254 or windows_for(plan.bits + 1, plan.c) > plan.W
    assert plan.bucket_bits == ((plan.W - 1).bit_length() if not plan.shared else 0) + plan.c - 1
    assert plan.W * plan.n < 1 << 31 and (not plan.shared or plan.stride >= plan.n)


@pytest.mark.parametrize("plan", ALL_PLANS, ids=repr)
def test_digits_recompose(plan):
    c, W = plan.c, plan.W
    n = small_n(plan)
    fams = ref.families(plan, np.random.default_rng(plan.c * 100 + plan.W), n)
    checked = 0
    for name, vals in fams.items():
        assert len(vals) == n and all(0 <= v < 1 << plan.bits for v in vals), name
        limbs = ref.to_limbs(vals)
        assert ref.from_limbs(limbs) == vals
        d, carry = ref.digits(limbs, c, W)
        assert not carry.any(), "%s: the top window carried out" % name
        assert all(np.abs(dw).max() <= 1 << (c - 1) for dw in d), name
        cols = [[int(x) for x in dw] for dw in d]
        for i, v in enumerate(vals):
            assert sum(cols[w][i] << (c * w) for w in range(W)) == v, (name, i)
            checked += 1
        ent = ref.entries(limbs, c, W, plan.shared, plan.stride)
        assert len(ent) == sum(int(np.count_nonzero(dw)) for dw in d), name
        assert len(np.unique(ent)) == len(ent), name  # (bucket, value) names one digit
    assert checked == n * len(fams)


def test_entry_layouts_by_hand():
    """c = 4: 0x9f has raw windows f, 9 -> digits -1, -6 (carry), +1: keys and values of both layouts"""
    limbs = ref.to_limbs([0, 0x9F, 8])
    d, carry = ref.digits(limbs, 4, 3)
    assert [[int(x) for x in dw] for dw in d] == [[0, -1, 8], [0, -6, 0], [0, 1, 0]] and not carry.any()
    pw = ref.entries(limbs, 4, 3, False, 0)
    want = sorted([(0 << 3 | 0) << 32 | (1 | ref.SIGN), (0 << 3 | 7) << 32 | 2, (1 << 3 | 5) << 32 | (1 | ref.SIGN),
                   (2 << 3 | 0) << 32 | 1])
    assert [int(x) for x in pw] == want
    sh = ref.entries(limbs, 4, 3, True, 10)
    want = sorted([0 << 32 | (1 | ref.SIGN), 0 << 32 | (2 * 10 + 1), 5 << 32 | ((10 + 1) | ref.SIGN), 7 << 32 | 2])
    assert [int(x) for x in sh] == want


def test_raw_window_crosses_limbs():
    v = (0x3FFFFF << 60) | (1 << 255)
    limbs = ref.to_limbs([v])
    assert int(ref.raw_window(limbs, 60, 22)[0]) == 0x3FFFFF
    assert int(ref.raw_window(limbs, 242, 22)[0]) == 1 << 13  # bits above 255 read as zero
    assert int(ref.raw_window(limbs, 264, 22)[0]) == 0
