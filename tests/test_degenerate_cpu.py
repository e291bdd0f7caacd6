"""The closed form that test_gpu_degenerate.py checks the MSM kernels against, pinned to the C
oracle's naive commit (one double-and-add per term, summed by a complete addition) on the same
dependent bases: repeated points, negated points and identity rows.  Runs without a GPU."""
import pytest

import degenerate as dg
from oracle import coracle as co

CASES = [(b, s, 200) for b in dg.BASES for s in ("uniform", "equal", "cancel")] + [(b, "edge", 64) for b in dg.BASES]


@pytest.mark.parametrize("base,scalars,n", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_closed_form_matches_naive_commit(base, scalars, n):
    c = dg.scalar_family(scalars, n)
    assert all(0 <= x < dg.R for x in c)
    st, out = co.commit(dg.base_limbs(base, n), dg.fr_mont(c))
    assert st == 0
    assert co.g1_from_limbs(out) == dg.expected_point(base, scalars, n)


def test_scalar_families_cover_the_whole_field():
    """uniform draws reach above 2^252 (the masked-limb generators of the older tests do not) and
    the edge values are the canonical ones."""
    c = dg.scalar_family("uniform", 200)
    assert max(c) >> 252 and len(set(c)) == 200
    assert dg.fr_mont([1])[0].tolist() == co.fr_array([1])[0].tolist()
    assert co.fr_ints(dg.fr_mont(list(dg.EDGE))) == list(dg.EDGE)


def test_identity_results_are_rare_but_present():
    """Of the (base, scalars, n) combinations of the GPU module at most one in eight expects the
    identity, and same x cancel does at every even n: neither "always the identity" nor "never the
    identity" can pass there.  (Sizes below 2^16 here; the GPU module asserts it over all of them.)"""
    sizes = [n for n in dg.SIZES if n < 1 << 16]
    zero = [(b, s, n) for b in dg.BASES for s in dg.SCALARS for n in sizes if dg.expected_scalar(b, s, n) == 0]
    assert 8 * len(zero) <= len(dg.BASES) * len(dg.SCALARS) * len(sizes)
    assert ("same", "cancel", 2) in zero and ("same", "cancel", 64) in zero
