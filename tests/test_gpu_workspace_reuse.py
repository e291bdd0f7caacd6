"""The device workspaces a context shares between its entry points, used small after large and
large after small: one fixed list of calls on the process context, run forwards and then
backwards, every call's second result bit-equal to its first.

The shapes are the smallest that still reach each workspace user: 65 scalars is the first MSM
past the tiny path (64), 4097 coefficients the first KZG opening whose suffix scan takes a second
level of carries (more than SCAN_K^2 = 64^2 coefficients, poly.hip), nv = 14 one above the
sum-check's split and persistent-tail thresholds of 13, and the four-table sum-check's fourth
fold buffer shares its storage with the node sweep of the Lagrange route's openings.
"""
import numpy as np
import pytest

from oracle import coracle as co

import twist_and_shout as ts
from test_gpu_sumcheck import COMPOSITIONS, host_threads, rand_tables

pytestmark = pytest.mark.gpu

L = 11  # setup_params(11): 2^13 operations, 2^13 + 1 SRS points


def _rand_rows(n, seed):
    """n Montgomery Fr: rand_tables' n one-entry tables as one (n, 4) array."""
    return np.concatenate(rand_tables(n, 0, seed))


def _sumcheck_call(name, nv, seed):
    terms = COMPOSITIONS[name]
    k = 1 + max(max(ix) for _, ix in terms if ix)
    tabs = rand_tables(k, nv, seed=seed)
    claim = co.fast_composition_sum(tabs, nv, terms, host_threads())
    return lambda: ts.SumCheck(nv, claim).prove(tabs, terms, ts.Transcript(bytes(32)), return_challenges=True)


def call_list():
    """(what, call) pairs on the process context, and the verifier parameters of the proofs."""
    pp, vp = ts.setup_params(L)
    cp = pp.commitment_params
    ctx = cp.srs.ctx
    assert ctx is ts.Context.get(0)
    cp.srs.prepare_lagrange(1 << 13)

    big = ts.bench_trace(1 << L, 1 << 13)
    small = ts.bench_trace(1 << 8, 1 << 10)
    coeffs = _rand_rows(4097, seed=1)
    values = _rand_rows(1 << 11, seed=2)
    mle = ts.MultilinearExtension(10, ts.from_mont(_rand_rows(1 << 10, seed=3)))
    point = ts.from_mont(_rand_rows(10, seed=4))
    sc64, sc65 = _rand_rows(64, seed=5), _rand_rows(65, seed=6)
    entries = ts.fr_from_u64_array(np.arange(64, dtype=np.uint64) * 3 + 1)
    lookups = (np.arange(1000, dtype=np.uint64) * 7) % 64

    def twist_coefficient_route():
        ctx.set_commit_basis(False)
        try:
            return ts.Twist(pp).prove_soa(*small)
        finally:
            ctx.set_commit_basis(True)

    calls = [
        ("twist 2^13, Lagrange route", lambda: ts.Twist(pp).prove_soa(*big)),
        ("kzg open, 4097 coefficients", lambda: ts.KZGCommitment.open(cp, coeffs, 2**200 + 9)),
        ("interpolate 2^11", lambda: ts.poly_utils.interpolate_consecutive(values).tobytes()),
        ("sum-check, 3 tables, nv 14", _sumcheck_call("twist_like", 14, seed=7)),
        ("sum-check, 4 tables, nv 9", _sumcheck_call("dense4", 9, seed=8)),
        ("mle evaluate nv 10", lambda: mle.evaluate(point)),
        ("msm 64", lambda: ts.msm(cp, sc64)),
        ("msm 65", lambda: ts.msm(cp, sc65)),
        ("shout T 64, M 1000", lambda: ts.Shout(pp).prove_arrays(entries, lookups)),
        ("twist 2^10, coefficient route", twist_coefficient_route),
    ]
    return calls, vp


def test_shared_workspaces_small_after_large_and_back():
    calls, vp = call_list()
    first = [call() for _, call in calls]
    # the two Twist proofs stand on their own: the host verifier accepts them
    assert ts.Twist.verify(first[0], vp)
    assert ts.Twist.verify(first[9], vp)
    for (what, call), want in reversed(list(zip(calls, first))):
        assert call() == want, what
