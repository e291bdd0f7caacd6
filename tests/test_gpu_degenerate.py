"""MSMs and KZG openings on inputs with known relations: dependent bases and zero quotients.

Every other GPU test runs its MSMs over powers of a random tau (or the Lagrange basis derived
from them): pairwise distinct points, none the identity, none the negative of another, so partial
sums never collide and the exceptional branches of the curve formulas (P == Q, P == -Q, identity
operands -- csrc/bn254.hpp's xyzz_madd_lazy / xyzz_add_lazy, k_accumulate's negated identity, the
window-table build over identities) are reached with negligible probability.  And no opened vector
is constant, so no quotient is all zero.  Here:

A. raw MSMs over bases B_i = k_i G with k_i from a small set (tests/degenerate.py), against the
   closed form (sum c_i k_i) G, with scalars drawn over all of [0, r);
B. whole proofs over the powers of tau = r - 1, 1 and 0 (G, -G, G, ... / all G / G then identities);
C. constant columns: every quotient value (v - y_j) / (z - j) is zero, through each opening path
   (commitment c G, opening value c, opening proof the identity).
Every comparison is exact.
"""
import numpy as np
import pytest

import degenerate as dg
from oracle import coracle as co
from oracle import pyoracle as po
from test_gpu_configs import check_pair, host_threads, replay

import twist_and_shout as ts

pytestmark = pytest.mark.gpu
R = po.R_MOD
SEED = bytes(range(32))


# ----------------------------------------------------------------------------- A. raw MSM
_SRS = {}
_MONT = {}


def family_srs(base):
    """One upload of 2^16 rows per base family; an MSM of n scalars runs over its first n rows."""
    if base not in _SRS:
        limbs = dg.base_limbs(base, 1 << 16)
        _SRS[base] = (ts.CommitmentParams.from_g1_limbs(limbs), limbs)
    return _SRS[base]


def scalars_mont(name, n):
    if (name, n) not in _MONT:
        _MONT[(name, n)] = dg.fr_mont(dg.scalar_family(name, n))
    return _MONT[(name, n)]


def msm(cp, scalars, tables=True):
    ctx = cp.srs.ctx
    ctx.set_msm_tables(tables)
    try:
        return ts.msm(cp, scalars)
    finally:
        ctx.set_msm_tables(True)


# 2^16 runs with the window table (shared buckets; the table build itself runs over the repeated
# and identity points) and without it (per-window buckets)
MSM_CASES = [(b, s, n, t) for b in dg.BASES for n in dg.SIZES for t in ((True, False) if n == 1 << 16 else (True,))
             for s in dg.SCALARS]


@pytest.mark.parametrize("base,scalars,n,tables", MSM_CASES,
                         ids=["%s-%s-%d-%s" % (b, s, n, "tables" if t else "plain") for b, s, n, t in MSM_CASES])
def test_msm_over_dependent_bases(base, scalars, n, tables):
    cp, _ = family_srs(base)
    got = msm(cp, scalars_mont(scalars, n), tables)
    assert got == dg.expected_point(base, scalars, n)


def test_identity_results_are_rare_but_present():
    """Pure integer arithmetic: at most one case in eight expects the identity, and same x cancel
    at 2^16 does -- neither "always the identity" nor "never the identity" passes the cases above."""
    combos = [(b, s, n) for b in dg.BASES for s in dg.SCALARS for n in dg.SIZES]
    zero = [k for k in combos if dg.expected_scalar(*k) == 0]
    assert 8 * len(zero) <= len(combos)
    assert ("same", "cancel", 1 << 16) in zero
    assert dg.expected_point("same", "cancel", 1 << 16) is None


@pytest.mark.parametrize("base", ["small", "holes"])
def test_upload_download_keeps_identity_rows(base):
    cp, limbs = family_srs(base)
    assert not limbs[1].any()  # row 1 is the identity in both families
    assert np.array_equal(cp.srs.download(), limbs)
    pts = cp.g1_powers[:6]
    assert pts[1] is None and pts[0] == co.g1_from_limbs(limbs[0])


def _stages(cp, scalars, tables=True):
    ctx = cp.srs.ctx
    ts.profile_enable(ctx, True)
    try:
        got = msm(cp, scalars, tables)
        out = {s: ts.profile_read_ex(ctx, s) for s in ("msm_sort", "msm_accumulate")}
    finally:
        ts.profile_enable(ctx, False)
    return got, out


def test_routes_by_stage_counters():
    """The stage counters confirm the routes the sizes were chosen for: 64 points take the
    one-thread-per-point kernel (no sort, no accumulation), 65 the sorted pipeline; at 2^16 the
    table plan sorts fewer windows than the per-window plan (msm_sort's algorithmic bytes are
    32 n + 16 W n), i.e. set_msm_tables switches the plan."""
    cp, _ = family_srs("small")
    want = {n: dg.expected_point("small", "uniform", n) for n in (64, 65, 1 << 16)}
    got, st = _stages(cp, scalars_mont("uniform", 64))
    assert got == want[64]
    assert st["msm_sort"]["launches"] == 0 and st["msm_accumulate"]["launches"] == 0
    got, st = _stages(cp, scalars_mont("uniform", 65))
    assert got == want[65]
    assert st["msm_sort"]["launches"] == 1 and st["msm_accumulate"]["launches"] == 1
    assert 0 < st["msm_accumulate"]["ops"]
    n = 1 << 16
    W = {}
    for tables in (True, False):
        got, st = _stages(cp, scalars_mont("uniform", n), tables)
        assert got == want[n]
        assert st["msm_sort"]["launches"] == 1 and st["msm_accumulate"]["launches"] == 1
        w, rem = divmod(int(st["msm_sort"]["bytes"]) - 32 * n, 16 * n)
        assert rem == 0
        W[tables] = w
    assert 0 < W[True] < W[False]


# ----------------------------------------------------------------------------- B. degenerate SRS
TAUS = {"minus_one": R - 1, "one": 1, "zero": 0}
_G = co.g1_to_limbs(po.G1_GEN)
_NEG_G = co.g1_to_limbs(po.g1_neg(po.G1_GEN))
_PP = {}


def tau_rows(tau, rows):
    """The powers tau^i G, i < rows, for tau in {r - 1, 1, 0}."""
    out = np.zeros((rows, 8), dtype=np.uint64)
    if tau == 0:
        out[0] = _G
    elif tau == 1:
        out[:] = _G
    else:
        assert tau == R - 1
        out[0::2] = _G
        out[1::2] = _NEG_G
    return out


def degenerate_params(tau, log_size):
    if (tau, log_size) not in _PP:
        max_ops = 1 << (log_size + 2)
        rows = tau_rows(tau, max_ops + 1)
        cp = ts.CommitmentParams.from_g1_limbs(rows, tau=tau)  # set_tau checks g1_powers[1] == tau G
        pp = ts.ProverParams(log_size, max_ops, cp, SEED)
        vp = ts.VerifierParams(log_size, max_ops, SEED, ts.CommitmentVerificationKey.from_tau(tau))
        _PP[(tau, log_size)] = (pp, vp, rows)
    return _PP[(tau, log_size)]


def oracle_params(pp, rows):
    return dict(max_operations=pp.max_operations, g1_powers=[co.g1_from_limbs(r) for r in rows],
                fiat_shamir_seed=pp.fiat_shamir_seed)


def both_routes(tau, ctx, prove):
    """The proof; for a tau that is no node also on the coefficient route (same proof).  tau = 0
    and tau = 1 are nodes: no Lagrange basis exists and the prover takes the coefficients itself."""
    g = prove()
    if tau == R - 1:
        ctx.set_commit_basis(False)
        try:
            assert prove() == g
        finally:
            ctx.set_commit_basis(True)
    return g


def assert_no_basis(pp, n):
    with pytest.raises(ts.InvalidParameters):
        pp.commitment_params.srs.lagrange_points(n)


@pytest.mark.parametrize("tau", TAUS.values(), ids=TAUS.keys())
@pytest.mark.parametrize("n_ops", [5, 16])
def test_twist_small_over_degenerate_srs_matches_oracle(tau, n_ops):
    pp, vp, rows = degenerate_params(tau, 2)
    vals = dg.scalar_family("uniform", 16)
    # (entries 0 and 1 of both columns are non-zero: f(0) = y[0] and f(1) = y[1] are the commitments there)
    ops = po.memory_trace_ops(4, [("w", (i + 1) % 4, vals[i]) if i % 3 == 0 else ("r", (i // 2 + 1) % 4)
                                  for i in range(n_ops)])
    addr = np.array([a for _, a, _ in ops], dtype=np.uint64)
    val = dg.fr_mont([v for _, _, v in ops])
    isw = np.array([w for w, _, _ in ops], dtype=np.uint8)
    g = both_routes(tau, pp.commitment_params.srs.ctx, lambda: ts.Twist(pp).prove_soa(addr, val, isw))
    if tau != R - 1:
        assert_no_basis(pp, 8 if n_ops == 5 else 16)
    want = po.twist_prove(oracle_params(pp, rows), ops)
    assert g.address_commitment.commitment == want["address_commitment"]
    assert g.value_commitment.commitment == want["value_commitment"]
    assert g.consistency_proof.round_polynomials == want["round_polynomials"]
    assert g.consistency_proof.final_evaluation == want["final_evaluation"]
    assert [q.proof for q in g.opening_proofs] == want["opening_proofs"]
    assert g.final_evaluations == want["final_evaluations"]
    assert g.opening_point == want["opening_point"]
    assert ts.Twist.verify(g, vp)


@pytest.mark.parametrize("tau", TAUS.values(), ids=TAUS.keys())
@pytest.mark.parametrize("T,M", [(5, 3), (16, 16)])
def test_shout_small_over_degenerate_srs_matches_oracle(tau, T, M):
    pp, vp, rows = degenerate_params(tau, 2)
    entries = dg.scalar_family("uniform", 16)[:T]
    idx = [int(i) for i in np.random.default_rng(T + M).integers(0, T, size=M)]
    prove = lambda: ts.Shout(pp).prove_arrays(dg.fr_mont(entries), np.array(idx, dtype=np.uint64))  # noqa: E731
    g = both_routes(tau, pp.commitment_params.srs.ctx, prove)
    want = po.shout_prove(oracle_params(pp, rows), entries, idx)
    assert g.table_commitment.commitment == want["table_commitment"]
    assert g.index_commitment.commitment == want["index_commitment"]
    assert g.lookup_proof.round_polynomials == want["round_polynomials"]
    assert g.lookup_proof.final_evaluation == want["final_evaluation"]
    assert [q.proof for q in g.opening_proofs] == want["opening_proofs"]
    assert g.final_evaluations == want["final_evaluations"]
    assert g.opening_point == want["opening_point"]
    assert ts.Shout.verify(g, vp)


@pytest.mark.parametrize("tau", TAUS.values(), ids=TAUS.keys())
@pytest.mark.parametrize("logn", [10, 16])
def test_twist_over_degenerate_srs_trapdoor(tau, logn):
    """2^10 operations (no tables) and 2^16 (the 2^16 + 1 uploaded rows: the coefficient route's
    MSMs build the window table over them; tau = r - 1 also builds the Lagrange basis and its
    table), by the trapdoor identities C = f(tau) G and pi (tau - z) = C - v G."""
    pp, vp, _ = degenerate_params(tau, 14)
    n = 1 << logn
    addr, _, isw = ts.bench_trace(1 << 14, n)
    addr += np.uint64(7)  # (no zero entries: at a node tau the commitments are y[tau] G)
    val = scalars_mont("uniform", 1 << 16)[:n]  # full-width values
    g = both_routes(tau, pp.commitment_params.srs.ctx, lambda: ts.Twist(pp).prove_soa(addr, val, isw))
    if tau != R - 1:
        assert_no_basis(pp, n)
    Ca, Cv = g.address_commitment.commitment, g.value_commitment.commitment
    chals, z = replay(pp.fiat_shamir_seed, (b"address_commitment", b"value_commitment"), Ca, Cv, logn)
    assert g.consistency_proof.round_polynomials == [[0, 0, 0, 0]] * logn
    assert g.consistency_proof.final_evaluation == 0
    assert g.sumcheck_challenges == chals and g.opening_point == z
    check_pair(tau, n, ts.fr_from_u64_array(addr), val, (Ca, Cv), z, g.final_evaluations,
               [p.proof for p in g.opening_proofs])
    assert ts.Twist.verify(g, vp)


@pytest.mark.parametrize("tau", TAUS.values(), ids=TAUS.keys())
@pytest.mark.parametrize("logn", [10, 16])
def test_shout_over_degenerate_srs_trapdoor(tau, logn):
    pp, vp, _ = degenerate_params(tau, 14)
    n = 1 << logn
    entries = scalars_mont("uniform", 1 << 16)[:n]
    idx = np.random.default_rng(logn).integers(0, n, size=n, dtype=np.uint64)
    g = both_routes(tau, pp.commitment_params.srs.ctx, lambda: ts.Shout(pp).prove_arrays(entries, idx))
    Ct, Ci = g.table_commitment.commitment, g.index_commitment.commitment
    chals, z = replay(pp.fiat_shamir_seed, (b"table_commitment", b"index_commitment"), Ct, Ci, logn)
    assert g.lookup_proof.round_polynomials == [[0, 0, 0, 0]] * logn
    assert g.sumcheck_challenges == chals and g.opening_point == z
    check_pair(tau, n, entries, ts.fr_from_u64_array(idx), (Ct, Ci), z, g.final_evaluations,
               [p.proof for p in g.opening_proofs])
    assert ts.Shout.verify(g, vp)


# ----------------------------------------------------------------------------- C. constant columns
_PARAMS = {}


def params(L):
    if L not in _PARAMS:
        _PARAMS[L] = ts.setup_params(L)
    return _PARAMS[L]


def const_rows(c, n):
    return np.ascontiguousarray(np.tile(dg.fr_mont([c]), (n, 1)))


def assert_constant_opening(c, commitment, value, proof):
    assert commitment == co.g1_mul_gen(c)  # (None for c = 0)
    assert value == c
    assert proof is None


# N = 2^7: more than 64 nodes -- the pair pass hands the MSMs canonical quotients and their bit
# lengths; no tables.  2^12: the Lagrange basis has its window table; the quotient pass is unfused.
# 2^21: the c = 22 / W = 12 table -- the fused quotient + count pass, which plans for full-width
# quotients and skips the bit-length readback (an all-zero quotient: a sort of no entries).
# a: all-zero values; b: values r - 5; c: both columns constant; d: as a, MSM tables off
TWIST_CONST = [(logn, case) for logn in (7, 12, 21) for case in "abc"] + [(12, "d")]


@pytest.mark.parametrize("logn,case", TWIST_CONST, ids=["2^%d-%s" % c for c in TWIST_CONST])
def test_twist_constant_columns(logn, case):
    N, L = 1 << logn, logn - 2
    pp, vp = params(L)
    addr, val, isw = ts.bench_trace(1 << L, N)
    ca = None
    cv = 0 if case in "ad" else R - 5
    val = const_rows(cv, N)
    if case == "c":
        ca = 3
        addr = np.full(N, ca, dtype=np.uint64)
    ctx = pp.commitment_params.srs.ctx
    d = [ts.DeviceBuffer(ctx, x) for x in (addr, val, isw)]
    ctx.set_msm_tables(case != "d")
    try:
        g = ts.Twist(pp).prove_soa(addr, val, isw)
        res = ts.twist_proof_from_raw(ts.twist_prove_resident(pp, *d, N))
    finally:
        ctx.set_msm_tables(True)
    Ca, Cv = g.address_commitment.commitment, g.value_commitment.commitment
    proofs = [p.proof for p in g.opening_proofs]
    assert_constant_opening(cv, Cv, g.final_evaluations[1], proofs[1])
    if ca is not None:
        assert_constant_opening(ca, Ca, g.final_evaluations[0], proofs[0])
    assert res == g
    chals, z = replay(pp.fiat_shamir_seed, (b"address_commitment", b"value_commitment"), Ca, Cv, logn)
    assert g.consistency_proof.round_polynomials == [[0, 0, 0, 0]] * logn
    assert g.consistency_proof.final_evaluation == 0
    assert g.sumcheck_challenges == chals and g.opening_point == z
    check_pair(pp.commitment_params.tau, N, ts.fr_from_u64_array(addr), val, (Ca, Cv), z, g.final_evaluations, proofs)
    assert ts.Twist.verify(g, vp)
    if case == "d":  # and the table plans give the same proof
        assert ts.Twist(pp).prove_soa(addr, val, isw) == g


@pytest.mark.parametrize("n", [8, 128])
@pytest.mark.parametrize("c", [0, R - 5])
def test_open_evaluations_of_a_constant_vector(n, c):
    pp, _ = params(8)
    cp = pp.commitment_params
    y = const_rows(c, n)
    z = dg.scalar_family("uniform", 16)[n % 16]
    v, pi = ts.KZGCommitment.open_evaluations(cp, y, z)
    assert_constant_opening(c, ts.KZGCommitment.commit_evaluations(cp, y).commitment, v, pi.proof)
    ctx = cp.srs.ctx
    ctx.set_commit_basis(False)
    try:
        v, pi = ts.KZGCommitment.open_evaluations(cp, y, z)
        assert_constant_opening(c, ts.KZGCommitment.commit_evaluations(cp, y).commitment, v, pi.proof)
    finally:
        ctx.set_commit_basis(True)


def test_open_coefficients_with_zero_quotient():
    """The coefficient route with n > 1 and a quotient that is all zero: [c, 0, 0, 0, 0]."""
    pp, _ = params(8)
    cp = pp.commitment_params
    c = R - 5
    z = dg.scalar_family("uniform", 16)[3]
    v, pi = ts.KZGCommitment.open(cp, [c, 0, 0, 0, 0], z)
    assert_constant_opening(c, ts.KZGCommitment.commit(cp, [c, 0, 0, 0, 0]).commitment, v, pi.proof)


def _check_one(tau, y, C, z, v, pi):
    """One committed vector against the trapdoor identities (check_pair for a single vector)."""
    w = co.bary_weights(len(y))
    ft, _, _ = co.bary_eval2(w, y, y, tau, host_threads())
    fz, _, _ = co.bary_eval2(w, y, y, z, host_threads())
    assert C == co.g1_mul_gen(ft) and v == fz
    assert co.g1_mul(pi, (tau - z) % R) == po.affine_add(C, po.g1_neg(co.g1_mul_gen(v)))


# T = 2^7 entries; M = 3 2^5 lookups pad to 2^7 nodes as well (both openings share one pass),
# M = 3 2^6 to 2^8: two single-vector openings
@pytest.mark.parametrize("M", [3 << 5, 3 << 6])
def test_shout_constant_table(M):
    pp, vp = params(8)
    T, c = 1 << 7, R - 5
    entries = const_rows(c, T)
    idx = np.random.default_rng(M).integers(0, T, size=M, dtype=np.uint64)
    g = ts.Shout(pp).prove_arrays(entries, idx)
    ctx = pp.commitment_params.srs.ctx
    raw = ts.shout_prove_resident(pp, ts.DeviceBuffer(ctx, entries), T, ts.DeviceBuffer(ctx, idx), M)
    assert ts.shout_proof_from_raw(raw) == g
    Ct, Ci = g.table_commitment.commitment, g.index_commitment.commitment
    proofs = [p.proof for p in g.opening_proofs]
    assert_constant_opening(c, Ct, g.final_evaluations[0], proofs[0])
    nv = (M - 1).bit_length()
    chals, z = replay(pp.fiat_shamir_seed, (b"table_commitment", b"index_commitment"), Ct, Ci, nv)
    assert g.lookup_proof.round_polynomials == [[0, 0, 0, 0]] * nv
    assert g.sumcheck_challenges == chals and g.opening_point == z
    padded = np.zeros(1 << nv, dtype=np.uint64)
    padded[:M] = idx
    _check_one(pp.commitment_params.tau, ts.fr_from_u64_array(padded), Ci, z, g.final_evaluations[1], proofs[1])
    assert ts.Shout.verify(g, vp)
