"""Every opening of a KZG vector commitment in one pass (tns_vc_open_all / tns_vc_open_many,
vc_open.hip; the batched form of KZGVectorCommitment::open, src/commitments.rs:435-471): pinned
index by index to the per-index opening (itself pinned to the oracle by test_gpu_vector.py), to the
trapdoor identity pi_i = [(f(tau) - v_i) / (tau - i)]G over all indices at once, and to closed
forms that need no oracle."""
import numpy as np
import pytest

from oracle import pyoracle as po

import twist_and_shout as ts
from twist_and_shout import _native as N

pytestmark = pytest.mark.gpu
R = po.R_MOD
P = po.P_MOD

_P = {}


def params(L):
    if L not in _P:
        _P[L] = ts.setup_params(L)
    return _P[L]


def rand_vals(n, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)]


def points(rows):
    """(n, 8) affine Montgomery limbs -> [None | (x, y)]"""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 8)
    xs = ts.from_mont(rows[:, :4], P)
    ys = ts.from_mont(rows[:, 4:], P)
    return [None if not row.any() else (x, y) for row, x, y in zip(rows, xs, ys)]


def limbs(pts):
    """[None | (x, y)] -> (n, 8) affine Montgomery limbs"""
    out = np.zeros((len(pts), 8), dtype=np.uint64)
    for i, p in enumerate(pts):
        if p is not None:
            out[i, :4] = ts.to_mont([p[0]], P)[0]
            out[i, 4:] = ts.to_mont([p[1]], P)[0]
    return out


def check_trapdoor(cp, vec, proofs, seed):
    """sum_i r_i pi_i == [sum_i r_i (f(tau) - v_i) / (tau - i)] G for random r: every index at once."""
    n, tau = len(vec), cp.tau
    r = rand_vals(n, seed)
    got = ts.msm(ts.CommitmentParams.from_g1_limbs(proofs), r)
    ftau = po.barycentric_eval(vec, tau)
    s = sum(ri * (ftau - v) % R * pow((tau - i) % R, -1, R) for i, (ri, v) in enumerate(zip(r, vec))) % R
    assert got == (po.affine_mul(po.G1_GEN, s) if s else None)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 40])
def test_open_all_equals_open_at_every_index(n):
    pp, vp = params(6)
    cp = pp.commitment_params
    vec = rand_vals(n, seed=100 + n)
    got = points(ts.KZGVectorCommitment.open_all(cp, vec))
    assert len(got) == n
    for i in range(n):
        v, pi = ts.KZGVectorCommitment.open(cp, vec, i)
        assert v == vec[i] and got[i] == pi.proof
    if n == 5:
        Cm = ts.KZGVectorCommitment.commit(cp, vec)
        for i in (0, n - 1):
            pi = ts.KZGProof(got[i])
            assert ts.KZGVectorCommitment.verify(vp.commitment_vk, Cm, i, vec[i], pi)
            assert not ts.KZGVectorCommitment.verify(vp.commitment_vk, Cm, i, (vec[i] + 1) % R, pi)


@pytest.mark.parametrize("n", [64, 100, 1024, 2048, 4096, 5000])
def test_open_all_trapdoor_every_index(n):
    pp, _ = params(11)
    cp = pp.commitment_params
    vec = rand_vals(n, seed=n)
    proofs = ts.KZGVectorCommitment.open_all(cp, vec)
    assert proofs.shape == (n, 8)
    check_trapdoor(cp, vec, proofs, seed=n + 1)
    got = points(proofs)
    for i in sorted({0, 1, n // 7, n // 3, n // 2, (2 * n) // 3, n - 2, n - 1}):
        v, pi = ts.KZGVectorCommitment.open(cp, vec, i)
        assert v == vec[i] and got[i] == pi.proof, i


@pytest.mark.parametrize("n", [1024, 37])
def test_open_all_closed_forms(n):
    pp, _ = params(11)
    cp = pp.commitment_params
    g = cp.srs.download(2)  # G, [tau]G
    for c in (0, 12345, R - 1):  # f constant: q_i = 0
        assert not ts.KZGVectorCommitment.open_all(cp, [c] * n).any()
    got = ts.KZGVectorCommitment.open_all(cp, list(range(n)))  # f = x: q_i = 1
    assert np.array_equal(got, np.tile(g[0], (n, 1)))
    got = ts.KZGVectorCommitment.open_all(cp, [i * i for i in range(n)])  # f = x^2: q_i = x + i
    tau_g = points(g[1:2])[0]
    acc, want = tau_g, []
    for i in range(n):
        want.append(acc)
        acc = po.affine_add(acc, po.G1_GEN)
    assert np.array_equal(got, limbs(want))


@pytest.mark.parametrize("n", [1024, 37])
def test_open_all_small_and_extreme_entries(n):
    pp, _ = params(11)
    cp = pp.commitment_params
    rng = np.random.default_rng(n)
    small = [int(x) for x in rng.integers(0, 1 << 63, size=n, dtype=np.uint64)]
    check_trapdoor(cp, small, ts.KZGVectorCommitment.open_all(cp, small), seed=7)
    extreme = [R - 1 if i % 3 else (i * i + 1) % R for i in range(n)]
    check_trapdoor(cp, extreme, ts.KZGVectorCommitment.open_all(cp, extreme), seed=8)


def test_open_all_reuses_the_cached_correlation():
    pp, _ = params(11)
    cp = pp.commitment_params
    n = 300
    for seed in (1, 2):  # the second call finds A in the SRS
        vec = rand_vals(n, seed)
        proofs = ts.KZGVectorCommitment.open_all(cp, vec)
        check_trapdoor(cp, vec, proofs, seed=seed + 10)
        assert points(proofs[n - 1:])[0] == ts.KZGVectorCommitment.open(cp, vec, n - 1)[1].proof


def test_prepare_open_all_gives_the_same_proofs():
    n = 40
    vec = rand_vals(n, seed=3)
    want = ts.KZGVectorCommitment.open_all(params(6)[0].commitment_params, vec)
    fresh, _ = ts.setup_params(6)  # a second SRS of the same setup, prepared ahead
    fresh.commitment_params.srs.prepare_open_all(n)
    assert np.array_equal(ts.KZGVectorCommitment.open_all(fresh.commitment_params, vec), want)


def test_open_all_on_a_tau_free_srs():
    pp, _ = params(6)
    cp = pp.commitment_params
    n = 64
    vec = rand_vals(n, seed=4)
    want = ts.KZGVectorCommitment.open_all(cp, vec)
    free = ts.CommitmentParams.from_g1_limbs(cp.srs.download())
    with pytest.raises(ts.InvalidParameters) as e:  # no tau, nothing prepared or attached
        ts.KZGVectorCommitment.open_all(free, vec)
    assert "tns_srs_prepare_lagrange_from_powers" in str(e.value) and "tns_srs_set_tau" in str(e.value)
    free.srs.prepare_lagrange_from_powers(n)
    assert np.array_equal(ts.KZGVectorCommitment.open_all(free, vec), want)


def test_open_all_ignores_the_commit_basis_setting():
    pp, _ = params(6)
    cp = pp.commitment_params
    vec = rand_vals(17, seed=5)
    want = ts.KZGVectorCommitment.open_all(cp, vec)
    cp.srs.ctx.set_commit_basis(False)
    try:
        assert np.array_equal(ts.KZGVectorCommitment.open_all(cp, vec), want)
    finally:
        cp.srs.ctx.set_commit_basis(True)


def test_open_many_request_order_and_duplicates():
    pp, _ = params(6)
    cp = pp.commitment_params
    n = 40
    vec = rand_vals(n, seed=6)
    idx = [39, 0, 17, 17, 3, 39]
    got = ts.KZGVectorCommitment.open_many(cp, vec, idx)
    assert got == [ts.KZGVectorCommitment.open(cp, vec, i) for i in idx]
    assert ts.KZGVectorCommitment.open_many(cp, vec, []) == []


def test_open_many_all_index_route_agrees_with_per_index_route():
    pp, _ = params(6)
    cp = pp.commitment_params
    n = 64  # M = 128: more than 8 * 7 = 56 indices take the all-index pass
    vec = rand_vals(n, seed=7)
    idx = [(7 * t + 3) % n for t in range(57)] + [5, 5]
    many = ts.KZGVectorCommitment.open_many(cp, vec, idx)
    each = (ts.KZGVectorCommitment.open_many(cp, vec, list(range(32))) +  # 32 <= 56: index by index
            ts.KZGVectorCommitment.open_many(cp, vec, list(range(32, n))))
    assert each[5] == ts.KZGVectorCommitment.open(cp, vec, 5)
    assert many == [each[i] for i in idx]


def test_open_all_resident_equals_host_call():
    pp, _ = params(11)
    cp = pp.commitment_params
    n = 1024
    vec = ts.to_mont(rand_vals(n, seed=8))
    want = ts.KZGVectorCommitment.open_all(cp, vec)
    ctx = cp.srs.ctx
    d_vec = ts.DeviceBuffer(ctx, vec)
    d_out = ts.DeviceBuffer(ctx, np.zeros((n, 8), dtype=np.uint64))
    ts.vc_open_all_resident(cp, d_vec, n, d_out)
    got = np.zeros((n, 8), dtype=np.uint64)
    ts.buffer_download(d_out, got)
    assert np.array_equal(got, want)


# ---- errors: the mirror's exception class, and through the C ABI that no output is written
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)


def raw_open_all(cp, vec, n):
    out = np.full((max(n, 1) + 1, 8), SENTINEL, dtype=np.uint64)
    st = N.load().tns_vc_open_all(cp.srs.ctx.handle, cp.srs.handle, N.p64(vec), n, N.p64(out))
    return st, bool((out == SENTINEL).all())


def raw_open_many(cp, vec, n, idx):
    idx = np.asarray(idx, dtype=np.uint64)
    v = np.full((len(idx), 4), SENTINEL, dtype=np.uint64)
    pi = np.full((len(idx), 12), SENTINEL, dtype=np.uint64)
    st = N.load().tns_vc_open_many(cp.srs.ctx.handle, cp.srs.handle, N.p64(vec), n, N.p64(idx), len(idx), N.p64(v),
                                   N.p64(pi))
    return st, bool((v == SENTINEL).all() and (pi == SENTINEL).all())


def test_errors_empty_vector():
    cp = params(6)[0].commitment_params
    with pytest.raises(ts.PolynomialError) as e:
        ts.KZGVectorCommitment.open_all(cp, [])
    assert "empty evaluation vector" in str(e.value)
    with pytest.raises(ts.PolynomialError):
        ts.KZGVectorCommitment.open_many(cp, [], [0])
    with pytest.raises(ts.PolynomialError):
        cp.srs.prepare_open_all(0)
    one = ts.to_mont([1])
    assert raw_open_all(cp, one, 0) == (5, True)
    assert raw_open_many(cp, one, 0, [0]) == (5, True)


def test_errors_vector_longer_than_the_srs():
    cp = params(3)[0].commitment_params
    n = len(cp.srs) + 1
    vec = ts.to_mont(list(range(n)))
    with pytest.raises(ts.CommitmentError) as e:
        ts.KZGVectorCommitment.open_all(cp, vec)
    assert "Polynomial degree exceeds setup size" in str(e.value)
    with pytest.raises(ts.CommitmentError):
        ts.KZGVectorCommitment.open_many(cp, vec, [0])
    with pytest.raises(ts.CommitmentError):
        cp.srs.prepare_open_all(n)
    assert raw_open_all(cp, vec, n) == (4, True)
    assert raw_open_many(cp, vec, n, [0]) == (4, True)


def test_errors_index_out_of_bounds():
    cp = params(6)[0].commitment_params
    vec = ts.to_mont([1, 2, 3])
    with pytest.raises(ts.CommitmentError) as e:
        ts.KZGVectorCommitment.open_many(cp, vec, [0, 3, 1])
    assert "Index out of bounds" in str(e.value)
    assert raw_open_many(cp, vec, 3, [0, 1, 2, 3]) == (4, True)  # the valid ones are not written either


def test_errors_sharded_srs():
    pp, _ = ts.setup_params_shard(4, 1, 2)
    cp = pp.commitment_params
    vec = ts.to_mont([1, 2, 3, 4])
    with pytest.raises(ts.InvalidParameters):
        ts.KZGVectorCommitment.open_all(cp, vec)
    with pytest.raises(ts.InvalidParameters):
        ts.KZGVectorCommitment.open_many(cp, vec, [0])
    with pytest.raises(ts.InvalidParameters):
        cp.srs.prepare_open_all(4)
    assert raw_open_all(cp, vec, 4) == (1, True)
    assert raw_open_many(cp, vec, 4, [0]) == (1, True)


def test_errors_no_lagrange_basis():
    cp = params(6)[0].commitment_params
    free = ts.CommitmentParams.from_g1_limbs(cp.srs.download(16))
    vec = ts.to_mont(list(range(1, 6)))
    with pytest.raises(ts.InvalidParameters) as e:
        ts.KZGVectorCommitment.open_all(free, vec)
    for call in ("tns_srs_set_tau", "tns_srs_prepare_lagrange_from_powers", "tns_srs_lagrange_deserialize"):
        assert call in str(e.value)
    with pytest.raises(ts.InvalidParameters):
        free.srs.prepare_open_all(5)
    assert raw_open_all(free, vec, 5) == (1, True)
    d_vec = ts.DeviceBuffer(free.srs.ctx, vec)
    d_out = ts.DeviceBuffer(free.srs.ctx, np.full((5, 8), SENTINEL, dtype=np.uint64))
    with pytest.raises(ts.InvalidParameters):
        ts.vc_open_all_resident(free, d_vec, 5, d_out)
    back = np.zeros((5, 8), dtype=np.uint64)
    ts.buffer_download(d_out, back)
    assert (back == SENTINEL).all()


def test_errors_null_pointers_with_a_live_context():
    cp = params(6)[0].commitment_params
    lib, ctx, srs = N.load(), cp.srs.ctx.handle, cp.srs.handle
    vec = ts.to_mont([1, 2])
    out = np.full((2, 12), SENTINEL, dtype=np.uint64)
    idx = np.zeros(2, dtype=np.uint64)
    assert lib.tns_vc_open_all(ctx, srs, None, 2, N.p64(out)) == 1
    assert lib.tns_vc_open_all(ctx, srs, N.p64(vec), 2, None) == 1
    assert lib.tns_vc_open_all_device(ctx, srs, None, 2, None) == 1
    assert lib.tns_vc_open_many(ctx, srs, N.p64(vec), 2, None, 2, N.p64(out), N.p64(out)) == 1
    assert lib.tns_vc_open_many(ctx, srs, N.p64(vec), 2, N.p64(idx), 2, None, N.p64(out)) == 1
    assert lib.tns_vc_open_many(ctx, srs, N.p64(vec), 2, N.p64(idx), 2, N.p64(out), None) == 1
    assert lib.tns_vc_open_many(ctx, srs, N.p64(vec), 2, None, 0, None, None) == 0  # k == 0 needs none of them
    assert (out == SENTINEL).all()
