"""The sound batched KZG verifier (tns_kzg_verify_many, tns_vc_verify_all, tns_vc_verify_all_device;
kzg_verify.hip): honest batches accept, every tamper is rejected and located at its lowest index,
malformed points are refused before any MSM, and the challenge derivation is pinned by a pair of
errors built to cancel for one known seed."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po

import twist_and_shout as ts
from twist_and_shout import _native as N

pytestmark = pytest.mark.gpu
R = po.R_MOD
P = po.P_MOD
VC = ts.KZGVectorCommitment

_P = {}
_BASE = {}


def params(L):
    if L not in _P:
        _P[L] = ts.setup_params(L)
    return _P[L]


def params_for(n):
    return params(6 if n <= 257 else 11)  # 4 * 2^L + 1 SRS points


def rand_vals(n, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)]


def point(row):
    """8 affine Montgomery limbs -> None | (x, y)"""
    row = np.asarray(row, dtype=np.uint64).reshape(8)
    if not row.any():
        return None
    return (ts.from_mont(row[:4], P)[0], ts.from_mont(row[4:], P)[0])


def limbs(p):
    out = np.zeros(8, dtype=np.uint64)
    if p is not None:
        out[:4] = ts.to_mont([p[0]], P)[0]
        out[4:] = ts.to_mont([p[1]], P)[0]
    return out


def base(n):
    """One honest vector of n entries with its commitment and all its proofs, shared and never modified."""
    if n not in _BASE:
        pp, vp = params_for(n)
        vec = rand_vals(n, seed=9000 + n)
        mont = ts.to_mont(vec)
        cm = VC.commit(pp.commitment_params, mont)
        _BASE[n] = (vp.commitment_vk, vec, mont, cm, VC.open_all(pp.commitment_params, mont))
    return _BASE[n]


def single(vk, cm, i, value, proof_row):
    return VC.verify(vk, cm, i, value, ts.KZGProof(point(proof_row)))


# ---- 1. honest batches
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 257, 5000])
def test_honest_batches_accept(n):
    pp, vp = params_for(n)
    cp = pp.commitment_params
    vec = ts.fr_rand_batch(bytes([n % 251] * 32), n)
    cm = VC.commit(cp, vec)
    proofs = VC.open_all(cp, vec)
    assert VC.verify_all(vp.commitment_vk, cm, vec, proofs) is True
    assert VC.verify_all(vp.commitment_vk, cm, vec, proofs, locate=True) == (True, None)


def test_honest_batch_agrees_with_verify_at_every_index():
    pp, vp = params(6)
    cp, vk = pp.commitment_params, vp.commitment_vk
    vec = rand_vals(5, seed=55)
    cm = VC.commit(cp, vec)
    proofs = VC.open_all(cp, vec)
    assert all(single(vk, cm, i, vec[i], proofs[i]) for i in range(5))
    assert VC.verify_all(vk, cm, vec, proofs)
    assert VC.verify_all(vk, cm, vec, [ts.KZGProof(point(r)) for r in proofs])  # a list of KZGProof
    assert not single(vk, cm, 3, (vec[3] + 1) % R, proofs[3])
    wrong = vec[:3] + [(vec[3] + 1) % R] + vec[4:]
    assert VC.verify_all(vk, cm, wrong, proofs, locate=True) == (False, 3)


def test_resident_form_gives_the_same_answer():
    n = 1024
    vk, vec, mont, cm, proofs = base(n)
    ctx = params_for(n)[0].commitment_params.srs.ctx
    d_vec, d_pi = ts.DeviceBuffer(ctx, mont), ts.DeviceBuffer(ctx, proofs)
    assert ts.vc_verify_all_resident(vk, cm, d_vec, n, d_pi) is True
    assert ts.vc_verify_all_resident(vk, cm, d_vec, n, d_pi, locate=True) == VC.verify_all(vk, cm, mont, proofs,
                                                                                          locate=True)
    bad = mont.copy()
    bad[700] = ts.to_mont([5])[0]
    d_bad = ts.DeviceBuffer(ctx, bad)
    assert ts.vc_verify_all_resident(vk, cm, d_bad, n, d_pi) is False
    assert ts.vc_verify_all_resident(vk, cm, d_bad, n, d_pi, locate=True) == (False, 700)


# ---- 2. indices beyond 16 bits
def test_above_2_16_entries():
    n = 66000
    pp, vp = params(15)
    cp, vk = pp.commitment_params, vp.commitment_vk
    vec = ts.fr_rand_batch(bytes([66] * 32), n)
    cm = VC.commit(cp, vec)
    proofs = VC.open_all(cp, vec)
    assert VC.verify_all(vk, cm, vec, proofs) is True
    vec[n - 1] = ts.to_mont([12345])[0]
    assert VC.verify_all(vk, cm, vec, proofs, locate=True) == (False, n - 1)


# ---- 3. degenerate but valid bases
@pytest.mark.parametrize("n", [37, 1024])
def test_degenerate_bases_accept(n):
    pp, vp = params_for(n)
    cp, vk = pp.commitment_params, vp.commitment_vk
    const = [777] * n  # every proof is the identity
    proofs = VC.open_all(cp, const)
    assert not proofs.any()
    assert VC.verify_all(vk, VC.commit(cp, const), const, proofs, locate=True) == (True, None)
    ramp = list(range(n))  # f = x: every proof is G
    proofs = VC.open_all(cp, ramp)
    assert np.array_equal(proofs, np.tile(limbs(po.G1_GEN), (n, 1)))
    assert VC.verify_all(vk, VC.commit(cp, ramp), ramp, proofs, locate=True) == (True, None)


# ---- 4. tampers are rejected and located
@pytest.mark.parametrize("n", [40, 1024])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_changed_value_is_located(n, where):
    vk, vec, mont, cm, proofs = base(n)
    i = {"first": 0, "middle": n // 2, "last": n - 1}[where]
    bad = mont.copy()
    bad[i] = ts.to_mont([(vec[i] + 1) % R])[0]
    assert VC.verify_all(vk, cm, bad, proofs) is False
    assert VC.verify_all(vk, cm, bad, proofs, locate=True) == (False, i)
    assert not single(vk, cm, i, (vec[i] + 1) % R, proofs[i])


@pytest.mark.parametrize("n", [40, 1024])
def test_swapped_proofs_report_the_lower_index(n):
    vk, vec, mont, cm, proofs = base(n)
    i, j = n // 3, n - 2
    bad = proofs.copy()
    bad[[i, j]] = proofs[[j, i]]
    assert VC.verify_all(vk, cm, mont, bad, locate=True) == (False, i)
    assert not single(vk, cm, i, vec[i], bad[i]) and not single(vk, cm, j, vec[j], bad[j])


@pytest.mark.parametrize("n", [40, 1024])
def test_identity_in_place_of_a_proof(n):
    vk, vec, mont, cm, proofs = base(n)
    i = n // 2 + 1
    bad = proofs.copy()
    bad[i] = 0
    assert VC.verify_all(vk, cm, mont, bad, locate=True) == (False, i)
    assert not single(vk, cm, i, vec[i], bad[i])


@pytest.mark.parametrize("n", [40, 1024])
def test_wrong_commitment_reports_index_0(n):
    vk, vec, mont, cm, proofs = base(n)
    other = ts.KZGCommitmentValue(po.affine_mul(po.G1_GEN, 31337))
    assert VC.verify_all(vk, other, mont, proofs) is False
    assert VC.verify_all(vk, other, mont, proofs, locate=True) == (False, 0)
    assert not single(vk, other, 0, vec[0], proofs[0])


@pytest.mark.parametrize("n", [40, 1024])
def test_two_bad_values_report_the_lower(n):
    vk, vec, mont, cm, proofs = base(n)
    i, j = n // 4, (3 * n) // 4
    bad = mont.copy()
    bad[i] = ts.to_mont([(vec[i] + 2) % R])[0]
    bad[j] = ts.to_mont([(vec[j] + 3) % R])[0]
    assert VC.verify_all(vk, cm, bad, proofs, locate=True) == (False, i)
    assert not single(vk, cm, i, (vec[i] + 2) % R, proofs[i])


# ---- 5. malformed points
P_LIMBS = np.array([(P >> (64 * t)) & ((1 << 64) - 1) for t in range(4)], dtype=np.uint64)


def corrupt(row, how):
    row = row.copy()
    if how == "y_limb":  # off the curve
        row[5] ^= np.uint64(1 << 17)
    elif how == "x_is_p":  # a coordinate that is no field element
        row[:4] = P_LIMBS
    else:  # x = 0 with the proof's y: not on y^2 = 3
        assert how == "x_zero" and row[4:].any()
        row[:4] = 0
    return row


@pytest.mark.parametrize("how", ["y_limb", "x_is_p", "x_zero"])
@pytest.mark.parametrize("pos", [0, 150, 299])
def test_malformed_proof_is_refused_at_its_position(how, pos):
    n = 300
    vk, vec, mont, cm, proofs = base(n)
    bad = proofs.copy()
    bad[pos] = corrupt(proofs[pos], how)
    assert VC.verify_all(vk, cm, mont, bad) is False
    assert VC.verify_all(vk, cm, mont, bad, locate=True) == (False, pos)


def test_two_malformed_proofs_report_the_lower():
    n = 300
    vk, vec, mont, cm, proofs = base(n)
    bad = proofs.copy()
    bad[260] = corrupt(proofs[260], "x_is_p")
    bad[41] = corrupt(proofs[41], "y_limb")
    assert VC.verify_all(vk, cm, mont, bad, locate=True) == (False, 41)


def raw_verify_many(ctx, vk, cs, z, v, pis, k, seed=None):
    ok, bad = C.c_int(-7), C.c_uint64(77)
    st = N.load().tns_kzg_verify_many(ctx.handle, C.byref(vk.raw), N.p64(cs), len(cs), N.p64(z), N.p64(v), N.p64(pis), k,
                                      seed, C.byref(ok), C.pointer(bad))
    return st, ok.value, bad.value


def test_malformed_commitment_reports_its_tuple():
    n = 300
    vk, vec, mont, cm, proofs = base(n)
    ctx = params_for(n)[0].commitment_params.srs.ctx
    cs = np.tile(limbs(cm.commitment), (n, 1))
    z = ts.fr_from_u64_array(np.arange(n, dtype=np.uint64))
    assert raw_verify_many(ctx, vk, cs, z, mont, proofs, n) == (0, 1, 77)  # honest: bad_index untouched
    cs[123] = corrupt(cs[123], "y_limb")
    assert raw_verify_many(ctx, vk, cs, z, mont, proofs, n) == (0, 0, 123)
    pis = proofs.copy()
    pis[200] = corrupt(pis[200], "x_zero")  # a commitment and a later proof: the lower position
    assert raw_verify_many(ctx, vk, cs, z, mont, pis, n) == (0, 0, 123)
    one = corrupt(limbs(cm.commitment), "x_is_p").reshape(1, 8)  # the shared commitment stands at every tuple
    assert raw_verify_many(ctx, vk, one, z, mont, proofs, n) == (0, 0, 0)


# ---- 6. the challenges are the documented ones, and a known seed can be played
@pytest.mark.parametrize("n,a,b", [(40, 3, 17), (1024, 1, 1023)])
def test_errors_built_for_a_known_seed_cancel_for_that_seed_only(n, a, b):
    vk, vec, mont, cm, proofs = base(n)
    tau = params_for(n)[0].commitment_params.tau
    seed = bytes([(7 * t + n) % 256 for t in range(32)])
    gam = ts.verify_challenges(seed, 0, n)
    # pi_i + e_i G leaves (i - tau) e_i in opening i's equation: the two weighted terms cancel
    e_a = gam[b] * (b - tau) % R
    e_b = -gam[a] * (a - tau) % R
    bad = proofs.copy()
    bad[a] = limbs(po.affine_add(point(proofs[a]), po.affine_mul(po.G1_GEN, e_a)))
    bad[b] = limbs(po.affine_add(point(proofs[b]), po.affine_mul(po.G1_GEN, e_b)))
    assert not single(vk, cm, a, vec[a], bad[a]) and not single(vk, cm, b, vec[b], bad[b])
    assert VC.verify_all(vk, cm, mont, bad, seed=seed, locate=True) == (True, None)
    assert VC.verify_all(vk, cm, mont, bad, seed=bytes(32), locate=True) == (False, min(a, b))
    assert VC.verify_all(vk, cm, mont, bad, seed=None, locate=True) == (False, min(a, b))


# ---- 7. the general form
def test_general_form_two_polynomials():
    pp, vp = params(6)
    cp, vk = pp.commitment_params, vp.commitment_vk
    polys = [rand_vals(10, seed=71), rand_vals(23, seed=72)]
    cms = [ts.KZGCommitment.commit(cp, f) for f in polys]
    which = [0, 1, 1, 0, 1, 0]
    zs = rand_vals(6, seed=73)
    opened = [ts.KZGCommitment.open(cp, polys[w], z) for w, z in zip(which, zs)]
    which, zs, opened = which + [which[2]], zs + [zs[2]], opened + [opened[2]]  # one tuple twice
    cs, vs, pis = [cms[w] for w in which], [o[0] for o in opened], [o[1] for o in opened]
    assert ts.KZGCommitment.verify_many(vk, cs, zs, vs, pis) is True
    assert ts.KZGCommitment.verify_many(vk, cs, zs, vs, pis, locate=True) == (True, None)
    vs[4] = (vs[4] + 1) % R
    assert ts.KZGCommitment.verify_many(vk, cs, zs, vs, pis) is False
    assert ts.KZGCommitment.verify_many(vk, cs, zs, vs, pis, locate=True) == (False, 4)
    assert not ts.KZGCommitment.verify(vk, cs[4], zs[4], vs[4], pis[4])


def test_general_form_shared_commitment_and_lengths():
    pp, vp = params(6)
    cp, vk = pp.commitment_params, vp.commitment_vk
    f = rand_vals(12, seed=74)
    cm = ts.KZGCommitment.commit(cp, f)
    zs = rand_vals(4, seed=75)
    opened = [ts.KZGCommitment.open(cp, f, z) for z in zs]
    vs, pis = [o[0] for o in opened], [o[1] for o in opened]
    assert ts.KZGCommitment.verify_many(vk, [cm], zs, vs, pis, locate=True) == (True, None)
    vs[1] = (vs[1] + 1) % R
    assert ts.KZGCommitment.verify_many(vk, [cm], zs, vs, pis, locate=True) == (False, 1)
    assert ts.KZGCommitment.verify_many(vk, [], [], [], []) is True  # k == 0
    assert ts.KZGCommitment.verify_many(vk, [], [], [], [], locate=True) == (True, None)
    with pytest.raises(ts.CommitmentError) as e:
        ts.KZGCommitment.verify_many(vk, [cm, cm], zs[:3], vs[:3], pis[:3])
    assert "Batch verify input lengths must match" in str(e.value)


def test_general_form_many_tuples_over_two_vectors():
    """One commitment per opening beyond the MSM's 64-point path, explicit points: the first half of
    one vector's openings and the second half of another's."""
    n, h = 300, 150
    vk, vec, mont, cm, proofs = base(n)
    pp, _ = params_for(n)
    vec2 = rand_vals(n, seed=76)
    mont2 = ts.to_mont(vec2)
    cm2 = VC.commit(pp.commitment_params, mont2)
    proofs2 = VC.open_all(pp.commitment_params, mont2)
    cs = [cm] * h + [cm2] * (n - h)
    zs = list(range(n))
    vs = np.concatenate([mont[:h], mont2[h:]])
    pis = np.concatenate([proofs[:h], proofs2[h:]])
    assert ts.KZGCommitment.verify_many(vk, cs, zs, vs, pis, locate=True) == (True, None)
    for i in (h - 1, 217):  # the other vector's proof at i: rejected, located through both MSM paths
        bad = pis.copy()
        bad[i] = (proofs2 if i < h else proofs)[i]
        assert ts.KZGCommitment.verify_many(vk, cs, zs, vs, bad, locate=True) == (False, i)
    cs[h], cs[h - 1] = cs[h - 1], cs[h]
    assert ts.KZGCommitment.verify_many(vk, cs, zs, vs, pis, locate=True) == (False, h - 1)


# ---- 8. errors through the raw ABI: status 1, nothing written
def test_null_arrays_with_a_live_context():
    vk, vec, mont, cm, proofs = base(40)
    lib, ctx = N.load(), params_for(40)[0].commitment_params.srs.ctx.handle
    cs = limbs(cm.commitment).reshape(1, 8)
    proj = np.concatenate([cs[0], ts.to_mont([1], P)[0]])
    z = ts.fr_from_u64_array(np.arange(40, dtype=np.uint64))
    ok, bad = C.c_int(-7), C.c_uint64(77)
    okp, badp, vkp = C.byref(ok), C.pointer(bad), C.byref(vk.raw)
    many = lib.tns_kzg_verify_many
    assert many(ctx, vkp, None, 1, N.p64(z), N.p64(mont), N.p64(proofs), 40, None, okp, badp) == 1
    assert many(ctx, vkp, N.p64(cs), 1, None, N.p64(mont), N.p64(proofs), 40, None, okp, badp) == 1
    assert many(ctx, vkp, N.p64(cs), 1, N.p64(z), None, N.p64(proofs), 40, None, okp, badp) == 1
    assert many(ctx, vkp, N.p64(cs), 1, N.p64(z), N.p64(mont), None, 40, None, okp, badp) == 1
    assert many(ctx, None, N.p64(cs), 1, N.p64(z), N.p64(mont), N.p64(proofs), 40, None, okp, badp) == 1
    assert many(ctx, vkp, N.p64(cs), 1, N.p64(z), N.p64(mont), N.p64(proofs), 40, None, None, badp) == 1
    assert many(ctx, vkp, N.p64(cs), 2, N.p64(z), N.p64(mont), N.p64(proofs), 40, None, okp, badp) == 4
    assert lib.tns_vc_verify_all(ctx, vkp, None, N.p64(mont), 40, N.p64(proofs), None, okp, badp) == 1
    assert lib.tns_vc_verify_all(ctx, vkp, N.p64(proj), None, 40, N.p64(proofs), None, okp, badp) == 1
    assert lib.tns_vc_verify_all(ctx, vkp, N.p64(proj), N.p64(mont), 40, None, None, okp, badp) == 1
    assert lib.tns_vc_verify_all_device(ctx, vkp, N.p64(proj), None, 40, None, None, okp, badp) == 1
    assert lib.tns_vc_verify_all_device(ctx, vkp, N.p64(proj), None, 40, None, None, None, None) == 1
    assert ok.value == -7 and bad.value == 77
    assert lib.tns_vc_verify_all(ctx, vkp, N.p64(proj), N.p64(mont), 40, N.p64(proofs), None, okp, None) == 0
    assert ok.value == 1 and bad.value == 77  # bad_index may be NULL, and is written only on failure
