"""SRS files (csrc/srs_io.hip): g1_powers and the Lagrange basis as ark-serialize 0.4 writes a
Vec<G1Affine> (u64 LE count, then 32 / 64 bytes a point), encoded, decoded and validated on the
device.  The encoder is pinned by the oracle's g1_serialize, the decoder by bit-equal round trips
and by the rejections of serialize.cpp's g1_deserialize, and a stored Lagrange basis must pass the
random check against g1_powers before a tau-less SRS proves through it."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from oracle import pyoracle as po

import twist_and_shout as ts
from twist_and_shout import _native as N

pytestmark = pytest.mark.gpu

P = po.P_MOD
SEEDS = [bytes(range(32)), None]
_PARAMS, _BYTES = {}, {}


def params(L):
    """setup_params(L): 4 * 2^L + 1 points (5, 17, 257 -- a partial last workgroup --, 1025, ...)."""
    if L not in _PARAMS:
        _PARAMS[L] = ts.setup_params(L)[0]
    return _PARAMS[L]


def srs_of(L):
    return params(L).commitment_params.srs


def file_of(L, compressed):
    if (L, compressed) not in _BYTES:
        _BYTES[L, compressed] = srs_of(L).serialize(compressed)
    return _BYTES[L, compressed]


def header(n):
    return n.to_bytes(8, "little")


def points_of(limbs):
    xs, ys = ts.from_mont(limbs[:, :4], P), ts.from_mont(limbs[:, 4:], P)
    return [None if x == 0 and y == 0 else (x, y) for x, y in zip(xs, ys)]


def oracle_file(points, compressed):
    return header(len(points)) + b"".join(po.g1_serialize(Q, compressed) for Q in points)


def split(data, compressed):
    sz = 32 if compressed else 64
    assert (len(data) - 8) % sz == 0
    return [bytearray(data[8 + i * sz:8 + (i + 1) * sz]) for i in range((len(data) - 8) // sz)]


def join(pts, count=None):
    return header(len(pts) if count is None else count) + b"".join(bytes(p) for p in pts)


def tau_free(L, compressed=True):
    """The setup SRS's g1_powers through a file: params without tau."""
    return ts.CommitmentParams.deserialize_g1_powers(file_of(L, compressed), compressed)


# ---------------------------------------------------------------- g1_powers
@pytest.mark.parametrize("compressed", [True, False])
@pytest.mark.parametrize("L", [0, 2, 6])
def test_encode_equals_oracle(L, compressed):
    cp = params(L).commitment_params
    powers = cp.g1_powers
    want = oracle_file(powers, compressed)
    if L == 6:  # both signs of y occur, or the sign branch is untested
        flags = {po.g1_serialize(Q, True)[-1] & 0x80 for Q in powers}
        assert flags == {0, 0x80}
    assert cp.srs.serialize(compressed) == want
    assert cp.serialize_g1_powers(compressed) == want
    assert len(want) == N.load().tns_srs_serialized_size(len(powers), int(compressed))


@pytest.mark.parametrize("compressed", [True, False])
@pytest.mark.parametrize("L", [0, 2, 6, 8])
def test_decode_round_trip(L, compressed):
    want = srs_of(L).download()
    cp = tau_free(L, compressed)
    assert cp.tau is None and len(cp.srs) == len(want)
    assert np.array_equal(cp.srs.download(), want)


@pytest.mark.parametrize("compressed", [True, False])
def test_decode_one_point_and_empty(compressed):
    pts = split(file_of(2, compressed), compressed)
    one = ts.CommitmentParams.deserialize_g1_powers(join(pts[:1]), compressed)
    assert len(one.srs) == 1
    assert np.array_equal(one.srs.download(), srs_of(2).download(1))
    empty = ts.CommitmentParams.deserialize_g1_powers(header(0), compressed)
    assert len(empty.srs) == 0
    assert empty.srs.serialize(compressed) == header(0)


@pytest.mark.parametrize("compressed", [True, False])
def test_infinity_point(compressed):
    pts = split(file_of(2, compressed), compressed)
    pts[3] = bytearray(po.g1_serialize(None, compressed))
    got = ts.CommitmentParams.deserialize_g1_powers(join(pts), compressed).srs.download()
    want = srs_of(2).download().copy()
    want[3] = 0
    assert np.array_equal(got, want)
    # and the identity encodes back to the infinity flag
    assert ts.CommitmentParams.from_g1_limbs(want).srs.serialize(compressed) == join(pts)


def first_non_residue_x():
    x = 0
    while pow((x * x * x + 3) % P, (P - 1) // 2, P) == 1:  # Euler's criterion
        x += 1
    return x


def le32(v):
    return bytearray(v.to_bytes(32, "little"))


def bad_file(kind, k=700):
    """The 1025-point file with point k made invalid: (bytes, compressed)."""
    compressed = kind in ("x_is_p", "both_flags", "non_residue")
    pts = split(file_of(8, compressed), compressed)
    assert len(pts) == 1025
    if kind in ("x_is_p", "x_is_p_unc"):
        pts[k][:32] = le32(P)
    elif kind == "y_is_p_unc":
        pts[k][32:] = le32(P)
    elif kind == "both_flags":
        pts[k][-1] |= 0xC0
    elif kind == "non_residue":
        pts[k] = le32(first_non_residue_x())
    elif kind == "off_curve_unc":
        y = int.from_bytes(pts[k][32:], "little") & ((1 << 254) - 1)
        pts[k][32:] = le32((y + 1) % P)
    else:
        raise AssertionError(kind)
    return join(pts), compressed


@pytest.mark.parametrize("kind", ["x_is_p", "x_is_p_unc", "y_is_p_unc", "both_flags", "non_residue", "off_curve_unc"])
def test_bad_point_rejected_with_index(kind):
    data, compressed = bad_file(kind)
    with pytest.raises(ts.InvalidParameters) as e:
        ts.CommitmentParams.deserialize_g1_powers(data, compressed)
    assert "G1 point 700:" in str(e.value)
    # the reason is the host decoder's for the same bytes
    sz = 32 if compressed else 64
    with pytest.raises(ts.InvalidParameters) as h:
        ts.g1_deserialize(data[8 + 700 * sz:8 + 701 * sz], compressed)
    reason = str(h.value).split("] ", 1)[1]
    assert str(e.value).endswith("G1 point 700: " + reason)


def test_lowest_bad_index_is_named():
    pts = split(file_of(8, True), True)
    pts[700][-1] |= 0xC0
    pts[5][:32] = le32(P)
    with pytest.raises(ts.InvalidParameters) as e:
        ts.CommitmentParams.deserialize_g1_powers(join(pts), True)
    assert "G1 point 5:" in str(e.value) and "700" not in str(e.value)


@pytest.mark.parametrize("compressed", [True, False])
def test_length_must_match_header(compressed):
    data = file_of(8, compressed)
    pts = split(data, compressed)
    for bad in (data[:-1], data + b"\0", join(pts, count=len(pts) + 1), data[:7], b""):
        with pytest.raises(ts.InvalidParameters):
            ts.CommitmentParams.deserialize_g1_powers(bad, compressed)
    with pytest.raises(ts.InvalidParameters):  # a count whose size overflows
        ts.CommitmentParams.deserialize_g1_powers(header((1 << 64) - 1) + bytes(64), compressed)


def test_serialize_into_small_buffer():
    srs = srs_of(2)
    lib = N.load()
    need = lib.tns_srs_serialized_size(17, 1)
    ln = C.c_size_t()
    assert lib.tns_srs_serialize(srs.ctx.handle, srs.handle, 1, None, 0, C.byref(ln)) == 0  # sizing only
    assert ln.value == need
    buf = np.zeros(need - 1, dtype=np.uint8)
    ln = C.c_size_t()
    assert lib.tns_srs_serialize(srs.ctx.handle, srs.handle, 1, N.p8(buf), len(buf), C.byref(ln)) == 1
    assert ln.value == need and not buf.any()
    ln = C.c_size_t()
    assert lib.tns_srs_lagrange_serialize(srs.ctx.handle, srs.handle, 8, 1, N.p8(buf), 8, C.byref(ln)) == 1
    assert ln.value == lib.tns_srs_serialized_size(8, 1)


def test_loaded_srs_commits_like_the_setup_srs():
    rng = np.random.default_rng(17)
    coeffs = [int(x) for x in rng.integers(0, 1 << 62, 17)]
    coeffs = [c * c * c % po.R_MOD for c in coeffs]  # full-width scalars
    want = ts.KZGCommitment.commit(params(2).commitment_params, coeffs)
    for compressed in (True, False):
        assert ts.KZGCommitment.commit(tau_free(2, compressed), coeffs) == want


def test_loaded_srs_takes_tau():
    pp = params(2)
    cp = tau_free(2)
    cp.srs.set_tau(pp.commitment_params.tau)
    assert np.array_equal(cp.srs.lagrange_points(8), pp.commitment_params.srs.lagrange_points(8))


def test_sharded_srs_refused():
    pp, _ = ts.setup_params_shard(4, 0, 2)
    srs = pp.commitment_params.srs
    with pytest.raises(ts.InvalidParameters):
        srs.serialize()
    with pytest.raises(ts.InvalidParameters):
        srs.lagrange_serialize(8)
    with pytest.raises(ts.InvalidParameters):
        srs.lagrange_deserialize(srs_of(4).lagrange_serialize(8))


# ---------------------------------------------------------------- Lagrange basis
@pytest.mark.parametrize("compressed", [True, False])
@pytest.mark.parametrize("n", [1, 2, 8, 64])
def test_lagrange_encode_equals_oracle(n, compressed):
    srs = srs_of(4)
    assert srs.lagrange_serialize(n, compressed) == oracle_file(points_of(srs.lagrange_points(n)), compressed)


ATTACH = [(4, 1, True), (4, 2, True), (4, 8, True), (4, 64, True), (4, 64, False), (10, 1 << 12, True)]


@pytest.mark.parametrize("seed", SEEDS, ids=["seed", "os"])
@pytest.mark.parametrize("L,n,compressed", ATTACH)
def test_lagrange_attach(L, n, compressed, seed):
    want = srs_of(L).lagrange_points(n)
    data = srs_of(L).lagrange_serialize(n, compressed)
    cp = tau_free(L)
    with pytest.raises(ts.InvalidParameters):  # no tau, nothing attached yet
        cp.srs.lagrange_points(n)
    cp.srs.lagrange_deserialize(data, compressed, seed=seed)
    assert np.array_equal(cp.srs.lagrange_points(n), want)
    assert cp.srs.lagrange_serialize(n, compressed) == data
    cp.srs.lagrange_deserialize(data, compressed, seed=seed)  # cached already: checked again, kept
    assert np.array_equal(cp.srs.lagrange_points(n), want)


def test_proof_parity_on_attached_basis():
    """Twist::prove on a tau-less SRS loaded from a file with its basis attached from a file equals
    the setup SRS's proof (n = 2^12: the basis has its window table)."""
    L, n = 10, 1 << 12
    pp = params(L)
    cp = tau_free(L)
    cp.srs.lagrange_deserialize(srs_of(L).lagrange_serialize(n))
    pp_free = dataclasses.replace(pp, commitment_params=cp, _raw=None)
    addr, val, isw = ts.bench_trace(1 << 10, n)
    assert ts.Twist(pp_free).prove_soa(addr, val, isw) == ts.Twist(pp).prove_soa(addr, val, isw)


def other_tau_basis():
    tau2 = 1000  # small, and not a node of 0..63
    powers = [po.affine_mul(po.G1_GEN, pow(tau2, i, po.R_MOD)) for i in range(64)]
    return ts.CommitmentParams.from_g1_powers(powers, tau=tau2).srs.lagrange_serialize(64)


def bad_basis(kind):
    good = srs_of(4).lagrange_serialize(64)
    pts = split(good, True)
    if kind == "swapped":  # still sums to G: a partition-of-unity check alone would pass
        pts[3], pts[7] = pts[7], pts[3]
        assert pts[3] != pts[7]
    elif kind == "negated":
        pts[5][-1] ^= 0x80
    elif kind == "other_tau":
        return other_tau_basis()
    elif kind == "six_points":
        return join(pts[:6])
    else:
        raise AssertionError(kind)
    return join(pts)


@pytest.mark.parametrize("seed", SEEDS, ids=["seed", "os"])
@pytest.mark.parametrize("kind", ["swapped", "negated", "other_tau", "six_points"])
def test_lagrange_mismatch_rejected(kind, seed):
    cp = tau_free(4)
    with pytest.raises(ts.InvalidParameters) as e:
        cp.srs.lagrange_deserialize(bad_basis(kind), seed=seed)
    if kind != "six_points":
        assert "does not match g1_powers" in str(e.value)
    with pytest.raises(ts.InvalidParameters):  # nothing was cached
        cp.srs.lagrange_points(64)
    cp.srs.lagrange_deserialize(srs_of(4).lagrange_serialize(64), seed=seed)  # the SRS is still usable
    assert np.array_equal(cp.srs.lagrange_points(64), srs_of(4).lagrange_points(64))


@pytest.mark.parametrize("seed", SEEDS, ids=["seed", "os"])
def test_lagrange_count_above_held_powers(seed):
    pts = split(file_of(4, True), True)
    cp = ts.CommitmentParams.deserialize_g1_powers(join(pts[:33]))
    with pytest.raises(ts.InvalidParameters):
        cp.srs.lagrange_deserialize(srs_of(4).lagrange_serialize(64), seed=seed)
    with pytest.raises(ts.InvalidParameters):
        cp.srs.lagrange_points(64)
    cp.srs.lagrange_deserialize(srs_of(4).lagrange_serialize(32), seed=seed)
    assert np.array_equal(cp.srs.lagrange_points(32), srs_of(4).lagrange_points(32))
