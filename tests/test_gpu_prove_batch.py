"""A batch of Twist or Shout proofs over one SRS in one call (tns_twist_prove_batch,
tns_shout_prove_batch and their _device forms; csrc/prove_batch.hip, with the transcripts of
csrc/prove.hip zero_closure_transcript and the folds of csrc/zero_folds.hip fold_batch; DESIGN.md
2.13).  Every proof
of a batch must be byte for byte the proof the single prover returns for that row alone, pass the
verifier, and for small traces equal the oracle's.  The route each call took, and forced routes and
group splits, come from tests/device/provebatchprobe.hip, so a silent fall-back to the row loop
cannot pass."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from oracle import pyoracle as po

import batchref
import twist_and_shout as ts
from twist_and_shout import _native as N

pytestmark = pytest.mark.gpu
R = po.R_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "multilinear-map-cryptography_amd", "libtns_provebatchprobe.so")
ROWS, BATCHED = batchref.ROUTE_ROWS, batchref.ROUTE_BATCHED
INFO = ["route", "c0_route", "c0_groups", "c0_group_rows", "c1_route", "c1_groups", "c1_group_rows", "o0_route",
        "o0_groups", "o0_group_rows", "o1_route", "o1_groups", "o1_group_rows", "open_calls", "rows_per_point"]


@functools.lru_cache(maxsize=None)
def params(L):
    return ts.setup_params(L)


@functools.lru_cache(maxsize=None)
def oracle_params(L):
    return po.setup_params(L)


def level_for(n):
    """the smallest setup whose max_operations = 4 * 2^L covers n operations"""
    L = 2
    while (4 << L) < n:
        L += 1
    return L


def rand_limbs(rng, count, bits=253):
    limbs = rng.integers(0, 2**64, size=(count, 4), dtype=np.uint64, endpoint=False)
    for l in range(4):
        keep = min(max(bits - 64 * l, 0), 64)
        limbs[:, l] &= np.uint64((1 << keep) - 1)
    return limbs


def mont(limbs):
    limbs = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros_like(limbs)
    if len(limbs):
        N.load().tns_fr_from_canonical(N.p64(limbs), len(limbs), N.p64(out))
    return out


def ints(limbs):
    return [sum(int(x) << (64 * i) for i, x in enumerate(row)) for row in np.asarray(limbs).reshape(-1, 4)]


def value_rows(rng, B, n):
    """canonical (B, n, 4) limbs: rows of full-width, 30-bit, all-zero and constant values in turn"""
    out = np.zeros((B, n, 4), dtype=np.uint64)
    for b in range(B):
        k = b % 4
        if k == 0:
            out[b] = rand_limbs(rng, n)
        elif k == 1:
            out[b] = rand_limbs(rng, n, bits=30)
        elif k == 3:
            out[b] = rand_limbs(rng, 1)[0]
    return out


def twist_batch(n, B, seed):
    rng = np.random.default_rng(seed)
    addr = rng.integers(0, 1 << 20, size=(B, n), dtype=np.uint64)
    addr[(B - 1) // 2] = 0  # an all-zero address row: the identity commitment
    canon = value_rows(rng, B, n)
    isw = rng.integers(0, 2, size=(B, n), dtype=np.uint8)
    return addr, canon, mont(canon).reshape(B, n, 4), isw


def shout_batch(ne, nl, B, seed):
    rng = np.random.default_rng(seed)
    canon = value_rows(rng, B, ne)
    canon[0] = rand_limbs(rng, ne)
    idx = rng.integers(0, ne, size=(B, nl), dtype=np.uint64)
    idx[(B - 1) // 2] = 0
    return canon, mont(canon).reshape(B, ne, 4), idx


def bits_of(canon):
    """the bit length of the widest value"""
    return max(v.bit_length() for v in ints(canon))


def pick_rows(B, k=8):
    return sorted(set(range(B)) if B <= k else set(np.linspace(0, B - 1, k).astype(int).tolist()))


def raw_twist_batch(pp, addr, val_m, isw):
    B, n = addr.shape
    srs = pp.commitment_params.srs
    prs = (N.TnsProof * B)()
    st = N.load().tns_twist_prove_batch(srs.ctx.handle, srs.handle, C.byref(pp.raw()), N.p64(addr.reshape(-1)),
                                        N.p64(val_m.reshape(-1, 4)), N.p8(isw.reshape(-1)), n, B, prs)
    assert st == 0, (st, N.last_error())
    return prs


def raw_shout_batch(pp, ent_m, idx):
    B, ne = ent_m.shape[:2]
    srs = pp.commitment_params.srs
    prs = (N.TnsProof * B)()
    st = N.load().tns_shout_prove_batch(srs.ctx.handle, srs.handle, C.byref(pp.raw()), N.p64(ent_m.reshape(-1, 4)), ne,
                                        N.p64(idx.reshape(-1)), idx.shape[1], B, prs)
    assert st == 0, (st, N.last_error())
    return prs


def raw_shout_single(pp, ent_m, idx):
    srs = pp.commitment_params.srs
    pr = N.TnsProof()
    st = N.load().tns_shout_prove(srs.ctx.handle, srs.handle, C.byref(pp.raw()), N.p64(np.ascontiguousarray(ent_m)),
                                  len(ent_m), N.p64(np.ascontiguousarray(idx)), len(idx), C.byref(pr))
    assert st == 0, (st, N.last_error())
    return pr


@functools.lru_cache(maxsize=None)
def probe():
    lib = C.CDLL(PROBE)
    tail = [C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(N.TnsProof), C.POINTER(C.c_int64)]
    lib.provebatchprobe_twist.restype = C.c_int
    lib.provebatchprobe_twist.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(N.TnsParams), C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_uint64, C.c_uint64] + tail
    lib.provebatchprobe_shout.restype = C.c_int
    lib.provebatchprobe_shout.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(N.TnsParams), C.c_void_p, C.c_uint64,
                                          C.c_void_p, C.c_uint64, C.c_uint64] + tail
    assert lib.provebatchprobe_info_words() == len(INFO)
    return lib


def vp_(a):
    return np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)


def probe_twist(pp, addr, val_m, isw, force=-1, entries=0, ws=0, crossover=0):
    B, n = addr.shape
    srs = pp.commitment_params.srs
    prs = (N.TnsProof * B)()
    info = (C.c_int64 * len(INFO))()
    a, v, w = addr.reshape(-1).copy(), val_m.reshape(-1, 4).copy(), isw.reshape(-1).copy()
    st = probe().provebatchprobe_twist(srs.ctx.handle, srs.handle, C.byref(pp.raw()), vp_(a), vp_(v), vp_(w), n, B, 0,
                                       force, entries, ws, crossover, prs, info)
    assert st == 0, (st, N.last_error())
    return prs, dict(zip(INFO, list(info)))


def probe_shout(pp, ent_m, idx, force=-1, entries=0, ws=0, crossover=0):
    B, ne = ent_m.shape[:2]
    srs = pp.commitment_params.srs
    prs = (N.TnsProof * B)()
    info = (C.c_int64 * len(INFO))()
    e, i = ent_m.reshape(-1, 4).copy(), idx.reshape(-1).copy()
    st = probe().provebatchprobe_shout(srs.ctx.handle, srs.handle, C.byref(pp.raw()), vp_(e), ne, vp_(i), idx.shape[1], B,
                                       0, force, entries, ws, crossover, prs, info)
    assert st == 0, (st, N.last_error())
    return prs, dict(zip(INFO, list(info)))


def same(a, b):
    return all(bytes(x) == bytes(y) for x, y in zip(a, b)) and len(a) == len(b)


def check_twist_oracle(L, pr, addr, canon, isw):
    want = po.twist_prove(oracle_params(L), [(int(w), int(a), v) for w, a, v in zip(isw, addr, ints(canon))])
    got = ts.twist_proof_from_raw(pr)
    assert got.address_commitment.commitment == want["address_commitment"]
    assert got.value_commitment.commitment == want["value_commitment"]
    assert got.consistency_proof.round_polynomials == want["round_polynomials"]
    assert [q.proof for q in got.opening_proofs] == want["opening_proofs"]
    assert got.final_evaluations == want["final_evaluations"]
    if want["opening_point"] is not None:
        assert got.opening_point == want["opening_point"]
        assert list(got.sumcheck_challenges) == list(want["sumcheck_challenges"])


# ---------------------------------------------------------------- Twist
@pytest.mark.parametrize("batch", [1, 2, 3, 7, 65])
@pytest.mark.parametrize("n_ops", [1, 2, 3, 5, 64, 300, 1025])
def test_twist_batch_equals_single_prover(n_ops, batch):
    """N = 1 .. 2048; n_ops = 1 takes the rows route (no openings), 1025 pads 1023 zeros"""
    L = level_for(n_ops)
    pp, vp = params(L)
    addr, canon, val_m, isw = twist_batch(n_ops, batch, seed=100 * n_ops + batch)
    prs = raw_twist_batch(pp, addr, val_m, isw)
    for b in pick_rows(batch):
        one = ts.twist_prove_host_raw(pp, addr[b], val_m[b], isw[b])
        assert bytes(prs[b]) == bytes(one), (b, n_ops, batch)
    for b in range(batch):
        assert ts.Twist.verify(ts.twist_proof_from_raw(prs[b]), vp), b
    if n_ops <= 16:
        for b in pick_rows(batch, 2):
            check_twist_oracle(L, prs[b], addr[b], canon[b], isw[b])
    again, info = probe_twist(pp, addr, val_m, isw)  # the route the rule takes, reported
    N2 = max(1, 1 << (n_ops - 1).bit_length())
    assert info["route"] == (BATCHED if batch >= 2 and N2 >= 2 else ROWS), info
    if info["route"] == BATCHED:
        assert (info["open_calls"], info["rows_per_point"]) == (1, 2)
        assert info["c1_route"] == BATCHED and info["o0_route"] == BATCHED
        assert info["o0_groups"] * info["o0_group_rows"] >= 2 * batch
    assert same(again, prs)


@pytest.mark.parametrize("n_ops,batch", [(5, 7), (300, 7), (1025, 3)])
def test_twist_forced_routes_and_splits_give_the_same_bytes(n_ops, batch):
    L = level_for(n_ops)
    pp, _ = params(L)
    addr, canon, val_m, isw = twist_batch(n_ops, batch, seed=n_ops)
    whole, iw = probe_twist(pp, addr, val_m, isw)
    assert iw["route"] == BATCHED and (iw["c1_groups"], iw["c1_group_rows"]) == (1, batch)
    rows, ir = probe_twist(pp, addr, val_m, isw, force=ROWS)
    assert ir["route"] == ROWS and same(rows, whole)
    Nn = 1 << (n_ops - 1).bit_length()
    c, W = batchref.batch_window(Nn, 254)
    cap = batchref.ws_bytes(Nn, 2, c, W)  # two full-width rows a group
    split, isp = probe_twist(pp, addr, val_m, isw, ws=cap)
    want = batchref.plan_batch(Nn, batch, bits_of(canon), ws=cap, crossover=1 << 62)
    assert isp["route"] == BATCHED and (isp["c1_route"], isp["c1_group_rows"], isp["c1_groups"]) == (want[0], want[3], want[4])
    assert isp["c1_groups"] >= 2
    assert (isp["o0_groups"], isp["o0_group_rows"]) == (batch, 2) and same(split, whole)
    one, i1 = probe_twist(pp, addr[:1], val_m[:1], isw[:1], force=BATCHED)  # one proof, forced batched
    assert i1["route"] == BATCHED and bytes(one[0]) == bytes(whole[0])
    past, ip = probe_twist(pp, addr, val_m, isw, crossover=16)  # rows past the crossover: the single prover
    assert ip["route"] == ROWS and same(past, whole)


def test_twist_device_form_and_python_mirror():
    pp, vp = params(7)
    n, B = 300, 7
    addr, canon, val_m, isw = twist_batch(n, B, seed=5)
    ctx = pp.commitment_params.srs.ctx
    da, dv, dw = ts.DeviceBuffer(ctx, addr), ts.DeviceBuffer(ctx, val_m), ts.DeviceBuffer(ctx, isw)
    dev = ts.twist_prove_batch_resident(pp, da, dv, dw, n, B)
    host = raw_twist_batch(pp, addr, val_m, isw)
    assert same(list(dev)[:B], list(host)[:B])
    tm = (C.c_double * 6)()
    assert N.load().tns_last_prove_timing(ctx.handle, tm) == 0 and tm[5] > 0  # the whole call in slot 5
    assert tm[0] == tm[1] == 0 and 0 < tm[2] + tm[3] + tm[4] <= tm[5]
    full = 256  # a resident batch of full-length rows is read in place
    a2, _, v2, w2 = twist_batch(full, 3, seed=6)
    dev2 = ts.twist_prove_batch_resident(pp, ts.DeviceBuffer(ctx, a2), ts.DeviceBuffer(ctx, v2), ts.DeviceBuffer(ctx, w2),
                                         full, 3)
    assert same(list(dev2)[:3], list(raw_twist_batch(pp, a2, v2, w2))[:3])
    # the mirror: proof objects, traces
    proofs = ts.Twist(pp).prove_soa_batch(addr, val_m, isw)
    assert len(proofs) == B and all(ts.Twist.verify(p, vp) for p in proofs)
    assert proofs[3].opening_point == ts.twist_proof_from_raw(host[3]).opening_point
    traces = []
    for k in range(3):
        t = ts.MemoryTrace(8)
        t.write(k, 40 + k)
        t.write(1, 100)
        t.read(k)
        t.read(1)
        traces.append(t)
    got = ts.Twist(pp).prove_batch(traces)
    want = [ts.Twist(pp).prove(t) for t in traces]
    assert [(g.address_commitment.commitment, g.value_commitment.commitment, [q.proof for q in g.opening_proofs],
             g.final_evaluations, g.opening_point) for g in got] == \
           [(g.address_commitment.commitment, g.value_commitment.commitment, [q.proof for q in g.opening_proofs],
             g.final_evaluations, g.opening_point) for g in want]
    traces[1].read(0)
    with pytest.raises(ts.InvalidParameters):
        ts.Twist(pp).prove_batch(traces)
    assert ts.Twist(pp).prove_batch([]) == []


# ---------------------------------------------------------------- Shout
@pytest.mark.parametrize("batch", [2, 7])
@pytest.mark.parametrize("ne,nl", [(4, 4), (5, 300), (300, 5), (1025, 64)])
def test_shout_batch_equals_single_prover(ne, nl, batch):
    """T == M (one opening call, two rows a point) and T != M (a call each)"""
    L = level_for(max(ne, nl))
    pp, vp = params(L)
    canon, ent_m, idx = shout_batch(ne, nl, batch, seed=ne + nl + batch)
    prs = raw_shout_batch(pp, ent_m, idx)
    for b in range(batch):
        assert bytes(prs[b]) == bytes(raw_shout_single(pp, ent_m[b], idx[b])), (b, ne, nl)
        assert ts.Shout.verify(ts.shout_proof_from_raw(prs[b]), vp), b
    if max(ne, nl) <= 16:
        for b in pick_rows(batch, 2):
            want = po.shout_prove(oracle_params(L), ints(canon[b]), [int(i) for i in idx[b]])
            got = ts.shout_proof_from_raw(prs[b])
            assert got.table_commitment.commitment == want["table_commitment"]
            assert got.index_commitment.commitment == want["index_commitment"]
            assert [q.proof for q in got.opening_proofs] == want["opening_proofs"]
            assert got.final_evaluations == want["final_evaluations"] and got.opening_point == want["opening_point"]
    T, M = 1 << (ne - 1).bit_length(), 1 << (nl - 1).bit_length()
    again, info = probe_shout(pp, ent_m, idx)
    assert info["route"] == BATCHED and same(again, prs)
    assert (info["open_calls"], info["rows_per_point"]) == ((1, 2) if T == M else (2, 1))
    assert info["c0_route"] == BATCHED and info["o0_route"] == BATCHED and (T == M or info["o1_route"] == BATCHED)
    rows, ir = probe_shout(pp, ent_m, idx, force=ROWS)
    assert ir["route"] == ROWS and same(rows, prs)
    (ct, Wt), (cm, Wm) = batchref.batch_window(T, 254), batchref.batch_window(M, 254)
    cap = 2 * max(Wt * T, Wm * M) + 1  # two rows of the longer kind a group
    split, isp = probe_shout(pp, ent_m, idx, entries=cap)
    want = batchref.plan_batch(T, batch, bits_of(canon), entries=cap, crossover=1 << 62)
    assert isp["route"] == BATCHED and (isp["c0_route"], isp["c0_group_rows"], isp["c0_groups"]) == (want[0], want[3], want[4])
    wo = batchref.plan_batch(T, 2 * batch if T == M else batch, 254, entries=cap, crossover=1 << 62)
    assert (isp["o0_group_rows"], isp["o0_groups"]) == (wo[3], wo[4]) and same(split, prs)
    assert T != M or isp["o0_groups"] == batch  # 2 batch rows, two a group


def test_shout_device_form_and_python_mirror():
    pp, vp = params(7)
    ne, nl, B = 5, 300, 7
    canon, ent_m, idx = shout_batch(ne, nl, B, seed=9)
    ctx = pp.commitment_params.srs.ctx
    dev = ts.shout_prove_batch_resident(pp, ts.DeviceBuffer(ctx, ent_m), ne, ts.DeviceBuffer(ctx, idx), nl, B)
    host = raw_shout_batch(pp, ent_m, idx)
    assert same(list(dev)[:B], list(host)[:B])
    proofs = ts.Shout(pp).prove_arrays_batch(ent_m, idx)
    assert len(proofs) == B and all(ts.Shout.verify(p, vp) for p in proofs)
    tables = []
    for k in range(3):
        t = ts.LookupTable([i * i + k for i in range(8)])
        for i in (3, k, 7, 0):
            t.lookup(i)
        tables.append(t)
    got = ts.Shout(pp).prove_batch(tables)
    want = [ts.Shout(pp).prove(t) for t in tables]
    key = lambda g: (g.table_commitment.commitment, g.index_commitment.commitment,
                     [q.proof for q in g.opening_proofs], g.final_evaluations, g.opening_point)
    assert [key(g) for g in got] == [key(g) for g in want]
    tables[2].lookup(1)
    with pytest.raises(ts.InvalidParameters):
        ts.Shout(pp).prove_batch(tables)


# ---------------------------------------------------------------- errors
def test_errors_match_the_single_prover_and_leave_nothing_running():
    pp, vp = params(2)  # max_operations = 16
    ne, nl, B = 8, 8, 5
    canon, ent_m, idx = shout_batch(ne, nl, B, seed=3)
    idx[B - 1, nl - 1] = ne  # out of range in the last row only
    with pytest.raises(ts.InvalidParameters) as single:
        ts.Shout(pp).prove_arrays(ent_m[B - 1], idx[B - 1])
    with pytest.raises(ts.InvalidParameters) as batch:
        ts.Shout(pp).prove_arrays_batch(ent_m, idx)
    assert str(batch.value) == str(single.value) and "Lookup index out of bounds" in str(batch.value)
    idx[B - 1, nl - 1] = 0
    assert all(ts.Shout.verify(p, vp) for p in ts.Shout(pp).prove_arrays_batch(ent_m, idx))  # the context still works
    addr, _, val_m, isw = twist_batch(17, 2, seed=4)
    with pytest.raises(ts.InvalidParameters) as single:
        ts.Twist(pp).prove_soa(addr[0], val_m[0], isw[0])
    with pytest.raises(ts.InvalidParameters) as batch:
        ts.Twist(pp).prove_soa_batch(addr, val_m, isw)
    assert str(batch.value) == str(single.value) and "Too many operations" in str(batch.value)
    with pytest.raises(ts.InvalidParameters) as e:
        ts.Shout(pp).prove_arrays_batch(ent_m[:, :4], np.zeros((B, 17), dtype=np.uint64))
    assert "Too many lookup operations" in str(e.value)
    addr, _, val_m, isw = twist_batch(16, 3, seed=5)
    good = ts.Twist(pp).prove_soa_batch(addr, val_m, isw)
    assert all(ts.Twist.verify(p, vp) for p in good)
    # the argument checks: NULL arrays, a shard, batch * N above 2^32, batch == 0
    lib = N.load()
    srs = pp.commitment_params.srs
    prs = (N.TnsProof * 3)()
    args = (N.p64(addr.reshape(-1)), N.p64(val_m.reshape(-1, 4)), N.p8(isw.reshape(-1)))
    raw = C.byref(pp.raw())
    assert lib.tns_twist_prove_batch(srs.ctx.handle, srs.handle, raw, None, args[1], args[2], 16, 3, prs) == 1
    assert lib.tns_twist_prove_batch(srs.ctx.handle, srs.handle, raw, *args, 16, 3, None) == 1
    assert lib.tns_twist_prove_batch(srs.ctx.handle, srs.handle, None, *args, 16, 3, prs) == 1
    assert lib.tns_twist_prove_batch(srs.ctx.handle, srs.handle, raw, *args, 16, 0, None) == 0
    assert lib.tns_twist_prove_batch(srs.ctx.handle, srs.handle, raw, *args, 16, 1 << 40, prs) == 1
    assert "2^32" in N.last_error()
    shard_pp, _ = ts.setup_params_shard(2, 0, 2)
    assert lib.tns_twist_prove_batch(srs.ctx.handle, shard_pp.commitment_params.srs.handle, raw, *args, 16, 3, prs) == 1
    assert "shard" in N.last_error()
    assert lib.tns_shout_prove_batch(srs.ctx.handle, shard_pp.commitment_params.srs.handle, raw, args[1], 8, args[0], 8,
                                     3, prs) == 1
    assert same(list(raw_twist_batch(pp, addr, val_m, isw))[:3], [ts.twist_prove_host_raw(pp, addr[b], val_m[b], isw[b])
                                                                  for b in range(3)])


# ---------------------------------------------------------------- one larger case
def test_twist_batch_of_64_traces_of_4096_operations():
    pp, vp = params(10)
    n, B = 1 << 12, 64
    addr, canon, val_m, isw = twist_batch(n, B, seed=77)
    prs, info = probe_twist(pp, addr, val_m, isw)
    assert info["route"] == BATCHED and (info["open_calls"], info["rows_per_point"]) == (1, 2)
    for b in (0, 31, 63):
        assert bytes(prs[b]) == bytes(ts.twist_prove_host_raw(pp, addr[b], val_m[b], isw[b])), b
    proofs = [ts.twist_proof_from_raw(prs[b]) for b in range(B)]
    cms, zs, vals, pis = [], [], [], []
    for p in proofs:
        cms += [p.address_commitment, p.value_commitment]
        zs += [p.opening_point] * 2
        vals += list(p.final_evaluations)
        pis += list(p.opening_proofs)
    assert len(pis) == 128
    assert ts.KZGCommitment.verify_many(vp.commitment_vk, cms, zs, vals, pis, seed=bytes(range(32)))
