"""tests/accref.py on its own, without a GPU: (a) the reference equals the MSM contract on the bucket
orders of real scalars (sortref.entries): its result is sum_i c_i a_i; (b) the reference's route --
chunk heads and tails, flags, level sums, peel and climb -- gives the buckets and flags of its
contract on every case test_gpu_accumulate.py runs; (c) csrc/msm_plan.hpp's tail_geom and
fix_level_sizes (tests/cpp/tail_geom_vectors.cpp, plain g++) equal accref's restatement, and which
values of L0, L1, CH, tree and sum_sets' 8-way passes occur over every legal window c = 4..23;
(d) the coverage the GPU cases are meant to have is a condition computed here, so an edit of the
case list that loses some of it fails without a device."""
import collections
import os
import shutil
import subprocess

import numpy as np
import pytest

import accref as A
import sortref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multilinear-map-cryptography_amd", "csrc")
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")


# ---------------------------------------------------------------- (a)
CONTRACT_PLANS = ["pw_c4_W1_n300", "pw_c6_W3_n300", "pw_c7_W37_n1000", "pw_c12_W22_n5000", "sh_c17_W4_n5000",
                  "sh_c20_W13_n3000"]


@pytest.mark.parametrize("name", CONTRACT_PLANS)
def test_reference_equals_the_msm_contract(name):
    """real scalars c_i through sortref's digits and bucket order, points a_i G (the shared layout over
    the window table 2^(c w) a_i at w stride + i): buckets, set sums and Horner give sum_i c_i a_i"""
    plan = next(p for p in sortref.PLANS if p.name == name)
    rng = np.random.default_rng(len(name))
    cs = sortref.rand_exact(rng, plan.bits, plan.n)
    cs[0], cs[1] = 0, cs[2]  # a zero scalar and a repeated one
    a = sortref.rand_exact(rng, 254, plan.n)
    a[3], a[4] = 0, A.R - a[5]  # the identity among the points, and a point with its negative
    ent = sortref.entries(sortref.to_limbs(cs), plan.c, plan.W, plan.shared, plan.stride)
    nb = 1 << plan.bucket_bits
    lengths = np.bincount((ent >> np.uint64(32)).astype(np.int64), minlength=nb)
    vals = (ent & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    if plan.shared:
        table = np.zeros(plan.W * plan.stride, dtype=object)
        for w in range(plan.W):
            table[w * plan.stride:w * plan.stride + plan.n] = [x << (plan.c * w) for x in a]
    else:
        table = np.array(a, dtype=object)
    Wr, half = (1, nb) if plan.shared else (plan.W, 1 << (plan.c - 1))
    assert half == 1 << (plan.c - 1)
    want = sum(c * x for c, x in zip(cs, a)) % A.R
    for k in (16, 37):
        o = A.Order(lengths[:Wr * half], vals, k, scalars=table)
        sums = o.set_sums(Wr, half)
        assert A.result_of(sums, plan.c, plan.shared) == want, (name, k)
        sim, flags = A.simulate(o)
        assert sim == o.buckets() and flags == o.flags(), (name, k)


# ---------------------------------------------------------------- (b)
def test_the_route_equals_the_contract_on_every_case():
    """heads, tails, level sums and the peel / climb sequence add up to every bucket, every level sum a
    run reads was formed (flag bit 1 set whenever one is needed), and the flags counted chunk by chunk
    are the flags stated run by run"""
    checked = 0
    for case in A.fixup_cases():
        for o in case.orders:
            sim, flags = A.simulate(o)
            assert flags == o.flags(), case
            assert sim == o.buckets(), case
            checked += 1
    assert checked >= 370


def test_flag_definitions_on_literal_orders():
    k = 16
    one = lambda ln, **kw: A.Order(ln, A.random_vals(np.random.default_rng(1), sum(ln)), k, **kw)  # noqa: E731
    assert one([k, k, 0, k]).flags() == 0               # runs end on chunk edges
    assert one([k - 1, 2, k - 1]).flags() == 1          # a run of two entries over an edge
    assert one([8 * k]).flags() == 3                    # one bucket over exactly 8 aligned chunks
    assert one([1, 8 * k]).flags() == 1                 # 8 k entries in one bucket, no aligned group
    assert one([8 * k, 7 * k + 1]).flags() == 3         # the first group lies in bucket 0
    assert one([k, 7 * k + 1]).flags() == 1             # the group spans two buckets
    assert one([7 * k + 1], nchunks=8).flags() == 3     # the eighth chunk holds one entry
    assert one([7 * k], nchunks=12).flags() == 1        # the eighth chunk lies past valid


def test_peel_and_climb_literal():
    assert A.fix_items(0, 1, 3) == []
    assert A.fix_items(0, 5, 3) == [(0, i) for i in range(1, 5)]
    # lo = 8 aligned, hi = 24 aligned, 16 chunks: climbs at once
    assert A.fix_items(7, 24, 1) == [(1, 1), (1, 2)]
    assert A.fix_items(7, 24, 0) == [(0, i) for i in range(8, 24)]  # no level to climb to
    # lo = 6 peels up to 8, then hi = 27 peels down to 24
    assert A.fix_items(5, 27, 2) == [(0, 6), (0, 7), (0, 26), (0, 25), (0, 24), (1, 1), (1, 2)]
    # 15 aligned chunks are not enough
    assert A.fix_items(7, 23, 2) == [(0, i) for i in range(8, 23)]


# ---------------------------------------------------------------- (c)
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("tailgeom") / "tail_geom_vectors"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "tail_geom_vectors.cpp"), "-o", str(out)])
    return out


def run(exe, tmp_path, lines):
    path = tmp_path / "cases.txt"
    path.write_text("".join(" ".join(str(x) for x in l) + "\n" for l in lines))
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    rows = [[int(w) for w in r.split()] for r in out.stdout.splitlines()]
    assert len(rows) == len(lines)
    return rows


LEGAL_C = range(4, 24)  # plan_msm: best_window takes c >= 4, the one-window plans reach 23


@needs_gxx
def test_constants(exe, tmp_path):
    assert run(exe, tmp_path, [["consts"]])[0] == [16, A.FIX_FAN, A.FIX_LEVELS, A.FIX_WAVE_SPAN]


@needs_gxx
def test_tail_geometry_equals_the_restatement(exe, tmp_path):
    rows = run(exe, tmp_path, [["tail", 1 << (c - 1)] for c in LEGAL_C])
    for c, row in zip(LEGAL_C, rows):
        t = A.tail_geom(1 << (c - 1))
        assert row == [t[f] for f in A.TAIL_FIELDS] + [A.sum_passes(t["sum_n"])], c
        # what the kernels rely on
        half = 1 << (c - 1)
        assert t["L0"] * t["g1"] == half and t["g"] * (t["L1"] or 1) == t["g1"] and t["g"] >= 2
        assert 1 << t["nbits"] == t["g"] and 2 * t["CH"] * t["nch"] == t["g"] and t["CH"] >= 1
        assert t["weight"] * t["g"] == half and 1 << t["lg0"] == t["L0"]


# the reduction's regimes (L0, L1, CH, tree, 8-way passes) -> the windows that take them: DESIGN 2.16
REGIMES = {
    (4, 0, 1, 0, 0): [4], (4, 0, 2, 0, 0): [5], (4, 0, 4, 0, 0): [6],
    (4, 0, 8, 0, 0): [7, 8, 9, 10, 11, 12],
    (4, 0, 8, 1, 0): [13, 14, 15],
    (4, 4, 8, 1, 0): [16, 17, 18, 19, 20],
    (16, 4, 8, 1, 0): [21, 22, 23],
}


def test_reachable_regimes():
    """Which branches of the tail occur for a legal plan.  Two never do: CH = 16 (sets of more than
    2^19 buckets always leave g1 >= 2^13 first-level groups, hence L1 = 4 and CH = 8) and the 8-way
    k_sum_chunks passes of sum_sets (they need more than 128 parts a spec; the most is 64, at c = 23).
    Both stay in the code."""
    got = collections.defaultdict(list)
    for c in LEGAL_C:
        got[A.regime(1 << (c - 1))].append(c)
    assert dict(got) == REGIMES
    geoms = [A.tail_geom(1 << (c - 1)) for c in LEGAL_C]
    assert {t["L0"] for t in geoms} == {4, 16}
    assert {t["L1"] for t in geoms} == {0, 4}
    assert {t["CH"] for t in geoms} == {1, 2, 4, 8}        # never 16
    assert {t["tree"] for t in geoms} == {0, 1}
    assert max(t["sum_n"] for t in geoms) == 64            # sum_sets splits only above 128
    assert {A.sum_passes(t["sum_n"]) for t in geoms} == {0}


@needs_gxx
def test_fix_level_sizes_equal_the_restatement(exe, tmp_path):
    ns = [1, 7, 8, 15, 16, 17, 127, 128, 129]
    for l in range(1, 10):
        ns += [2 * 8 ** l - 1, 2 * 8 ** l, 2 * 8 ** l + 1, 3 * 8 ** l]
    rows = run(exe, tmp_path, [["fix", n] for n in ns])
    for n, row in zip(ns, rows):
        want = A.fix_level_sizes(n)
        assert row == [len(want), sum(want)] + want, n
    assert A.fix_level_sizes(15) == [] and A.fix_level_sizes(16) == [2] and A.fix_level_sizes(128) == [16, 2]
    assert len(A.fix_level_sizes(2 * 8 ** 8)) == 8 == len(A.fix_level_sizes(2 * 8 ** 9))  # FIX_LEVELS caps it


def test_msm_plan_header_still_has_no_hip_include():
    with open(os.path.join(CSRC, "msm_plan.hpp")) as f:
        incs = [l.split()[1] for l in f if l.startswith("#include")]
    assert incs and all(i in ("<algorithm>", "<cstddef>", "<cstdint>") for i in incs), incs


# ---------------------------------------------------------------- (d)
@pytest.fixture(scope="module")
def geometry():
    """(case, run geometry) of every run across chunks of every fix-up case"""
    return [(case, g) for case in A.fixup_cases() for o in case.orders for g in A.run_geometry(o)]


def test_every_peel_pair_occurs_on_the_thread_path(geometry):
    for depth in (1, 2):
        pairs = collections.Counter()
        for case in A.thread_cases(depth):
            g = max(A.run_geometry(case.orders[0]), key=lambda g: g["span"])
            assert g["path"] == "thread" and max(g["levels"]) == depth, (case, g)
            assert (20 <= g["span"] <= 40) if depth == 1 else (130 <= g["span"] <= 200), (case, g)
            pairs[g["pair"]] += 1
        assert len(pairs) == 64 and set(pairs.values()) == {2}, depth  # each pair: same-point and random


def test_both_sides_of_the_wave_threshold_occur(geometry):
    spans = {g["span"]: g["path"] for _, g in geometry}
    assert spans[A.FIX_WAVE_SPAN] == "thread" and spans[A.FIX_WAVE_SPAN + 1] == "wave"
    for case in A.threshold_cases():
        g = max(A.run_geometry(case.orders[0]), key=lambda g: g["span"])
        assert g["span"] == (512 if "span512" in case.name else 513), case
        assert g["path"] == ("thread" if g["span"] == 512 else "wave"), case


def test_levels_one_to_five_are_read(geometry):
    wave = [g for _, g in geometry if g["path"] == "wave"]
    assert {l for g in wave for l in g["levels"]} >= {1, 2, 3, 4, 5}
    for level in (3, 4, 5):
        for case in A.deep_cases(level):
            g = max(A.run_geometry(case.orders[0]), key=lambda g: g["span"])
            assert g["path"] == "wave" and max(g["levels"]) == level, (case, g)
    # the wave's item loop: runs of at most 64 items (one round) and of more (a second round)
    assert min(g["items"] for g in wave) <= 64 < max(g["items"] for g in wave)
    # unaligned starts of the deep runs, in chunks mod 512
    starts = {int(c.orders[0].bstart[3 if "tf0_" not in c.name else 0]) // 16 % 512 for l in (3, 4, 5) for c in A.deep_cases(l)}
    assert starts >= {0, 1, 7, 63, 511}


def test_wave_edges():
    """two heavy runs in one wave of 64 buckets; a heavy run in a wave that ends at nb"""
    cases = {c.name: c for c in A.wave_edge_cases()}
    for v in ("same", "rand"):
        o = cases["two_heavy_in_a_wave_" + v].orders[0]
        heavy = [bk for bk, tf, tl in o.runs() if A.on_wave_path(tf, tl)]
        assert len(heavy) == 2 and heavy[0] // 64 == heavy[1] // 64
        for bk in (64, 71):
            o = cases["heavy_b%d_of_72_%s" % (bk, v)].orders[0]
            assert o.nb == 72 and [b for b, tf, tl in o.runs() if A.on_wave_path(tf, tl)] == [bk]


def test_lattice_edges():
    """what the chunk-edge lattice is meant to hold, per acc_k"""
    for k in A.ACC_KS:
        cases = A.lattice_cases(k)
        assert {c.orders[0].acc_k for c in cases} == {k}
        kinds = collections.Counter()
        for c in cases:
            o = c.orders[0]
            b = o.bstart.astype(np.int64)
            for bk, tf, tl in o.runs():
                s, e = int(b[bk]), int(b[bk + 1])
                kinds["ends on an edge"] += e % k == 0 and e < o.valid
                kinds["starts on an edge"] += s % k == 0 and s > 0
                kinds["contains a chunk"] += tl - tf >= 2
                kinds["straddles"] += tl - tf == 1
                kinds["empty before"] += bk > 0 and o.lengths[bk - 1] == 0
                kinds["empty after"] += bk + 1 < o.nb and o.lengths[bk + 1] == 0
            kinds["bucket 0 empty"] += o.lengths[0] == 0
            kinds["last bucket empty"] += o.lengths[-1] == 0
            kinds["valid a multiple"] += o.valid % k == 0
            kinds["valid one more"] += o.valid % k == 1
            kinds["chunks past valid"] += o.nchunks > -(-o.valid // k)
            kinds["keys"] += o.keys is not None
            kinds["no keys"] += o.keys is None
        assert all(kinds[n] > 0 for n in ("ends on an edge", "starts on an edge", "contains a chunk", "straddles",
                                           "empty before", "empty after", "bucket 0 empty", "last bucket empty",
                                           "valid a multiple", "valid one more", "chunks past valid", "keys", "no keys")), (k, kinds)
    assert any(c.orders[0].valid == 1 for c in A.lattice_cases(16))


def test_flag_combinations_occur():
    flags = collections.Counter(o.flags() for c in A.fixup_cases() for o in c.orders)
    assert set(flags) == {0, 1, 3}  # (bit 1 implies bit 0: a group inside one bucket crosses chunks)
    for c in A.no_crossing_cases():
        assert c.orders[0].flags() == 0 and (c.orders[0].lengths == 0).sum() > 40
        assert (c.prefill.orders[0].lengths > 0).all() and c.prefill.nb == c.nb
    two = {c.name: [o.flags() for o in c.orders] for c in A.two_set_cases()}
    assert two["two_crossing_light"] == [3, 0] and two["two_light_heavy"] == [0, 3]
    for c in A.two_set_cases():  # different level counts in one tail
        n = [len(A.fix_level_sizes(o.nchunks)) for o in c.orders]
        assert n[0] != n[1], (c, n)


def test_every_reachable_regime_is_swept():
    """every reduction regime a plan of at most 2^20 buckets a set takes is run, in both layouts
    where both can reach it"""
    swept = {A.regime(1 << (c - 1)) for c, W, shared in A.SWEEP_SHAPES}
    assert swept == {r for r, cs in REGIMES.items() if min(cs) <= 21}
    assert {c for c, W, shared in A.SWEEP_SHAPES if shared} == set(range(4, 22))
    assert {(W, c) for c, W, shared in A.SWEEP_SHAPES if not shared} == {(W, c) for W in (2, 3, 13) for c in (4, 8, 12, 16)}
    for c, W, shared in A.SWEEP_SHAPES:
        t = A.tail_geom(1 << (c - 1))
        pos = set(A.sweep_positions(1 << (c - 1)))
        half, w = 1 << (c - 1), t["weight"]
        assert pos >= {0, 1, t["L0"] - 1, t["L0"], half // 2 - 1, half // 2, half - 1} | {w - 1, w} and (w + 1 in pos or w + 1 >= half)
        assert {p // w for p in pos} >= {1 << b for b in range(t["nbits"])} | {t["g"] - 1}
