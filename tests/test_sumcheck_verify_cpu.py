"""tns_sumcheck_verify (SumCheck::verify, src/sumcheck.rs:113-153; host code, no GPU) through
SumCheck.verify, against tests/mleref.py's restatement on the C oracle's proofs of the compositions
of tests/test_gpu_sumcheck_batch.py at nv 0, 1, 2, 5: honest proofs; a coefficient changed in
round 0, a middle round and the last round; a changed final evaluation; a wrong claimed sum; a
wrong number of rounds.  The transcript's state after every call is pinned by a challenge drawn
from it afterwards.  Every comparison is exact."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from oracle import coracle as co
from oracle import pyoracle as po

import twist_and_shout as ts
from twist_and_shout import _native as N

import mleref as ref

R = po.R_MOD
COMPOSITIONS = {  # tests/test_gpu_sumcheck_batch.py's table
    "twist_like": [(1, [0, 1]), (R - 1, [2, 2, 1]), (2, [2])],
    "dense4": [(17, [0, 1, 2]), (R - 3, [3, 3]), (5, [1, 2, 3]), (R - 1, [0]), (2, [2, 3]), (7, [])],
    "single": [(3, [0, 0, 0]), (R - 2, [0]), (5, [])],
    "pair2": [(1, [0, 1]), (4, [1, 1])],
}
LABEL, ELEMENT = b"instance", 1000003
NVS = [0, 1, 2, 5]


def h(x):
    return int(x, 16)


@functools.lru_cache(maxsize=None)
def case(name, nv):
    """(claim, rounds, final, challenges) of the oracle's proof on the prefixed transcript"""
    terms = COMPOSITIONS[name]
    k = 1 + max(max(ix) for _, ix in terms if ix)
    rng = random.Random(97 * nv + k)
    tables = [[rng.randrange(R) for _ in range(1 << nv)] for _ in range(k)]
    claim = sum(ref.composition(terms, [t[x] for t in tables]) for x in range(1 << nv)) % R
    st, rounds, fin, chal = co.sumcheck_prove([co.fr_array(t) for t in tables], nv, claim, terms,
                                              prefix=LABEL + ELEMENT.to_bytes(32, "little"))
    assert st == 0
    return claim, [co.fr_ints(r) for r in rounds], co.fr_ints(fin)[0], co.fr_ints(chal) if nv else []


def transcripts():
    """the product's transcript and the oracle's, in the same state"""
    a, b = ts.Transcript(bytes(32)), po.Transcript(bytes(32))
    a.append_field_element(LABEL, ELEMENT)
    b.append_field_element(LABEL, ELEMENT)
    return a, b


def both(nv, claim, rounds, final):
    """SumCheck.verify and the restatement on equal transcripts: the product's answer, checked
    against the restatement's, with a challenge drawn from both transcripts afterwards"""
    a, b = transcripts()
    got = ts.SumCheck(nv, claim).verify(ts.SumCheckProof(rounds, final), a)
    want = ref.sumcheck_verify(claim, rounds, final, b)
    assert got == want
    assert a.challenge_field_element(b"after") == b.challenge_field_element(b"after")
    return got


@pytest.mark.parametrize("nv", NVS)
@pytest.mark.parametrize("name", sorted(COMPOSITIONS))
def test_honest_proofs_verify(name, nv):
    claim, rounds, final, chal = case(name, nv)
    assert both(nv, claim, rounds, final) == (True, chal)


@pytest.mark.parametrize("nv", [1, 2, 5])
@pytest.mark.parametrize("name", sorted(COMPOSITIONS))
def test_a_changed_coefficient_stops_the_replay_at_its_round(name, nv):
    claim, rounds, final, chal = case(name, nv)
    for r in sorted({0, nv // 2, nv - 1}):
        for coef in (0, 3):
            bad = [list(g) for g in rounds]
            bad[r][coef] = (bad[r][coef] + 1) % R  # g(0) + g(1) moves by 2 (c0) or 1 (c3)
            ok, got = both(nv, claim, bad, final)
            assert ok is False and got == chal[:r]


@pytest.mark.parametrize("nv", NVS)
@pytest.mark.parametrize("name", sorted(COMPOSITIONS))
def test_a_changed_final_fails_with_every_challenge(name, nv):
    claim, rounds, final, chal = case(name, nv)
    assert both(nv, claim, rounds, (final + 1) % R) == (False, chal)


@pytest.mark.parametrize("nv", NVS)
@pytest.mark.parametrize("name", sorted(COMPOSITIONS))
def test_a_wrong_claimed_sum_fails_round_zero(name, nv):
    claim, rounds, final, chal = case(name, nv)
    # (nv == 0: no round; the claim is compared with the final evaluation)
    assert both(nv, (claim + 1) % R, rounds, final) == (False, [])


@pytest.mark.parametrize("nv", [1, 2, 5])
def test_a_wrong_number_of_rounds_is_an_error_and_leaves_the_transcript(nv):
    claim, rounds, final, chal = case("twist_like", nv)
    for shape in (rounds[:-1], rounds + [rounds[-1]]):
        a, b = transcripts()
        with pytest.raises(ts.SumCheckError, match="Proof has wrong number of rounds"):
            ts.SumCheck(nv, claim).verify(ts.SumCheckProof(shape, final), a)
        assert a.challenge_field_element(b"after") == b.challenge_field_element(b"after")
    # the C entry point itself: the status, the message, nothing written
    a, b = transcripts()
    rd = co.fr_array([c for g in rounds for c in g])
    ch = np.zeros((nv + 1, 4), dtype=np.uint64)
    nch, ok = C.c_size_t(77), C.c_int(77)
    st = N.load().tns_sumcheck_verify(nv + 1, N.p64(co.fr_array([claim])[0]), N.p64(rd), nv, N.p64(co.fr_array([final])[0]),
                                      a._h, N.p64(ch), C.byref(nch), C.byref(ok))
    assert st == 6 and "Proof has wrong number of rounds" in N.last_error()
    assert (nch.value, ok.value) == (77, 77) and not ch.any()
    assert a.challenge_field_element(b"after") == b.challenge_field_element(b"after")


def test_c_entry_point_reports_the_failing_round_index():
    nv = 5
    claim, rounds, final, chal = case("dense4", nv)
    bad = [list(g) for g in rounds]
    bad[3][1] = (bad[3][1] + 5) % R
    a, _ = transcripts()
    ch = np.zeros((nv, 4), dtype=np.uint64)
    nch, ok = C.c_size_t(77), C.c_int(77)
    st = N.load().tns_sumcheck_verify(nv, N.p64(co.fr_array([claim])[0]), N.p64(co.fr_array([c for g in bad for c in g])), nv,
                                      N.p64(co.fr_array([final])[0]), a._h, N.p64(ch), C.byref(nch), C.byref(ok))
    assert (st, ok.value, nch.value) == (0, 0, 3)  # an invalid proof is a result, not an error
    assert co.fr_ints(ch[:3]) == chal[:3] and not ch[3:].any()
    # the optional outputs may be left out
    a, _ = transcripts()
    st = N.load().tns_sumcheck_verify(nv, N.p64(co.fr_array([claim])[0]), N.p64(co.fr_array([c for g in rounds for c in g])),
                                      nv, N.p64(co.fr_array([final])[0]), a._h, None, None, C.byref(ok))
    assert (st, ok.value) == (0, 1)


def test_reference_x1_x2_proof_verifies(golden):
    """the reference's test_sumcheck_protocol_basic: f = x1 x2 over two variables, claimed sum 1,
    seed [42; 32] -- verify-only on the recorded proof (proving needs a device:
    tests/test_gpu_sumcheck_verify_batch.py proves and verifies)"""
    g = golden["sumcheck_x1x2"]
    rounds, final = [[h(c) for c in r] for r in g["rounds"]], h(g["final"])
    ok, chal = ts.SumCheck(2, 1).verify(ts.SumCheckProof(rounds, final), ts.Transcript(bytes([42] * 32)))
    assert ok is True and chal == [h(c) for c in g["challenges"]]
    assert final == chal[0] * chal[1] % R
    assert ref.sumcheck_verify(1, rounds, final, po.Transcript(bytes([42] * 32))) == (True, chal)
    ok, _ = ts.SumCheck(2, 2).verify(ts.SumCheckProof(rounds, final), ts.Transcript(bytes([42] * 32)))
    assert ok is False
