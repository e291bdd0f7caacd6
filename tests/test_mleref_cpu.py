"""tests/mleref.py against the oracle's definitions (no GPU): the O(N) fold against
pyoracle.mle_evaluate (the reference's O(N n) sum over basis products) and against the table entry
at boolean points; sumcheck_verify against pyoracle.sumcheck_verify on the golden Twist / Shout
proofs (claimed sum 0) and on the C oracle's proofs of non-zero honest claims, which it must accept
with the prover's challenges."""
import random

import pytest

from oracle import coracle as co
from oracle import pyoracle as po

import mleref as ref

R = po.R_MOD
COMPOSITIONS = {  # tests/test_gpu_sumcheck_batch.py's table
    "twist_like": [(1, [0, 1]), (R - 1, [2, 2, 1]), (2, [2])],
    "dense4": [(17, [0, 1, 2]), (R - 3, [3, 3]), (5, [1, 2, 3]), (R - 1, [0]), (2, [2, 3]), (7, [])],
    "single": [(3, [0, 0, 0]), (R - 2, [0]), (5, [])],
    "pair2": [(1, [0, 1]), (4, [1, 1])],
}


def h(x):
    return int(x, 16)


@pytest.mark.parametrize("nv", range(7))
def test_fold_matches_the_basis_sum(nv):
    rng = random.Random(100 + nv)
    n = 1 << nv
    evals = [rng.randrange(R) for _ in range(n)]
    evals[rng.randrange(n)] = 0
    evals[rng.randrange(n)] = R - 1
    for point in ([rng.randrange(R) for _ in range(nv)], [0] * nv, [1] * nv, [R - 1] * nv,
                  [rng.choice([0, 1, R - 1, rng.randrange(R)]) for _ in range(nv)]):
        assert ref.mle_eval(evals, point) == po.mle_evaluate(evals, point)
    for index in {0, n - 1, rng.randrange(n)}:
        assert ref.mle_eval(evals, [(index >> i) & 1 for i in range(nv)]) == evals[index]
    # the Montgomery route: fold the forms, convert the one result
    arr = co.fr_array(evals)
    point = [rng.randrange(R) for _ in range(nv)]
    assert ref.mont_ints(arr) == [e * po.MONT_R % R for e in evals]
    assert ref.mle_eval_mont(arr, point) == po.mle_evaluate(evals, point)


def test_fold_rejects_a_wrong_dimension():
    with pytest.raises(AssertionError):
        ref.mle_eval([1, 2, 3, 4], [5])


def _golden_transcript(proof, labels):
    tr = po.Transcript(bytes(32))
    for lab, key in zip(labels, ("c0", "c1")):
        tr.append_field_element(lab, po.commitment_hash(proof[key]))
    return tr


def _golden_cases(golden):
    for kind, labels, keys in (("twist", (b"address_commitment", b"value_commitment"), ("address_commitment", "value_commitment")),
                               ("shout", (b"table_commitment", b"index_commitment"), ("table_commitment", "index_commitment"))):
        for name, case in golden[kind].items():
            g = case["proof"]
            pts = {k: (None if g[src] is None else (h(g[src][0]), h(g[src][1]))) for k, src in zip(("c0", "c1"), keys)}
            yield name, labels, pts, [[h(c) for c in r] for r in g["round_polynomials"]], h(g["final_evaluation"]), \
                [h(c) for c in g["sumcheck_challenges"]]


def test_verify_matches_the_oracle_on_golden_proofs(golden):
    seen = 0
    for name, labels, pts, rounds, final, chal in _golden_cases(golden):
        a, b = _golden_transcript(pts, labels), _golden_transcript(pts, labels)
        ok, got = ref.sumcheck_verify(0, rounds, final, a)
        assert ok is True and po.sumcheck_verify(rounds, final, b) is True, name
        assert got == chal, name
        assert a.state == b.state, name
        # a changed final and a changed coefficient: the same answers, the same transcript
        tampered = [(rounds, (final + 1) % R)]
        if rounds:
            last = [(rounds[-1][0] + 1) % R] + list(rounds[-1][1:])
            tampered.append((rounds[:-1] + [last], final))
        for r2, f2 in tampered:
            a, b = _golden_transcript(pts, labels), _golden_transcript(pts, labels)
            ok, got = ref.sumcheck_verify(0, r2, f2, a)
            assert ok is False and po.sumcheck_verify(r2, f2, b) is False, name
            assert a.state == b.state, name
        seen += 1
    assert seen >= 4


@pytest.mark.parametrize("nv", [0, 1, 2, 5])
@pytest.mark.parametrize("name", sorted(COMPOSITIONS))
def test_verify_accepts_oracle_proofs_of_nonzero_claims(name, nv):
    terms = COMPOSITIONS[name]
    k = 1 + max(max(ix) for _, ix in terms if ix)
    rng = random.Random(7 * nv + k)
    tables = [[rng.randrange(R) for _ in range(1 << nv)] for _ in range(k)]
    claim = sum(ref.composition(terms, [t[x] for t in tables]) for x in range(1 << nv)) % R
    assert claim != 0
    prefix = b"instance" + (12345).to_bytes(32, "little")
    st, rounds, fin, chal = co.sumcheck_prove([co.fr_array(t) for t in tables], nv, claim, terms, prefix=prefix)
    assert st == 0
    rounds = [co.fr_ints(r) for r in rounds]
    fin, chal = co.fr_ints(fin)[0], (co.fr_ints(chal) if nv else [])
    tr = po.Transcript(bytes(32))
    tr.append_field_element(b"instance", 12345)
    ok, got = ref.sumcheck_verify(claim, rounds, fin, tr)
    assert ok is True and got == chal
    # and the final evaluation is the composition of the tables' extensions at the challenges
    assert fin == ref.composition(terms, [ref.mle_eval(t, chal) for t in tables])
    # a wrong claim fails round 0 with nothing drawn and nothing appended
    if nv:
        tr = po.Transcript(bytes(32))
        assert ref.sumcheck_verify((claim + 1) % R, rounds, fin, tr) == (False, []) and not tr.state
