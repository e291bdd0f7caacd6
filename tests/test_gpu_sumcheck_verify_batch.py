"""SumCheck::verify of a batch of generic sum-check proofs against their tables
(tns_sumcheck_verify_batch and its _device form; csrc/sumcheck_verify.hip).  The
proofs come from tns_sumcheck_prove_batch at (nv, batch) in {(1,3), (5,5), (8,4), (11,3), (14,2)}
over the four compositions of tests/test_gpu_sumcheck_batch.py, every instance with tables and a
transcript prefix of its own.  Honest proofs: every verdict 0, the prover's challenges, the
prover's transcript state (a challenge drawn afterwards), the tables' values equal to
tests/mleref.py's fold; host and resident entries agree.  Then one instance of a batch gets a
changed round coefficient, a changed final evaluation, one changed table entry, and a proof that is
valid for other tables: exactly that instance gets verdict 1, 2, 3 and 3.  Without tables the call
is the reference's check, which the changed entry passes -- asserted, since that is what the
evaluation adds.  Also: the oracle's proofs, nv = 0, a duplicate transcript, an empty batch, the
reference's x1 x2 example proved and verified, and the launch count of the evaluation inside one
call.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from oracle import coracle as co
from oracle import pyoracle as po

import twist_and_shout as ts
from twist_and_shout import _native as N

import mleevalprobe as mp
import mleref as ref
import test_gpu_sumcheck_batch as sb  # its compositions, cases (tables, claims, oracle proofs) and transcripts

pytestmark = pytest.mark.gpu
R = po.R_MOD
SHAPES = [(1, 3), (5, 5), (8, 4), (11, 3), (14, 2)]
NAMES = ["twist_like", "dense4", "single", "pair2"]


def prove(name, nv, batch, tabs=None, claims=None):
    """tns_sumcheck_prove_batch on fresh prefixed transcripts: (proofs, challenges, the challenge
    drawn from every transcript afterwards)"""
    t0, c0, _ = sb.case(name, nv, batch)
    trs = sb.transcripts(batch)
    proofs, chals = ts.SumCheck(nv, 0).prove_batch(tabs or t0, sb.COMPOSITIONS[name], trs, claims or c0,
                                                   return_challenges=True)
    return proofs, chals, sb.after(trs)


def values_of(tabs, chals):
    return [[ref.mle_eval_mont(t[b], chals[b]) for t in tabs] for b in range(len(chals))]


def tamper_round(proofs, b, r):
    out = [ts.SumCheckProof([list(g) for g in p.round_polynomials], p.final_evaluation) for p in proofs]
    out[b].round_polynomials[r][1] = (out[b].round_polynomials[r][1] + 1) % R  # g(0) + g(1) moves by 1
    return out


@pytest.mark.parametrize("nv,batch", SHAPES)
@pytest.mark.parametrize("name", NAMES)
def test_honest_proofs_verify_against_their_tables(name, nv, batch):
    terms = sb.COMPOSITIONS[name]
    tabs, claims, want = sb.case(name, nv, batch)
    proofs, chals, drawn = prove(name, nv, batch)
    trs = sb.transcripts(batch)
    verdicts, vch, vals = ts.SumCheck(nv, 0).verify_batch(proofs, tabs, terms, trs, claims, return_values=True)
    assert verdicts == [0] * batch
    assert vch == chals
    assert sb.after(trs) == drawn
    assert vals == values_of(tabs, chals)
    for b in range(batch):  # what verdict 0 states
        assert proofs[b].final_evaluation == ref.composition(terms, vals[b])
    # the resident entry: the same answers, the inputs only read
    ctx = ts.Context.get(0)
    bufs = [ts.DeviceBuffer(ctx, t) for t in tabs]
    trs = sb.transcripts(batch)
    assert ts.SumCheck(nv, 0).verify_batch_resident(proofs, bufs, terms, trs, claims, return_values=True) == \
        (verdicts, vch, vals)
    assert sb.after(trs) == drawn
    for t, dt in zip(tabs, bufs):
        back = np.empty_like(t)
        ts.buffer_download(dt, back)
        assert np.array_equal(back, t)
    # without tables: the reference's verify, batched
    trs = sb.transcripts(batch)
    assert ts.SumCheck(nv, 0).verify_batch(proofs, None, terms, trs, claims) == (verdicts, vch)
    assert sb.after(trs) == drawn


@pytest.mark.parametrize("nv,batch", SHAPES)
@pytest.mark.parametrize("name", NAMES)
def test_one_bad_instance_gets_its_verdict_and_the_others_stay_valid(name, nv, batch):
    terms = sb.COMPOSITIONS[name]
    tabs, claims, want = sb.case(name, nv, batch)
    proofs, chals, drawn = prove(name, nv, batch)
    honest_vals = values_of(tabs, chals)
    bad = batch // 2
    sc = ts.SumCheck(nv, 0)

    def expect(verdict):
        return [verdict if b == bad else 0 for b in range(batch)]

    def honest_rows_but_zero_at_bad():
        return [[0] * len(tabs) if b == bad else honest_vals[b] for b in range(batch)]

    # a changed round coefficient: verdict 1, the replay stops at that round
    r = nv // 2
    trs = sb.transcripts(batch)
    verdicts, vch, vals = sc.verify_batch(tamper_round(proofs, bad, r), tabs, terms, trs, claims, return_values=True)
    assert verdicts == expect(1)
    assert vch == [chals[b][:r] if b == bad else chals[b] for b in range(batch)]
    assert vals == honest_rows_but_zero_at_bad()  # the failed instance rode along at the zero point: a zero row
    assert [d for b, d in enumerate(sb.after(trs)) if b != bad] == [d for b, d in enumerate(drawn) if b != bad]

    # a changed final evaluation: verdict 2, every challenge drawn
    off = [ts.SumCheckProof(p.round_polynomials, (p.final_evaluation + (b == bad)) % R) for b, p in enumerate(proofs)]
    trs = sb.transcripts(batch)
    verdicts, vch, vals = sc.verify_batch(off, tabs, terms, trs, claims, return_values=True)
    assert verdicts == expect(2) and vch == chals and vals == honest_rows_but_zero_at_bad()
    assert sb.after(trs) == drawn

    # one changed entry of table 0 (a factor of a term in every composition): verdict 3
    t0 = tabs[0].copy()
    x = (3 * bad + 1) % (1 << nv)
    t0[bad, x] = co.fr_array([(co.fr_ints(t0[bad, x])[0] + 1) % R])[0]
    changed = [t0] + list(tabs[1:])
    trs = sb.transcripts(batch)
    verdicts, vch, vals = sc.verify_batch(proofs, changed, terms, trs, claims, return_values=True)
    assert verdicts == expect(3) and vch == chals
    assert vals == values_of(changed, chals) and vals[bad][0] != honest_vals[bad][0]
    assert sb.after(trs) == drawn
    # ... which the reference's check passes: it never looks at a table
    trs = sb.transcripts(batch)
    assert sc.verify_batch(proofs, None, terms, trs, claims) == ([0] * batch, chals)

    # a valid proof of other tables (instance `bad` proved on its neighbour's rows, same transcript
    # prefix, that neighbour's honest claim): the replay holds, the tables do not -- verdict 3
    other = (bad + 1) % batch
    swapped = []
    for t in tabs:
        s = t.copy()
        s[bad] = t[other]
        swapped.append(s)
    claims2 = list(claims)
    claims2[bad] = claims[other]
    proofs2, chals2, drawn2 = prove(name, nv, batch, swapped, claims2)
    trs = sb.transcripts(batch)
    verdicts, vch = sc.verify_batch(proofs2, swapped, terms, trs, claims2)
    assert verdicts == [0] * batch and vch == chals2  # (valid where it was proved)
    trs = sb.transcripts(batch)
    verdicts, vch = sc.verify_batch(proofs2, tabs, terms, trs, claims2)
    assert verdicts == expect(3) and vch == chals2
    assert sb.after(trs) == drawn2


@pytest.mark.parametrize("nv,batch", [(5, 5), (11, 3)])
def test_oracle_proofs_verify(nv, batch):
    name = "dense4"
    terms = sb.COMPOSITIONS[name]
    tabs, claims, want = sb.case(name, nv, batch)
    proofs = [ts.SumCheckProof(w[0], w[1]) for w in want]
    trs = sb.transcripts(batch)
    verdicts, vch = ts.SumCheck(nv, 0).verify_batch(proofs, tabs, terms, trs, claims)
    assert verdicts == [0] * batch and vch == [w[2] for w in want]
    assert sb.after(trs) == [w[3] for w in want]


def test_no_variables():
    terms = sb.COMPOSITIONS["twist_like"]
    tabs, claims, want = sb.case("twist_like", 0, 3)
    proofs = [ts.SumCheckProof([], w[1]) for w in want]
    entries = [[co.fr_ints(t[b])[0] for t in tabs] for b in range(3)]
    out = ts.SumCheck(0, 0).verify_batch(proofs, tabs, terms, sb.transcripts(3), claims, return_values=True)
    assert out == ([0, 0, 0], [[], [], []], entries)  # the table value is T[b][0]
    wrong = [claims[0], (claims[1] + 1) % R, claims[2]]
    out = ts.SumCheck(0, 0).verify_batch(proofs, tabs, terms, sb.transcripts(3), wrong, return_values=True)
    assert out == ([0, 2, 0], [[], [], []], [entries[0], [0, 0, 0], entries[2]])  # claim != final
    t2 = tabs[2].copy()
    t2[2, 0] = co.fr_array([5])[0]
    assert ts.SumCheck(0, 0).verify_batch(proofs, [tabs[0], tabs[1], t2], terms, sb.transcripts(3), claims)[0] == [0, 0, 3]


def test_empty_batch_and_invalid_calls():
    nv, batch = 5, 5
    terms = sb.COMPOSITIONS["twist_like"]
    tabs, claims, want = sb.case("twist_like", nv, batch)
    proofs = [ts.SumCheckProof(w[0], w[1]) for w in want]
    assert ts.SumCheck(nv, 0).verify_batch([], [t[:0] for t in tabs], terms, [], []) == ([], [])
    trs = sb.transcripts(batch)
    trs[3] = trs[0]  # the same transcript twice
    with pytest.raises(ts.InvalidParameters, match="twice"):
        ts.SumCheck(nv, 0).verify_batch(proofs, tabs, terms, trs, claims)
    with pytest.raises(ts.InvalidParameters, match="missing table"):
        ts.SumCheck(nv, 0).verify_batch(proofs, tabs[:2], terms, sb.transcripts(batch), claims)
    with pytest.raises(ts.InvalidParameters):  # a table one entry short
        ts.SumCheck(nv, 0).verify_batch(proofs, [tabs[0], tabs[1].reshape(-1, 4)[:-1], tabs[2]], terms,
                                        sb.transcripts(batch), claims)
    with pytest.raises(ts.SumCheckError, match="wrong number of rounds"):  # (the Python mirror's own check)
        ts.SumCheck(nv, 0).verify_batch([ts.SumCheckProof(p.round_polynomials[:-1], p.final_evaluation) for p in proofs],
                                        tabs, terms, sb.transcripts(batch), claims)
    many = [(1, [0])] * 65
    with pytest.raises(ts.InvalidParameters, match="64"):
        ts.SumCheck(nv, 0).verify_batch(proofs, tabs, many, sb.transcripts(batch), claims)
    # the context verifies correctly afterwards
    trs = sb.transcripts(batch)
    assert ts.SumCheck(nv, 0).verify_batch(proofs, tabs, terms, trs, claims)[0] == [0] * batch
    assert sb.after(trs) == [w[3] for w in want]


def test_reference_x1_x2_prove_then_verify():
    """the reference's test_sumcheck_protocol_basic: f = x1 x2, claimed sum 1, seed [42; 32], proved
    and then verified on a fresh transcript"""
    x1, x2 = [0, 1, 0, 1], [0, 0, 1, 1]
    terms = [(1, [0, 1])]
    sc = ts.SumCheck(2, 1)
    proof = sc.prove([x1, x2], terms, ts.Transcript(bytes([42] * 32)))
    ok, chal = sc.verify(proof, ts.Transcript(bytes([42] * 32)))
    assert ok is True and len(chal) == 2 and proof.final_evaluation == chal[0] * chal[1] % R
    assert sc.verify_tables(proof, [x1, x2], terms, ts.Transcript(bytes([42] * 32))) == (True, chal)
    assert sc.verify_tables(proof, [x1, [0, 0, 1, 0]], terms, ts.Transcript(bytes([42] * 32))) == (False, chal)


@pytest.mark.parametrize("nv,batch", [(8, 4), (14, 2)])
def test_one_verify_call_is_one_evaluation_pass(nv, batch):
    name = "twist_like"
    terms = sb.COMPOSITIONS[name]
    tabs, claims, want = sb.case(name, nv, batch)
    trs = sb.transcripts(batch)
    rounds = co.fr_array([c for w in want for g in w[0] for c in g])
    finals = co.fr_array([w[1] for w in want])
    ch = np.zeros((batch * nv, 4), dtype=np.uint64)
    nch = np.zeros(batch, dtype=np.uint32)
    verdicts = np.full(batch, 9, dtype=np.int32)
    vals = np.zeros((batch, len(tabs), 4), dtype=np.uint64)
    info = (C.c_int64 * 4)()
    st = mp.lib().mleevalprobe_verify(ts.Context.get(0).handle, mp.table_ptrs(tabs, None), len(tabs), nv, batch,
                                      N.p64(co.fr_array(claims)), sb.terms_array(terms), len(terms),
                                      (C.c_void_p * batch)(*[t._h for t in trs]), N.p64(rounds), N.p64(finals), 0,
                                      N.p64(ch), nch.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      verdicts.ctypes.data_as(C.POINTER(C.c_int)), N.p64(vals), info)
    assert st == 0, N.last_error()
    assert tuple(info) == mp.plan(nv, batch) and info[1] <= 2
    assert list(verdicts) == [0] * batch and list(nch) == [nv] * batch
    assert co.fr_ints(ch) == [c for w in want for c in w[2]]
