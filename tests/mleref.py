"""Plain Python big-integer restatements for the verifier side of the generic sum-check
(tests/test_mleref_cpu.py proves them against the oracle's definitions):

  mle_eval        MultilinearExtension::evaluate (src/polynomials.rs:85-122) as an O(N) fold, one
                  variable a pass, variable i <-> index bit i (least significant first);
  sumcheck_verify SumCheck::verify (src/sumcheck.rs:113-153) for any claimed sum on
                  oracle.pyoracle.Transcript, with the reference's early return;
  composition     sum_t coeff_t prod_j values[idx_tj], the closure of the generic provers.

The fold is linear in the table, so it runs on whatever representation the entries come in:
mont_ints() reads a (n, 4) uint64 Montgomery array as integers a R without a conversion an entry,
and the folded result is then the value's Montgomery form (from_mont_int converts that one number).
"""
import numpy as np

from oracle import pyoracle as po

R = po.R_MOD
R_INV = pow(po.MONT_R, -1, R)


def mle_eval(evals, point):
    """sum_x evals[x] prod_i (x_i ? point[i] : 1 - point[i]) over len(evals) == 2^len(point) entries"""
    ev = list(evals)
    assert len(ev) == 1 << len(point), "Point dimension must match number of variables"
    for r in point:  # T'[s] = T[2s] + r (T[2s+1] - T[2s]) binds the lowest remaining variable
        ev = [(a + r * (b - a)) % R for a, b in zip(ev[0::2], ev[1::2])]
    return ev[0] % R


def mont_ints(arr):
    """(n, 4) uint64 limbs -> the n integers the limbs spell (Montgomery forms stay Montgomery forms)"""
    buf = np.ascontiguousarray(arr, dtype="<u8").reshape(-1, 4).tobytes()
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


def from_mont_int(x):
    return x * R_INV % R


def mle_eval_mont(arr, point):
    """mle_eval of a Montgomery table at a canonical point, canonical result"""
    return from_mont_int(mle_eval(mont_ints(arr), point))


def sumcheck_verify(claimed, rounds, final, transcript):
    """(ok, challenges); a failed round check returns before the round is appended"""
    cur = claimed % R
    challenges = []
    for r, c in enumerate(rounds):
        if (po.horner_eval(c, 0) + po.horner_eval(c, 1)) % R != cur:
            return False, challenges
        transcript.append_field_elements(b"sumcheck_round_%d" % r, c)
        ch = transcript.challenge_field_element(b"sumcheck_challenge_%d" % r)
        challenges.append(ch)
        cur = po.horner_eval(c, ch)
    return cur == final % R, challenges


def composition(terms, values):
    s = 0
    for coeff, idx in terms:
        p = coeff
        for j in idx:
            p = p * values[j] % R
        s = (s + p) % R
    return s % R
