"""The transform reference (tests/nttref.py) proved on its own, without a device: the fast forward
and inverse transforms against an O(n^2) DFT, the convolution against the schoolbook product, the
operand convention of ntt_conv_blocks as an identity, the twiddle table's spot values and orders,
the factorials against math.factorial, and the pass split against a table worked out by hand from
the rule in ntt.hip's comment.  Every test counts what it checked."""
import math
import random

import nttref as ref

R = ref.R


def test_root_orders():
    assert ref.root(0) == 1 and ref.root(1) == R - 1
    checked = 0
    for lo in range(1, 29):
        w = ref.root(lo)
        assert pow(w, 1 << lo, R) == 1 and pow(w, 1 << (lo - 1), R) == R - 1, lo
        checked += 1
    assert checked == 28
    assert (R - 1) % (1 << 28) == 0 and (R - 1) % (1 << 29) != 0


def test_forward_is_the_bit_reversed_dft():
    rng = random.Random(1)
    checked = 0
    for s in range(0, 8):
        x = ref.rand_vec(rng, 1 << s)
        assert ref.forward(x) == ref.bitrev_permute(ref.dft_naive(x)), s
        checked += 1
    assert checked == 8


def test_inverse_against_the_naive_dft():
    """inverse(X bit-reversed)[j] = sum_k X[k] w^(-j k): the naive DFT with its output index negated"""
    rng = random.Random(2)
    checked = 0
    for s in range(0, 8):
        n = 1 << s
        X = ref.rand_vec(rng, n)
        d = ref.dft_naive(X)
        assert ref.inverse(ref.bitrev_permute(X)) == [d[-j % n] for j in range(n)], s
        checked += 1
    assert checked == 8


def test_inverse_of_forward_scales_by_n():
    rng = random.Random(3)
    checked = 0
    for s in list(range(0, 8)) + [11]:
        x = ref.rand_vec(rng, 1 << s)
        assert ref.inverse(ref.forward(x)) == [(v << s) % R for v in x], s
        checked += 1
    assert checked == 9


def test_cyclic_conv_agrees_with_schoolbook():
    rng = random.Random(4)
    checked = 0
    for s in range(0, 9):  # 2^7 and 2^8 take cyclic_conv's transform route
        x, k = ref.rand_vec(rng, 1 << s), ref.rand_vec(rng, 1 << s)
        assert ref.cyclic_conv(x, k) == ref.schoolbook_cyclic(x, k), s
        checked += 1
    assert checked == 9
    assert ref.schoolbook_cyclic([1, 2, 3, 4], [0, 1, 0, 0]) == [4, 1, 2, 3]


def test_conv_operand_identity():
    """inverse(forward(x) .* conv_operand(k, s)) is the cyclic convolution, with no further scaling"""
    rng = random.Random(5)
    checked = 0
    for s in range(1, 8):
        n = 1 << s
        x, k = ref.rand_vec(rng, n), ref.rand_vec(rng, max(1, n - 3))  # a short kernel is zero-padded
        w = ref.conv_operand(k, s)
        got = ref.inverse([a * b % R for a, b in zip(ref.forward(x), w)])
        assert got == ref.schoolbook_cyclic(x, k + [0] * (n - len(k))), s
        checked += 1
    assert checked == 7
    assert ref.conv_operand([1], 3) == [pow(8, R - 2, R)] * 8


def test_twiddle_table():
    L = 12
    tw = ref.twiddle_table(L)
    assert len(tw) == 1 << L
    assert tw[0] == 1 and tw[1] == 1 and tw[2] == 1 and tw[3] * tw[3] % R == R - 1
    checked = 0
    for lh in range(L):
        h = 1 << lh
        w = tw[h + 1] if h > 1 else R - 1  # (stage 0 has the one entry w_2^0)
        assert tw[h] == 1
        assert pow(w, 2 * h, R) == 1 and pow(w, h, R) == R - 1, "stage %d: order is not 2h" % lh
        assert w == ref.root(lh + 1)
        for k in (0, 1 % h, h // 2, h - 1):
            assert tw[h + k] == pow(w, k, R), (lh, k)
        checked += 1
    assert checked == L
    assert ref.twiddle_table(4) == tw[:16] and ref.twiddle_table(0) == [1]


def test_factorials():
    fact, ifact = ref.factorials(70)
    checked = 0
    for k in range(70):
        assert fact[k] == math.factorial(k) % R and fact[k] * ifact[k] % R == 1, k
        checked += 1
    assert checked == 70
    assert ref.factorials(1) == ([1], [1])


def test_pass_split_by_hand():
    table = {11: [(10, 1)], 12: [(10, 2)], 13: [(10, 3)], 14: [(10, 4)], 15: [(10, 5)],
             16: [(10, 3), (13, 3)], 17: [(10, 4), (14, 3)]}
    checked = 0
    for s, want in table.items():
        assert ref.pass_split(s) == want, s
        checked += 1
    assert checked == 7
    assert all(ref.pass_split(s) == [] for s in range(0, 11))
    assert ref.pass_split(21) == [(10, 4), (14, 4), (18, 3)]  # 11 stages in three passes: 4, 4, 3
    assert ref.pass_key(13, 3) == 0xD03


def test_rand_vec_mixes_in_the_edges():
    rng = random.Random(6)
    v = ref.rand_vec(rng, 64)
    assert all(e in v for e in ref.EDGES) and all(0 <= x < R for x in v)
    assert len(ref.rand_vec(rng, 2)) == 2
    limbs = ref.to_limbs(v)
    assert limbs.shape == (64, 4) and ref.from_limbs(limbs) == v
