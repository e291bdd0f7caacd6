"""The Montgomery products of mont_mul.inc at the operands that load the columns whose carry
handling the generator (tools/gen_mac_blocks.py) reasons away or re-homes:

* column 0's first multiply-add has no carry instruction, and none of column 14's has one: the
  whole sum T = a b [+ c d] + m M stays below 2^512 (lazy: T <= 4M^2 + M 2^256, pair:
  T <= 8M^2 + M 2^256, inputs up to the closed bound 2M), so the last 64-bit column cannot
  overflow.  The operands here push T to those bounds: 2M - 1 and 2M in every position, M - 1, M,
  M + 1, the largest low limb and the largest top two limbs of the domain, 0 and 1.
* every column's overflow word is created by its first carry instruction and lives in the odd
  half of the register pair the next column accumulates into.  A word that leaked from one
  product's last column into the next product's first would show in dependent products: a chain
  of 33 steps alternating mul / sqr / mul2 from those corners, every step compared, and one XYZZ
  mixed-addition chain of 64 points (ten products a step, back to back in one kernel) that
  passes through doubling, cancellation and the identity.
* the mixed addition runs its independent products two at a time in one instruction stream
  (mul_lazy_x2_dev, sqr_lazy_x2_dev); one addition with corner values as coordinates is compared
  word for word with the host formulas.

Expected values are exact integers, (a b [+ c d] + m M) / 2^256 with m formed limb by limb as
the device forms it (redc_limbwise, checked against fieldref's closed form), not residues.  Same probe libraries, ops and runner as
test_gpu_field_primitives.py, on both carry-chain builds and both fields."""
import functools

import pytest

import fieldref as ref
from test_gpu_field_primitives import build, check_exact, check_points, field, flat, run

pytestmark = pytest.mark.gpu
CHAIN_STEPS = 33
MADD_STEPS = 64


def redc_limbwise(f, T):
    """(T + m M) / 2^256, m chosen one 32-bit limb at a time as the product scanning does: m_k
    clears word k of the running sum.  Equal to fieldref's closed form; kept separate so that the
    expected values do not rest on one formula."""
    for k in range(8):
        m_k = ((T >> (32 * k)) & 0xFFFFFFFF) * f.INV32 & 0xFFFFFFFF
        T += (m_k * f.M) << (32 * k)
    assert T % ref.R == 0 and T < 1 << 512
    return T >> 256


def red2m(f, t):
    return t - f.M2 if t >= f.M2 else t


@functools.lru_cache(maxsize=None)
def corners(field, top):
    """The corner operands inside [0, top]: see the module docstring."""
    f = ref.BY_NAME[field]
    ones32, ones192 = (1 << 32) - 1, (1 << 192) - 1
    v = [0, 1, f.M - 1, f.M, f.M + 1, f.M2 - 1, f.M2]
    for hi in (f.M - 1, f.M2 - 1, f.M2):
        low = hi | ones32  # the largest low limb ...
        v += [low if low <= hi else low - (1 << 32)]
        v += [hi >> 192 << 192, ((hi >> 192) - 1) << 192 | ones192]  # ... and the largest top two limbs
    v += [ref.all_ones_value(f.M), ones32, ones32 << 224]
    return tuple(sorted(set(x for x in v if 0 <= x <= top)))


@build
@field
def test_canonical_product_corners(build, field):
    """mul on every ordered pair of the corners of [0, M)."""
    f = ref.BY_NAME[field]
    cs = corners(field, f.M - 1)
    assert {0, 1, f.M - 1} <= set(cs) and any(c & 0xFFFFFFFF == 0xFFFFFFFF for c in cs)
    pairs = [(a, b) for a in cs for b in cs]
    want = [redc_limbwise(f, a * b) for a, b in pairs]
    want = [w - f.M if w >= f.M else w for w in want]
    assert want == [f.mont_mul(a, b) for a, b in pairs]
    check_exact("mul", pairs, run(build, field, "F_MUL", pairs), want)


@build
@field
def test_lazy_product_corners(build, field):
    """mul_lazy_dev / sqr_lazy_dev on every ordered pair of the corners of the closed domain
    [0, 2M]: T reaches 4M^2 + m M, results stay below 2M and equal the exact quotient."""
    f = ref.BY_NAME[field]
    cs = corners(field, f.M2)
    assert {0, 1, f.M - 1, f.M, f.M + 1, f.M2 - 1, f.M2} <= set(cs)
    pairs = [(a, b) for a in cs for b in cs]
    want = [redc_limbwise(f, a * b) for a, b in pairs]
    assert all(w < f.M2 for w in want) and want == [f.mul_lazy_exact(a, b) for a, b in pairs]
    check_exact("mul_lazy_dev", pairs, run(build, field, "F_MUL_LAZY", pairs), want)
    xs = [(a,) for a in cs]
    check_exact("sqr_lazy_dev", xs, run(build, field, "F_SQR_LAZY", xs), [redc_limbwise(f, a * a) for a, in xs])


@build
@field
def test_pair_product_corners(build, field):
    """mul2_lazy_dev with all four inputs at 2M, every mixed corner of {0, 1, M, 2M - 1, 2M}^4 and
    the large-limb corners in every position: T reaches 8M^2 + m M."""
    f = ref.BY_NAME[field]
    core = (0, 1, f.M, f.M2 - 1, f.M2)
    quads = [(a, b, c, d) for a in core for b in core for c in core for d in core]
    big = [c for c in corners(field, f.M2) if c > f.M + 1]
    for i, x in enumerate(big):
        y = big[(i + 1) % len(big)]
        quads += [(x, f.M2, f.M2, y), (f.M2, x, y, f.M2), (x, x, y, y), (x, y, y, x)]
    assert (f.M2,) * 4 in quads
    pre = [redc_limbwise(f, a * b + c * d) for a, b, c, d in quads]
    assert pre == [f.mul2_presub_exact(*q) for q in quads] and max(pre) < 4 * f.M
    assert sum(t >= f.M2 for t in pre) > 16  # the subtraction of 2M is exercised
    check_exact("mul2_lazy_dev", quads, run(build, field, "F_MUL2_LAZY", quads), [red2m(f, t) for t in pre])


@build
@field
def test_dependent_product_chain(build, field):
    """x = mul_lazy_dev(x, b); x = sqr_lazy_dev(x); x = mul2_lazy_dev(x, b, c, x); ... for 33
    steps from every corner, each step's result read back, compared exactly and fed to the next."""
    f = ref.BY_NAME[field]
    cs = corners(field, f.M2)
    xs = list(cs)
    bs = [cs[(3 * i + 1) % len(cs)] for i in range(len(cs))]
    ds = [cs[(5 * i + 2) % len(cs)] for i in range(len(cs))]
    for step in range(CHAIN_STEPS):
        kind = step % 3
        if kind == 0:
            cases = list(zip(xs, bs))
            got = run(build, field, "F_MUL_LAZY", cases)
            want = [redc_limbwise(f, x * b) for x, b in cases]
        elif kind == 1:
            cases = [(x,) for x in xs]
            got = run(build, field, "F_SQR_LAZY", cases)
            want = [redc_limbwise(f, x * x) for x, in cases]
        else:
            cases = [(x, b, d, x) for x, b, d in zip(xs, bs, ds)]
            got = run(build, field, "F_MUL2_LAZY", cases)
            want = [red2m(f, redc_limbwise(f, x * b + d * x)) for x, b, d, _ in cases]
        assert all(w < f.M2 for w in want)
        check_exact("chain step %d (%s)" % (step, ("mul", "sqr", "mul2")[kind]), cases, got, want)
        xs = want


def madd_lazy_exact(p, q):
    """xyzz_madd_lazy's generic branch in exact integers, product for product as bn254.hpp forms
    it (the independent products go through mul_lazy_x2_dev / sqr_lazy_x2_dev in pairs); None
    where the step leaves that branch (P = 0 mod M)."""
    f = ref.FQ
    mulx = lambda a, b: redc_limbwise(f, a * b)
    add2 = lambda a, b: red2m(f, a + b)
    sub2 = ref.sub2_exact
    x1, y1, zz, zzz = p
    U2, S2 = mulx(q[0], zz), mulx(q[1], zzz)
    P, R = sub2(U2, x1), sub2(S2, y1)
    if P % f.M == 0:
        return None
    PP, RR = mulx(P, P), mulx(R, R)
    PPP, Q = mulx(P, PP), mulx(x1, PP)
    zz3, zzz3 = mulx(zz, PP), mulx(zzz, PPP)
    x3 = sub2(sub2(RR, PPP), add2(Q, Q))
    y3 = red2m(f, redc_limbwise(f, R * sub2(Q, x3) + y1 * (f.M2 - PPP)))
    return (x3, y3, zz3, zzz3)


@build
def test_madd_lazy_exact_corners(build):
    """One mixed addition with corner values as coordinates (field arithmetic only: the operands
    need not be curve points), every output word against the host formulas.  This is where the
    paired products (two products' statements interleaved) meet the operands that load their
    carry-free columns: zz, zzz over the corners of [0, 2M), the affine x, y over those of [0, M)."""
    f = ref.FQ
    rng = ref._rng("madd-corners")
    zs = [c for c in corners("fq", f.M2 - 1) if c % f.M]  # zz = 0, M: the identity, another branch
    qs = [c for c in corners("fq", f.M - 1)]
    cases, want = [], []
    for i, zz in enumerate(zs):
        for j, x2 in enumerate(qs):
            p = (rng.randrange(f.M2), rng.randrange(f.M2), zz, zs[(i + j) % len(zs)])
            q = (x2, qs[(i + 2 * j + 1) % len(qs)])
            if q == (0, 0):
                continue
            for pp in (p, (f.M2 - 1, f.M2 - 1) + p[2:]):
                w = madd_lazy_exact(pp, q)
                if w is not None:
                    cases.append(flat(pp, q))
                    want.append(w)
    assert len(cases) > 100 and all(v < f.M2 for w in want for v in w)
    check_exact("xyzz_madd_lazy", cases, run(build, "fq", "G_MADD_LAZY", cases), want)


@functools.lru_cache(maxsize=None)
def madd_chain():
    """(acc0, 64 affine addends, 64 plain affine partial sums): from the identity, through a point
    twice in a row (copy, then doubling), the running sum itself (doubling with zz != 1), its
    negative (cancellation), the affine identity, and generic additions in between."""
    pts = [A for k, A in ref.g1_points()]
    plan = ("pt", "same", "pt", "pt", "sum", "pt", "negsum", "inf", "pt", "pt", "same", "pt", "pt", "negsum", "pt", "sum")
    acc0 = ref.identities(ref.LAZY)[0]
    S, qs, sums, nxt, last = None, [], [], 0, None
    for step in range(MADD_STEPS):
        what = plan[step % len(plan)]
        if what == "pt":
            last = pts[nxt % len(pts)]
            nxt += 1
        elif what == "sum":
            last = S
        elif what == "negsum":
            last = ref.g1_neg(S)
        elif what == "inf":
            last = None
        S = ref.g1_add(S, last)
        qs.append(ref.affine_mont(last))
        sums.append(S)
    assert sum(s is None for s in sums) >= 4
    return acc0, tuple(qs), tuple(sums)


@build
def test_madd_chain_64(build):
    acc0, qs, sums = madd_chain()
    cases = [flat(acc0, *qs)]
    got = run(build, "fq", "G_MADD_CHAIN", cases, MADD_STEPS)
    check_points("madd chain of 64", cases, got, [sums], canonical=False)
