"""Big-integer reference of the device field and point primitives (csrc/bn254.hpp, mont_mul.inc,
field_asm.inc / field_bi.inc, group_ntt.hpp) and the operand sets their tests share.

Everything is a plain Python int.  The Montgomery constants are derived here from the two moduli
and R = 2^256 (test_field_primitives_cpu.py compares them with the header's); a field element on
the device is 8 x u32 little-endian limbs holding x R mod M, possibly lifted by +M in the lazy
domain [0, 2M).  test_gpu_field_primitives.py runs the operand sets through the device functions,
test_field_primitives_cpu.py through their host twins."""
import functools
import itertools
import random

from oracle import pyoracle as po

R = 1 << 256
MODULI = {"fr": po.R_MOD, "fq": po.P_MOD}
FIELDS = ("fr", "fq")
SEED = 0x7715F1E1D


class Field:
    """The constants of one field, derived from its modulus."""

    def __init__(self, name):
        self.name = name
        self.M = M = MODULI[name]
        self.M2 = 2 * M
        self.ONE = R % M
        self.R2 = R * R % M
        self.R3 = R * R * R % M
        self.RINV = pow(R, M - 2, M)
        self.INV32 = (-pow(M, -1, 1 << 32)) % (1 << 32)  # -M^-1 mod 2^32

    # ---- Montgomery-form arithmetic, canonical results
    def mont_mul(self, a, b):
        return a * b * self.RINV % self.M

    def mont_mul2(self, a, b, c, d):
        return (a * b + c * d) * self.RINV % self.M

    def add(self, a, b):
        return (a + b) % self.M

    def sub(self, a, b):
        return (a - b) % self.M

    def neg(self, a):
        return (-a) % self.M

    def to_mont(self, x):
        return x * R % self.M

    def from_mont(self, a):
        return a * self.RINV % self.M

    def inv_plain(self, x):
        return pow(x, self.M - 2, self.M)

    def mont_inv(self, a):
        """(x R) -> x^-1 R; inverse of zero is zero."""
        return self.to_mont(self.inv_plain(self.from_mont(a)))

    def sqrt_plain(self, x):
        """x^((p+1)/4): a square root of x where x is a square (p = 3 mod 4)."""
        assert self.M % 4 == 3
        return pow(x, (self.M + 1) // 4, self.M)

    def mont_sqrt_candidate(self, a):
        return self.to_mont(self.sqrt_plain(self.from_mont(a)))

    # ---- the exact integers of the lazy products (no final subtraction)
    def redc_exact(self, T):
        """(T + m M) / R with m = -T M^-1 mod R: what the product-scanning reduction leaves."""
        m = (-T * pow(self.M, -1, R)) % R
        q, rem = divmod(T + m * self.M, R)
        assert rem == 0
        return q

    def mul_lazy_exact(self, a, b):
        return self.redc_exact(a * b)

    def mul2_presub_exact(self, a, b, c, d):
        """Mont(a b + c d) before mul2_lazy_dev's one subtraction of 2M."""
        return self.redc_exact(a * b + c * d)


FR = Field("fr")
FQ = Field("fq")
BY_NAME = {"fr": FR, "fq": FQ}


# ------------------------------------------------------------------ limbs
def to_limbs(x):
    assert 0 <= x < R
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def from_limbs(w):
    return sum(int(v) << (32 * i) for i, v in enumerate(w))


def hexs(x):
    return "0x%064x" % x


# ------------------------------------------------------------------ operand sets
def all_ones_value(M):
    """The largest value below 2M whose low seven limbs are all ones."""
    low = (1 << 224) - 1
    v = ((2 * M - 1) >> 224 << 224) | low
    if v >= 2 * M:
        v -= 1 << 224
    return v


def edge_values(M):
    """Every edge operand, before filtering by a function's domain (sorted, no duplicates)."""
    ks = list(range(32, 225, 32)) + [254]
    v = [0, 1, 2, 3, M - 2, M - 1, M, M + 1, 2 * M - 2, 2 * M - 1]
    v += [R % M, R * R % M, M - R % M, R % M + M]
    v += [(M - 1) // 2, (M + 1) // 2]
    for k in ks:
        v += [(1 << k) - 1, 1 << k, (1 << k) + 1, M - (1 << k), M + (1 << k)]
    for i in range(8):
        cleared = M & ~(0xFFFFFFFF << (32 * i))
        v += [cleared, cleared | (0xFFFFFFFF << (32 * i))]
    v.append(all_ones_value(M))
    return sorted(set(x for x in v if 0 <= x < R))


def _rng(*tag):
    return random.Random("%x/%s" % (SEED, "/".join(str(t) for t in tag)))


@functools.lru_cache(maxsize=None)
def unary_cases(field, hi, closed=False, lo=0):
    """Edge values inside [lo, hi) (hi itself too when `closed`) plus 256 uniform draws."""
    M = MODULI[field]
    top = hi + 1 if closed else hi
    edges = [x for x in edge_values(M) if lo <= x < top]
    if closed and hi not in edges:
        edges.append(hi)
    rng = _rng(field, "unary", hi, closed, lo)
    return tuple(edges + [rng.randrange(lo, top) for _ in range(256)])


@functools.lru_cache(maxsize=None)
def binary_cases(field, hi, closed=False):
    """Every ordered pair of the in-domain edge values plus 4096 uniform pairs."""
    M = MODULI[field]
    top = hi + 1 if closed else hi
    edges = [x for x in edge_values(M) if x < top]
    if closed and hi not in edges:
        edges.append(hi)
    rng = _rng(field, "binary", hi, closed)
    pairs = list(itertools.product(edges, repeat=2))
    pairs += [(rng.randrange(top), rng.randrange(top)) for _ in range(4096)]
    return tuple(pairs)


@functools.lru_cache(maxsize=None)
def quad_cases(field):
    """mul2_lazy_dev: every quadruple of a ten-value core of [0, 2M) plus 4096 uniform ones."""
    M = MODULI[field]
    rng = _rng(field, "quad")
    core = [0, 1, M - 1, M, M + 1, 2 * M - 1, R % M, all_ones_value(M), rng.randrange(2 * M), rng.randrange(2 * M)]
    quads = list(itertools.product(core, repeat=4))
    quads += [tuple(rng.randrange(2 * M) for _ in range(4)) for _ in range(4096)]
    return tuple(quads)


@functools.lru_cache(maxsize=None)
def sqrt_cases():
    """Montgomery forms of squares, non-squares, 0, 1 and x^3 + 3 for small x (canonical Fq)."""
    f = FQ
    rng = _rng("sqrt")
    plain = [0, 1, 2, 3, 4, f.M - 1]
    plain += [(x * x * x + 3) % f.M for x in range(0, 40)]
    for _ in range(64):
        x = rng.randrange(f.M)
        plain += [x * x % f.M, x]
    non_squares = [x for x in plain if x and pow(x, (f.M - 1) // 2, f.M) != 1]
    squares = [x for x in plain if x and pow(x, (f.M - 1) // 2, f.M) == 1]
    assert len(non_squares) >= 16 and len(squares) >= 64
    return tuple(f.to_mont(x) for x in plain)


# ------------------------------------------------------------------ G1 (plain affine ints)
G1 = po.G1_GEN


def g1_add(A, B):
    return po.affine_add(A, B)


def g1_dbl(A):
    return po.affine_add(A, A)


def g1_mul(A, k):
    return po.affine_mul(A, k)


def g1_neg(A):
    return po.g1_neg(A)


def xyzz_is_inf(P):
    """The identity in the lazy domain: zz in {0, M}."""
    return P[2] % FQ.M == 0


def xyzz_to_affine(P):
    """Montgomery-form XYZZ (any representatives) -> plain affine (x / zz, y / zzz), None = identity."""
    f = FQ
    x, y, zz, zzz = (f.from_mont(c % f.M) for c in P)
    if zz == 0:
        return None
    return (x * f.inv_plain(zz) % f.M, y * f.inv_plain(zzz) % f.M)


def xyzz_of(A, lam=1, mask=0):
    """Plain affine A as Montgomery-form XYZZ (x l^2, y l^3, l^2, l^3), coordinate i lifted by +M
    where bit i of `mask` is set."""
    f = FQ
    l2, l3 = lam * lam % f.M, lam * lam * lam % f.M
    c = [f.to_mont(A[0] * l2 % f.M), f.to_mont(A[1] * l3 % f.M), f.to_mont(l2), f.to_mont(l3)]
    return tuple(v + (f.M if (mask >> i) & 1 else 0) for i, v in enumerate(c))


def affine_mont(A):
    """Plain affine -> the device's G1Affine (Montgomery x, y; the all-zero pair is the identity)."""
    if A is None:
        return (0, 0)
    return (FQ.to_mont(A[0]), FQ.to_mont(A[1]))


# ------------------------------------------------------------------ G1 operand sets
LAZY, CANON = "lazy", "canon"
INF_CANON = (1, 1, 0, 0)  # G1Xyzz::inf() before to_mont: only zz == 0 matters


@functools.lru_cache(maxsize=None)
def g1_points():
    """k G for k = 1..8 and eight random k, as (k, plain affine)."""
    rng = _rng("g1")
    ks = list(range(1, 9)) + [rng.randrange(1, FR.M) for _ in range(8)]
    return tuple((k, g1_mul(G1, k)) for k in ks)


@functools.lru_cache(maxsize=None)
def lambdas():
    return (1, 2, FQ.M - 1, _rng("lambda").randrange(3, FQ.M - 1))


def identities(domain):
    """The identity with junk in the other coordinates: zz = 0, and zz = M in the lazy domain."""
    rng = _rng("identity", domain)
    top = FQ.M2 if domain == LAZY else FQ.M
    out = []
    for zz in (0, FQ.M) if domain == LAZY else (0,):
        out.append((rng.randrange(top), rng.randrange(top), zz, rng.randrange(top)))
    return out


def _reps(A, domain, all_masks):
    """XYZZ forms of the plain affine point A: four lambdas; in the lazy domain also +M lifts."""
    out = []
    for n, lam in enumerate(lambdas()):
        if domain == CANON:
            masks = (0,)
        elif all_masks:
            masks = range(16)
        else:
            masks = (0, (5 * n + 3) % 16)
        out += [xyzz_of(A, lam, m) for m in masks]
    return out


@functools.lru_cache(maxsize=None)
def add_cases(domain, mixed):
    """(p, q, want) for xyzz_add[_lazy] (mixed = False: q in XYZZ) or xyzz_madd[_lazy] (mixed = True:
    q affine, canonical): generic sums, equal points in different forms (the doubling branch),
    opposite points, either or both operands the identity.  `want` is plain affine or None."""
    pts = g1_points()
    cases = []

    def q_forms(B, n):
        if mixed:
            return [affine_mont(B)]
        reps = _reps(B, domain, False)
        return [reps[n % len(reps)], reps[(n + 3) % len(reps)]]

    n = 0
    for i, (ka, A) in enumerate(pts):  # generic sums
        for j, (kb, B) in enumerate(pts):
            if i == j:
                continue
            reps = _reps(A, domain, False)
            for q in q_forms(B, n)[:1]:
                cases.append((reps[n % len(reps)], q, g1_add(A, B)))
            n += 1
    for i, (ka, A) in enumerate(pts):  # equal and opposite points
        for p in _reps(A, domain, i < 4):
            for q in q_forms(A, n):
                cases.append((p, q, g1_dbl(A)))
            for q in q_forms(g1_neg(A), n):
                cases.append((p, q, None))
            n += 1
    q_inf = [(0, 0)] if mixed else identities(domain)
    # xyzz_madd[_lazy] takes its accumulator's identity as zz == 0 only (bn254.hpp)
    p_inf = identities(domain)[:1] if mixed else identities(domain)
    for i, (ka, A) in enumerate(pts[:6]):  # identities
        for p in _reps(A, domain, False)[:3]:
            for q in q_inf:
                cases.append((p, q, A))
        for p in p_inf:
            for q in q_forms(A, i):
                cases.append((p, q, A))
    for p in p_inf:
        for q in q_inf:
            cases.append((p, q, None))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def dbl_cases(domain):
    """(p, want) for xyzz_dbl[_lazy]: every form of every point, the identities, and y = 0 (mod M)."""
    cases = []
    for i, (k, A) in enumerate(g1_points()):
        cases += [(p, g1_dbl(A)) for p in _reps(A, domain, i < 4)]
    cases += [(p, None) for p in identities(domain)]
    x, one = FQ.to_mont(5), FQ.ONE
    cases.append(((x, 0, one, one), None))
    if domain == LAZY:
        cases.append(((x, FQ.M, one + FQ.M, one), None))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def mdbl_cases():
    pts = [(affine_mont(A), g1_dbl(A)) for k, A in g1_points()]
    return tuple(pts + [((0, 0), None), ((FQ.to_mont(5), 0), None)])


@functools.lru_cache(maxsize=None)
def canon_cases():
    out = []
    for i, (k, A) in enumerate(g1_points()):
        out += _reps(A, LAZY, i < 4)
    return tuple(out + identities(LAZY))


@functools.lru_cache(maxsize=None)
def mul_cases():
    """(p, k, want) for xyzz_mul_canon: k a canonical plain integer below r."""
    rng = _rng("mul")
    r = FR.M
    ks = [0, 1, 2, r - 1, (1 << 32) - 1, 1 << 32, 1 << 64, 1 << 224] + [rng.randrange(r) for _ in range(8)]
    cases = []
    for i, (ka, A) in enumerate(g1_points()[5:9]):
        reps = _reps(A, LAZY, False)
        for n, k in enumerate(ks):
            for p in (reps[n % len(reps)], reps[(n + 5) % len(reps)]):
                cases.append((p, k, g1_mul(A, k)))
    for p in identities(LAZY):
        cases += [(p, k, None) for k in ks[:10]]
    return tuple(cases)


MADD_CHAIN_STEPS = 16


@functools.lru_cache(maxsize=None)
def madd_chain_cases():
    """(acc0, [16 affine q], [16 plain affine partial sums]) for a chain of xyzz_madd_lazy: from the
    identity, a point twice in a row (copy, then the doubling branch), generic steps, a repeated
    point mid-chain, the running sum itself (doubling with zz != 1), the sum's negation (back to
    the identity), the affine identity, then on from the identity."""
    pts = [A for k, A in g1_points()]
    chains = []
    for c in range(4):
        P = pts[c:] + pts[:c]
        acc0 = identities(LAZY)[0]  # (zz == 0: the only identity xyzz_madd_lazy's accumulator takes)
        plan = ["pt", "same", "pt", "pt", "same", "sum", "pt", "negsum", "inf", "pt", "same", "pt", "negsum", "pt",
                "sum", "pt"]
        assert len(plan) == MADD_CHAIN_STEPS
        S, qs, sums, nxt, last = None, [], [], 0, None
        for what in plan:
            if what == "pt":
                last = P[nxt]
                nxt += 1
            elif what == "sum":
                last = S
            elif what == "negsum":
                last = g1_neg(S)
            elif what == "inf":
                last = None
            q = last
            S = g1_add(S, q)
            qs.append(affine_mont(q))
            sums.append(S)
        assert any(s is None for s in sums)
        chains.append((acc0, tuple(qs), tuple(sums)))
    return tuple(chains)


def sub2_exact(a, b, f=FQ):
    return a - b if a >= b else a - b + f.M2


def branch_differences(cases, mixed):
    """The exact lazy differences (P, R) that xyzz_madd_lazy / xyzz_add_lazy form for each case
    whose operands are both finite: shows which representative of zero the doubling branch sees."""
    f = FQ
    out = []
    for p, q, want in cases:
        if p[2] % f.M == 0:
            continue
        if mixed:
            if q == (0, 0):
                continue
            U1, S1 = p[0], p[1]
            U2, S2 = f.mul_lazy_exact(q[0], p[2]), f.mul_lazy_exact(q[1], p[3])
        else:
            if q[2] % f.M == 0:
                continue
            U1, S1 = f.mul_lazy_exact(p[0], q[2]), f.mul_lazy_exact(p[1], q[3])
            U2, S2 = f.mul_lazy_exact(q[0], p[2]), f.mul_lazy_exact(q[1], p[3])
        out.append((sub2_exact(U2, U1), sub2_exact(S2, S1)))
    return out
