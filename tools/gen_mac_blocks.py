#!/usr/bin/env python3
"""Generate product-scanning Montgomery multiplications whose MACs are emitted G per inline-asm
block (tools/mac_blocks.inc).  One asm block per MAC lets the compiler insert a wait state
(s_nop) between consecutive blocks; larger blocks keep the carry chain inside one statement.
Also writes the library's csrc/mont_mul.inc (whole columns per block; its header comment,
LIB_HEADER, describes the column shift) and csrc/field_asm.inc.  Run from the repository root."""
import sys


def ab_products(k):
    lo = 0 if k < 8 else k - 7
    return [(f"a.v[{i}]", f"b.v[{k - i}]", "v") for i in range(lo, min(k, 7) + 1)]


# Squaring: a^2 = sum_i a_i^2 2^(64 i) + sum_i a_i (2 S_i) with 2 S_i = 2 sum_{j>i} a_j 2^(32 j), whose
# limbs are e_i = a_{i+1} << 1 at j = i + 1 and d_j = a_j << 1 | a_{j-1} >> 31 above; its top limb
# a_7 >> 31 is zero for inputs < 2M < 2^255.  36 products instead of 64.
def sqr_products(k):
    lo = 0 if k < 8 else k - 7
    prods = []
    for i in range(lo, min(k, 7) + 1):
        j = k - i
        if i < j:
            prods.append((f"a.v[{i}]", f"e[{i}]" if j == i + 1 else f"d[{j}]", "v"))
        elif i == j:
            prods.append((f"a.v[{i}]", f"a.v[{i}]", "v"))
    return prods


SQR_PRELUDE = """  u32 d[8], e[7];
#pragma unroll
  for (int j = 2; j < 8; j++) d[j] = (a.v[j] << 1) | (a.v[j - 1] >> 31);
#pragma unroll
  for (int i = 0; i < 7; i++) e[i] = a.v[i + 1] << 1;"""


def cd_products(k):
    lo = 0 if k < 8 else k - 7
    return [(f"c.v[{i}]", f"d.v[{k - i}]", "v") for i in range(lo, min(k, 7) + 1)]


def one_products(k):
    return [(f"a.v[{k}]", "1u", "s")] if k < 8 else []


def gen_body(G, square=False, pair=False, redc=False):
    """The declarations and the statements (one list entry each) of one product on the operands
    a, b[, c, d]; the result is left in r[0..7].  No asm statement has an early-clobber output
    (see emit)."""
    out = []
    products = sqr_products if square else ab_products
    if redc:  # a * 1: Montgomery reduction of a alone (the canonical value of a Montgomery form)
        products = one_products
    elif pair:
        products = lambda k: ab_products(k) + cd_products(k)
    decls = ([SQR_PRELUDE] if square else []) + ["  u32 m[8], r[8];\n  unsigned long long acc;\n  u32 c2;"]

    MAD = "v_mad_u64_u32 %0, vcc, %{x}, %{y}, %0"

    def stmt(body, outs, macs):
        ins = []
        for x, y, yc in macs:
            ins += [f'"v"({x})', f'"{yc}"({y})']
        out.append('  asm("' + "\\n\\t".join(body) + '" : ' + outs + " : " + ", ".join(ins) + ' : "vcc");')

    def emit(macs, opens=True, carries=True):
        # macs: list of (xexpr, yexpr, ycons), one column's (or its Montgomery step's) multiply-adds.
        # opens: the first MAC creates the column's overflow word c2 from constants (0 + 0 + carry)
        # instead of adding into a word zeroed beforehand.  c2 is then a fresh, untied output, legal
        # WITHOUT an early clobber only as the destination of its statement's last instruction (every
        # input has been read by then), so that MAC and its carry are a statement of their own.
        # Everywhere else acc and c2 are TIED operands ("+v"): no statement has an early-clobber
        # output.  hipcc (ROCm 7.2) allocated an early-clobber carry word on the register of a live
        # input (a.v[7]) when it coalesced the word into the next column's 64-bit pair
        # (tools/chainfuse.hip)
        # carries=False: no MAC of the list can carry out of the 64-bit accumulator (the caller
        # states the bound); VCC is still written, nothing reads it.
        if not carries:
            for s in range(0, len(macs), G):
                grp = macs[s:s + G]
                stmt([MAD.format(x=1 + 2 * t, y=2 + 2 * t) for t in range(len(grp))], '"+v"(acc)', grp)
            return
        if opens:
            stmt([MAD.format(x=2, y=3), "v_addc_co_u32_e64 %1, vcc, 0, 0, vcc"], '"+v"(acc), "=v"(c2)', macs[:1])
            macs = macs[1:]
        for s in range(0, len(macs), G):
            grp = macs[s:s + G]
            body = []
            for t in range(len(grp)):
                body.append(MAD.format(x=2 + 2 * t, y=3 + 2 * t))
                body.append("v_addc_co_u32_e32 %1, vcc, 0, %1, vcc")
            stmt(body, '"+v"(acc), "+v"(c2)', grp)

    # Column shift: the sum moves down one word, acc = acc >> 32 | c2 << 32.  c2 is a new value in
    # every column, so the register allocator homes it in the odd half of the pair the NEXT column
    # accumulates into, and the shift is the one move "next pair's low word = this pair's high
    # word"; two pairs alternate.  (Recycling the low word a Montgomery step cleared as the next
    # zero carry word, as before, put that zero in an even register: every second shift then took
    # two moves, and columns 8-14 a copy of a zero register each.)
    SHIFT = "  acc = (acc >> 32) | ((unsigned long long)c2 << 32);"
    # Dead carries, by the size of T = (the products) + m M, m < 2^256:
    #   canonical (mul_ps_dev, redc_dev):  T < M^2 + M 2^256
    #   lazy (mul_lazy_dev, sqr_lazy_dev), inputs <= 2M (the closed domain of sumcheck.hip included):
    #                                      T <= 4M^2 + M 2^256
    #   pair (mul2_lazy_dev), inputs <= 2M: T <= 8M^2 + M 2^256
    # With M < 2^254 all of them are below 2^509 + 2^510 < 2^512.  The column sums add T up from
    # its low end, every partial sum is <= T, and entering column k the accumulator holds the
    # partial sum >> 32 k.  So in column 14 the accumulator never exceeds T >> 448 < 2^64: none of
    # its MACs carries, and r[7] is its high word.  Column 0's first MAC adds one 64-bit product to
    # nothing: it is written as the product alone (src2 = 0), which also spares zeroing acc.
    for k in range(8):
        macs = products(k)
        macs += [(f"m[{i}]", f"C::M[{k - i}]", "s") for i in range(k)]
        if k == 0:
            x, y, yc = macs[0]
            out.append(f"  acc = (unsigned long long){x} * {y};")
            macs = macs[1:]
        if macs:
            emit(macs)
        out.append(f"  m[{k}] = (u32)acc * C::INV;")
        # its own block: m[k] depends on the column sum
        emit([(f"m[{k}]", "C::M[0]", "s")], opens=not macs)
        out.append(SHIFT)
    for k in range(8, 15):
        macs = products(k)
        macs += [(f"m[{i}]", f"C::M[{k - i}]", "s") for i in range(k - 7, 8)]
        emit(macs, carries=k < 14)
        out.append(f"  r[{k - 8}] = (u32)acc;")
        if k < 14:
            out.append(SHIFT)
        else:
            out.append("  acc >>= 32;")
    out.append("  r[7] = (u32)acc;")
    return decls, out


def gen(G, name, reduce=True, square=False, pair=False, redc=False):
    """reduce: True -> conditional subtraction of M; False -> none (lazy, inputs < 2M give < 2M);
    "2m" -> subtraction of 2M (pair: Mont(a b + c d) < 2.51 M for inputs < 2M, back below 2M)."""
    if pair:
        args = "const Fp<C> &a, const Fp<C> &b, const Fp<C> &c, const Fp<C> &d"
    else:
        args = "const Fp<C> &a" if square or redc else "const Fp<C> &a, const Fp<C> &b"
    decls, steps = gen_body(G, square, pair, redc)
    out = [f"template <class C>\n__device__ __forceinline__ Fp<C> {name}({args}) {{"] + decls + steps
    out.append("  Fp<C> o;\n#pragma unroll\n  for (int i = 0; i < 8; i++) o.v[i] = r[i];")
    if reduce == "2m":
        out.append("  reduce_once_2m_dev(o);\n  return o;\n}\n")
    else:
        out.append("  reduce_once(o);\n  return o;\n}\n" if reduce else "  return o;\n}\n")
    return "\n".join(out)


def step_kind(text):
    """asm: an inline-asm statement; free: a word of the accumulator taken as a result limb (no
    instruction); valu: C the compiler turns into one VALU instruction (column 0's product, m[k],
    the column shift's move)."""
    if text.startswith("  asm("):
        return "asm"
    return "free" if text.startswith("  r[") or text.startswith("  acc >>=") else "valu"


def interleave(steps0, steps1, window=6):
    """Merge two independent products' statement lists into the order that costs the fewest wait
    states.  hipcc (gfx950) puts an s_nop after an asm statement when the next instruction is
    another asm statement (any: they all write VCC) or reads the statement's outputs -- within
    one product that is the next step, whatever it is.  Each list stays in order and the two stay
    within `window` steps of each other (register pressure).  Dynamic programming over (steps
    taken of each, what the last instruction was); returns [(which product, step index)]."""
    kinds = [[step_kind(t) for t in steps0], [step_kind(t) for t in steps1]]
    n = [len(steps0), len(steps1)]
    best = {(0, 0, "valu", 0): (0, None)}  # state -> (wait states so far, previous state)
    order = sorted((i + j, i, j) for i in range(n[0] + 1) for j in range(n[1] + 1) if abs(i - j) <= window)
    for _, i, j in order:
        for last in ("valu", "asm"):
            for who in (0, 1):
                st = (i, j, last, who)
                if st not in best:
                    continue
                cost = best[st][0]
                for c in ((0, 1) if i <= j else (1, 0)):  # ties go to the product that is behind
                    pos = (i, j)[c]
                    if pos == n[c] or abs(i + (c == 0) - j - (c == 1)) > window:
                        continue
                    k = kinds[c][pos]
                    if k == "free":
                        nxt, add = (i + (c == 0), j + (c == 1), last, who), 0
                    else:
                        add = int(last == "asm" and (k == "asm" or who == c))
                        nxt = (i + (c == 0), j + (c == 1), k, c)
                    if nxt not in best or best[nxt][0] > cost + add:
                        best[nxt] = (cost + add, (st, c, pos))
    end = min((v[0], k) for k, v in best.items() if k[0] == n[0] and k[1] == n[1])[1]
    seq = []
    while best[end][1] is not None:
        prev, c, pos = best[end][1]
        seq.append((c, pos))
        end = prev
    return seq[::-1]


def gen_x2(G, name, square=False):
    """Two independent lazy products (or squares) in one instruction stream: (a0 b0, a1 b1) ->
    (o0, o1).  Inside one product every statement continues the one before, so hipcc owes a wait
    state at every boundary; with a second, independent product at hand most boundaries can be
    followed by an instruction of the other product (interleave).  The order is pinned with
    scheduling barriers -- left alone, the machine scheduler regroups the statements.  The
    results are written after the last statement, so an output may be one of the inputs."""
    import re
    both = []
    for sfx in "01":
        decls, steps = gen_body(G, square)
        ren = lambda t: re.sub(r"\b(acc|c2|m|r|d|e|a|b)\b", lambda mo: mo.group(1) + sfx, t)
        both.append(([ren(t) for t in decls], [ren(t) for t in steps]))
    args = ("const Fp<C> &x0, const Fp<C> &x1" if square else
            "const Fp<C> &x0, const Fp<C> &y0, const Fp<C> &x1, const Fp<C> &y1")
    out = [f"template <class C>\n__device__ __forceinline__ void {name}({args}, Fp<C> &o0, Fp<C> &o1) {{"]
    # operands that still sit in memory are loaded here, ahead of the first barrier: a load left at
    # its first use could not be moved up any more and would be waited for inside the product
    out.append("  const Fp<C> a0 = x0, a1 = x1;" if square else "  const Fp<C> a0 = x0, b0 = y0, a1 = x1, b1 = y1;")
    out += both[0][0] + both[1][0]
    for c, pos in interleave(both[0][1], both[1][1]):
        text = both[c][1][pos]
        out.append(text if step_kind(text) == "free" else text + "\n  __builtin_amdgcn_sched_barrier(0);")
    out.append("#pragma unroll\n  for (int i = 0; i < 8; i++) o0.v[i] = r0[i], o1.v[i] = r1[i];\n}\n")
    return "\n".join(out)


LIB_HEADER = """// mont_mul.inc -- generated by tools/gen_mac_blocks.py (do not edit): the device Montgomery
// product of bn254.hpp.  Product scanning: column k accumulates every a_i b_j and m_i M_j with
// i + j = k into a 64-bit register pair with v_mad_u64_u32, whose carry-out (VCC) feeds a
// 32-bit overflow word via v_addc_co_u32.  Each column's MACs (up to 16) go out as one
// inline-asm block: the compiler separates consecutive asm statements by a wait state (s_nop),
// so one MAC per statement cost ~1 nop per MAC (tools/mulbench2.hip: Fq mul 112 -> 117 G/s with
// blocks of 8; tools/maddbench.hip: XYZZ madd 10.51 -> 10.66 G/s from 8 to whole columns).
// The column shift: a column's overflow word is a NEW value, created by the column's first carry
// instruction from constants (v_addc_co_u32_e64 c2, vcc, 0, 0, vcc), so the register allocator
// homes it in the odd half of the pair the next column accumulates into and the shift is one
// move (next pair's low word = this pair's high word); two pairs alternate, nothing is zeroed
// or copied beforehand.  That first MAC and its carry are a two-instruction statement of their
// own: the fresh word is the destination of the statement's LAST instruction, the one place
// where an untied output needs no early clobber; everywhere else the accumulator and the word
// are tied operands -- no statement has an early-clobber output (tools/gen_mac_blocks.py emit).
// Carries that cannot occur have no instruction: column 0's first MAC is the product alone, and
// column 14 cannot overflow 64 bits because the whole sum is below 2^512 (bounds: gen_body).
// mul_lazy_x2_dev / sqr_lazy_x2_dev run two independent products in one instruction stream, in
// the order that owes the fewest wait states (gen_x2 / interleave).
"""

G_LIB = int(__import__("os").environ.get("TNS_MAC_BLOCK", "16"))

if __name__ == "__main__":
    dst = sys.argv[1] if len(sys.argv) > 1 else "tools/mac_blocks.inc"
    with open(dst, "w") as f:
        f.write("// generated by tools/gen_mac_blocks.py -- do not edit\n")
        for G in (2, 4, 8):
            f.write(gen(G, f"mul_blk{G}") + "\n")
    with open("multilinear-map-cryptography_amd/csrc/mont_mul.inc", "w") as f:
        f.write(LIB_HEADER)
        f.write("#define TNS_HAVE_MUL_X2 1  // mul_lazy_x2_dev / sqr_lazy_x2_dev are defined here\n")
        f.write("// a b / R mod M, canonical: a, b in [0, M) -> [0, M) (any a b < M 2^256 would do: the sum is\n"
                "// below 2M before the one conditional subtraction)\n")
        f.write(gen(G_LIB, "mul_ps_dev") + "\n")
        f.write("// the same product without the final conditional subtraction: for inputs < 2M the\n"
                "// result is < 2M (4M < 2^256), the lazy-reduction domain of the MSM accumulation; so do inputs\n"
                "// <= 2M (4M^2 / R + M < 1.76 M: the closed domain of sumcheck.hip's round kernel)\n")
        f.write(gen(G_LIB, "mul_lazy_dev", reduce=False) + "\n")
        f.write("// the lazy product a * a: 36 products instead of 64 (input <= 2M < 2^255, see sqr_products;\n"
                "// result < 2M as mul_lazy_dev's)\n")
        f.write(gen(G_LIB, "sqr_lazy_dev", reduce=False, square=True) + "\n")
        f.write("// two independent lazy products / squares at once, statement by statement (see gen_x2): the\n"
                "// mixed addition's products come in independent pairs (bn254.hpp xyzz_madd_lazy)\n")
        f.write(gen_x2(G_LIB, "mul_lazy_x2_dev") + "\n")
        f.write(gen_x2(G_LIB, "sqr_lazy_x2_dev", square=True) + "\n")
        f.write("// Mont(a b + c d) with ONE reduction for inputs < 2M: the column sums take both products\n"
                "// (T < 8M^2 < 1.52 M 2^256, so the result is < 2.51 M) and a subtraction of 2M brings it back\n"
                "// below 2M -- 64 multiply-adds fewer than two products and an addition\n")
        f.write(gen(G_LIB, "mul2_lazy_dev", reduce="2m", pair=True) + "\n")
        f.write("// the canonical value of a Montgomery form a < M: a * 1 / R, i.e. the reduction alone (8 + 64\n"
                "// multiply-adds instead of a full product's 128)\n")
        f.write(gen(G_LIB, "redc_dev", reduce=True, redc=True) + "\n")


# ---------------------------------------------------------------- add / sub / reduce_once
# gfx9 allows one constant-bus read per VALU instruction and the implicit carry-in VCC is one,
# so a borrow chain against the modulus needs it in VGPRs ("v" operands: the compiler keeps
# them in registers across a loop); the masked add-back of sub uses v_and with SGPR moduli.
FIELD_HEADER = """// field_asm.inc -- generated by tools/gen_mac_blocks.py (do not edit): device add / sub /
// conditional subtraction of bn254.hpp as explicit carry chains (v_add_co/v_addc_co,
// v_sub_co/v_subb_co, v_cndmask).  The C forms ((u64) sums and shifts) compile to ~5
// instructions per limb (64-bit adds, sign extensions, moves); these take 2-3.
"""


def gen_field():
    o = []
    for suffix, K in (("", "M"), ("_2m", "M2")):
        o += gen_reduce(suffix, K)
    o += gen_add("", "")
    o += gen_add("2", "_2m")
    o += gen_sub("", "M")
    o += gen_sub("2", "M2")
    return "\n".join(o)


def gen_reduce(suffix, K):
    o = []
    # reduce_once: t = a - K; a = borrow ? a : t
    # t starts as the modulus (tied: no early-clobber output, see gen) and becomes a - K
    o.append("// a - M where a >= M: [0, 2M) -> [0, M)" if K == "M" else
             "// a - 2M where a >= 2M: [0, 4M) -> [0, 2M); 4M itself -> 2M (the closed Fr domain of sumcheck.hip)")
    o.append(f"template <class C>\n__device__ __forceinline__ void reduce_once{suffix}_dev(Fp<C> &a) {{\n  u32 t[8];\n"
             f"#pragma unroll\n  for (int i = 0; i < 8; i++) t[i] = C::{K}[i];")
    body = ["v_sub_co_u32_e32 %0, vcc, %8, %0"]
    body += [f"v_subb_co_u32_e32 %{i}, vcc, %{8 + i}, %{i}, vcc" for i in range(1, 8)]
    body += [f"v_cndmask_b32_e32 %{8 + i}, %{i}, %{8 + i}, vcc" for i in range(8)]
    outs = ", ".join(f'"+v"(t[{i}])' for i in range(8)) + ", " + ", ".join(f'"+v"(a.v[{i}])' for i in range(8))
    o.append('  asm("' + "\\n\\t".join(body) + '"\n      : ' + outs + '\n      :\n      : "vcc");\n}\n')
    return o


def gen_add(name_sfx, red_sfx):
    o = []
    # add: r = a + b, then reduce_once (inputs < K: the sum < 2K < 2^256)
    # in place on r = a (tied: no early-clobber output, see gen)
    o.append("// a + b mod M: a, b in [0, M) -> [0, M)" if name_sfx == "" else
             "// a + b in the lazy domain: a, b in [0, 2M) -> [0, 2M), = a + b mod M; a, b <= 2M -> <= 2M (sumcheck.hip)")
    o.append(f"template <class C>\n__device__ __forceinline__ Fp<C> add{name_sfx}_dev(const Fp<C> &a, const Fp<C> &b) {{\n  Fp<C> r = a;")
    body = ["v_add_co_u32_e32 %0, vcc, %0, %8"]
    body += [f"v_addc_co_u32_e32 %{i}, vcc, %{i}, %{8 + i}, vcc" for i in range(1, 8)]
    outs = ", ".join(f'"+v"(r.v[{i}])' for i in range(8))
    ins = ", ".join(f'"v"(b.v[{i}])' for i in range(8))
    o.append('  asm("' + "\\n\\t".join(body) + '"\n      : ' + outs + "\n      : " + ins + '\n      : "vcc");')
    o.append(f"  reduce_once{red_sfx}_dev(r);\n  return r;\n}}\n")
    return o


def gen_sub(name_sfx, K):
    o = []
    # sub: d = a - b; d += K & -borrow
    # in place on r = a (tied); the borrow mask m and the masked modulus t are written only after the
    # last read of b, so they need no early clobber either (see gen)
    o.append("// a - b mod M: a, b in [0, M) -> [0, M)" if name_sfx == "" else
             "// a - b in the lazy domain: a, b in [0, 2M) -> [0, 2M), = a - b mod M; a, b <= 2M -> <= 2M (sumcheck.hip)")
    o.append(f"template <class C>\n__device__ __forceinline__ Fp<C> sub{name_sfx}_dev(const Fp<C> &a, const Fp<C> &b) {{\n  Fp<C> r = a;\n  u32 m, t[8];")
    body = ["v_sub_co_u32_e32 %0, vcc, %0, %17"]
    body += [f"v_subb_co_u32_e32 %{i}, vcc, %{i}, %{17 + i}, vcc" for i in range(1, 8)]
    body += ["v_cndmask_b32_e64 %8, 0, -1, vcc"]
    body += [f"v_and_b32_e32 %{9 + i}, %{25 + i}, %8" for i in range(8)]
    body += ["v_add_co_u32_e32 %0, vcc, %0, %9"]
    body += [f"v_addc_co_u32_e32 %{i}, vcc, %{i}, %{9 + i}, vcc" for i in range(1, 8)]
    outs = (", ".join(f'"+v"(r.v[{i}])' for i in range(8)) + ', "=v"(m), ' +
            ", ".join(f'"=v"(t[{i}])' for i in range(8)))
    ins = (", ".join(f'"v"(b.v[{i}])' for i in range(8)) +
           ", " + ", ".join(f'"s"(C::{K}[{i}])' for i in range(8)))
    o.append('  asm("' + "\\n\\t".join(body) + '"\n      : ' + outs + "\n      : " + ins + '\n      : "vcc");')
    o.append("  return r;\n}\n")
    return o


if __name__ == "__main__":
    with open("multilinear-map-cryptography_amd/csrc/field_asm.inc", "w") as f:
        f.write(FIELD_HEADER)
        f.write(gen_field())


# ---------------------------------------------------------------- one-block Montgomery product
# The whole product in ONE asm statement on a fixed temporary block v[T .. T+11] (clobbered):
# m0..m7 = v[T..T+7], column accumulators A = v[T+8:T+9], B = v[T+10:T+11] (even-aligned
# pairs, as VOP3 64-bit operands require).  Column k accumulates into P = A|B and its carries
# into the HIGH word of the other pair Q; the column shift is then one move (lo Q = hi P).
# Compared with per-column asm blocks joined by C (acc >> 32 | c2 << 32), this drops the
# compiler's 2-3 moves per column and the wait states it puts at every asm boundary.
def gen_one_block(T, name):
    v = lambda i: f"v{T + i}"
    pair = lambda p: f"v[{T + 8 + 2 * p}:{T + 9 + 2 * p}]"
    lo = lambda p: f"v{T + 8 + 2 * p}"
    hi = lambda p: f"v{T + 9 + 2 * p}"
    A_ = lambda i: f"%{8 + i}"
    B_ = lambda i: f"%{16 + i}"
    M_ = lambda i: f"%{24 + i}"
    INV = "%32"
    body = [f"v_mov_b64 {pair(0)}, 0"]
    for k in range(15):
        P, Q = k & 1, (k & 1) ^ 1
        if k < 8:
            macs = [(A_(i), B_(k - i)) for i in range(k + 1)] + [(v(i), M_(k - i)) for i in range(k)]
        else:
            macs = [(A_(i), B_(k - i)) for i in range(k - 7, 8)] + [(v(i), M_(k - i)) for i in range(k - 7, 8)]
        for j, (x, y) in enumerate(macs):
            body.append(f"v_mad_u64_u32 {pair(P)}, vcc, {x}, {y}, {pair(P)}")
            body.append(f"v_addc_co_u32_e64 {hi(Q)}, vcc, 0, 0, vcc" if j == 0 else
                        f"v_addc_co_u32_e32 {hi(Q)}, vcc, 0, {hi(Q)}, vcc")
        if k < 8:
            body.append(f"v_mul_lo_u32 {v(k)}, {lo(P)}, {INV}")
            body.append(f"v_mad_u64_u32 {pair(P)}, vcc, {v(k)}, {M_(0)}, {pair(P)}")
            body.append(f"v_addc_co_u32_e32 {hi(Q)}, vcc, 0, {hi(Q)}, vcc")
        else:
            body.append(f"v_mov_b32 %{k - 8}, {lo(P)}")
        if k == 14:
            body.append(f"v_mov_b32 %7, {hi(P)}")
        else:
            body.append(f"v_mov_b32 {lo(Q)}, {hi(P)}")
    outs = ", ".join(f'"=&v"(r[{i}])' for i in range(8))
    ins = (", ".join(f'"v"(a.v[{i}])' for i in range(8)) + ", " + ", ".join(f'"v"(b.v[{i}])' for i in range(8)) +
           ", " + ", ".join(f'"s"(C::M[{i}])' for i in range(8)) + ', "s"(C::INV)')
    clob = ", ".join(f'"v{T + i}"' for i in range(12)) + ', "vcc"'
    o = [f"template <class C>\n__device__ __forceinline__ Fp<C> {name}(const Fp<C> &a, const Fp<C> &b) {{",
         "  u32 r[8];",
         '  asm("' + "\\n\\t".join(body) + '"\n      : ' + outs + "\n      : " + ins + "\n      : " + clob + ");",
         "  Fp<C> o;\n#pragma unroll\n  for (int i = 0; i < 8; i++) o.v[i] = r[i];\n  reduce_once(o);\n  return o;\n}\n"]
    return "\n".join(o)


if __name__ == "__main__" and __import__("os").environ.get("TNS_MUL_ONEBLOCK"):
    T = int(__import__("os").environ["TNS_MUL_ONEBLOCK"])
    with open("multilinear-map-cryptography_amd/csrc/mont_mul.inc", "w") as f:
        f.write(LIB_HEADER)
        f.write(gen_one_block(T, "mul_ps_dev") + "\n")
