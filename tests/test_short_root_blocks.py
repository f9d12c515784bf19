"""The 8-point block form of the N = 512 transforms (ntt_fp64.h: fwd_blk8 / inv_blk8 / mul_broot), CPU only.

In Geo<9> each register block is three radix-2 stages on the eight values of one lane, and those eight values are one
8-group of the negacyclic transform: the block evaluates sum_e x_e y^e at the eight roots y = w z, where w is the
group's root (the twiddle of the block's last stage for hi = 0) and z runs over the eighth roots of unity
{+-1, +-b^2, +-b, +-b^3} of a field p = b^4 + 1.  So a block is a diagonal of seven general twiddles w^t followed by a
DFT8 whose five nontrivial multiplications are by powers of b (mul_broot: 4 operations instead of mulmod's 6), and the
inverse block is the DFT8 over b^-k followed by the diagonal w^-t.

Part 1 restates both forms in exact integers - mulmod and mul_broot with their rounded quotients computed in doubles,
as the kernels do - and checks that they give the same residues as the radix-2 stages for every lane of every block,
on random and on extreme inputs, and through whole transforms.
Part 2 is the interval bound of a CMUX step of the lockstep kernel in the field the block form is enabled for (FpG),
in the style of tests/test_lazy_bounds.py: every addition and every mulmod / mul_broot input stays below 2^53, and the
recentrings of ntt_inverse's LEAN form (slot 0 alone at each transpose) follow from it.
"""
import random

import pytest

LIMIT = 2.0 ** 53
LOGN, N, E = 9, 512, 8
FIELDS = {"FpG": (5072, 3)}   # (b, generator): the fields the block form is enabled for (ntt_fp64.h: blk8_field)


# ---- exact arithmetic as the kernels perform it ------------------------------------------------------------------
def rint(v):
    return int(round(v))      # round half to even, as v_rndne_f64


def mulmod(a, w, p):
    """ntt_fp64.h mulmod: h = fl(a w), l = a w - h (exact), q = rint(h / p), r = (h - q p) + l = a w - q p"""
    assert abs(a) < LIMIT and abs(w) <= p // 2
    h = float(a) * float(w)
    q = rint(h * (1.0 / p))
    r = a * w - q * p
    assert abs(r) < LIMIT
    return r


def mul_broot(x, k, b):
    """x b^k mod p (k = 1..7, k != 4): x = q b^(4-j) + x0 with j = k mod 4, then x b^j = x0 b^j - q (b^4 = -1)"""
    assert abs(x) < LIMIT and k in (1, 2, 3, 5, 6, 7)
    j = k & 3
    bc, bk = b ** (4 - j), b ** j
    q = rint(float(x) * (1.0 / bc))
    x0 = x - q * bc                      # fma(-q, b^(4-j), x): exact
    assert abs(x0) < LIMIT
    r = x0 * bk - q if k < 4 else q - x0 * bk
    assert abs(r) < LIMIT
    return r


def brev(i):
    return int(format(i, "09b")[::-1], 2)


def centred(v, p):
    v %= p
    return v - p if v > p // 2 else v


def tables(b, gen):
    """helm_hip's host tables: psi a primitive 2N-th root with psi^(N/4) = b, tf[brev(i)] = psi^i, ti[brev(i)] = psi^-i"""
    p = b ** 4 + 1
    psi = pow(gen, (p - 1) // (2 * N), p)
    psi = pow(psi, next(t for t in range(1, 8, 2) if pow(psi, t * N // 4, p) == b), p)
    tf, ti = [0] * N, [0] * N
    for i in range(N):
        tf[brev(i)] = centred(pow(psi, i, p), p)
        ti[brev(i)] = centred(pow(psi, -i, p), p)
    assert tf[1] == b * b and tf[2] == b and tf[3] == b ** 3
    return p, psi, tf, ti


def tw_pow(tf, x):
    """psi^x from the forward table (psi^N = -1): ntt_fp64.h tw_pow"""
    x %= 2 * N
    v = tf[brev(x % N)]
    return -v if x >= N else v


# ---- layouts (ntt_fp64.h Geo<9>) -----------------------------------------------------------------------------------
def jA(lane, e):
    return (e << 6) | lane


def jB(lane, e):
    return ((lane >> 3) << 6) | (e << 3) | (lane & 7)


def jC(lane, e):
    return (lane << 3) | e


BLOCKS = {"A": (jA, 6), "B": (jB, 3), "C": (jC, 0)}   # layout, lowest stride bit of the block


def omega_exp(block, lane):
    """exponent a (w = psi^a) of the lane's group root: the block's last stage's twiddle for hi = 0"""
    j, s = BLOCKS[block]
    return brev((N >> (s + 1)) + (j(lane, 0) >> (s + 1)))


# ---- radix-2 stages (fwd_block / inv_block) ------------------------------------------------------------------------
def fwd_radix2(x, tf, p, block, lane):
    j, s = BLOCKS[block]
    x = list(x)
    for sb in (s + 2, s + 1, s):
        eb = sb - s
        for e0 in range(8):
            if (e0 >> eb) & 1:
                continue
            e1 = e0 | (1 << eb)
            w = tf[(N >> (sb + 1)) + (j(lane, e0) >> (sb + 1))]
            u, v = x[e0], mulmod(x[e1], w, p)
            x[e0], x[e1] = u + v, u - v
    return x


def inv_radix2(x, ti, p, block, lane):
    j, s = BLOCKS[block]
    x = list(x)
    for sb in (s, s + 1, s + 2):
        eb = sb - s
        for e0 in range(8):
            if (e0 >> eb) & 1:
                continue
            e1 = e0 | (1 << eb)
            w = ti[(N >> (sb + 1)) + (j(lane, e0) >> (sb + 1))]
            u, v = x[e0], x[e1]
            x[e0], x[e1] = u + v, mulmod(u - v, w, p)
    return x


# ---- the block form -------------------------------------------------------------------------------------------------
# stage 3 of the DFT8 (slot bit 0): pair (2q, 2q + 1) multiplies by z_q = 1, b^2, b, b^3 -> mul_broot k = -, 2, 1, 3;
# the inverse by z_q^-1 = 1, b^6, b^7, b^5.  Stage 2 (slot bit 1): pairs (4, 6), (5, 7) by b^2 (inverse b^6).
FWD_K3, INV_K3 = (0, 2, 1, 3), (0, 6, 7, 5)


def dft8(z, b):
    a = [0] * 8
    for e in range(4):
        a[e], a[e + 4] = z[e] + z[e + 4], z[e] - z[e + 4]
    c = list(a)
    for e in (0, 1):
        c[e], c[e + 2] = a[e] + a[e + 2], a[e] - a[e + 2]
    for e in (4, 5):
        t = mul_broot(a[e + 2], 2, b)
        c[e], c[e + 2] = a[e] + t, a[e] - t
    y = list(c)
    for q in range(4):
        t = c[2 * q + 1] if q == 0 else mul_broot(c[2 * q + 1], FWD_K3[q], b)
        y[2 * q], y[2 * q + 1] = c[2 * q] + t, c[2 * q] - t
    return y


def idft8(y, b):
    c = list(y)
    for q in range(4):
        u, v = y[2 * q], y[2 * q + 1]
        c[2 * q] = u + v
        c[2 * q + 1] = u - v if q == 0 else mul_broot(u - v, INV_K3[q], b)
    a = list(c)
    for e in (0, 1):
        a[e], a[e + 2] = c[e] + c[e + 2], c[e] - c[e + 2]
    for e in (4, 5):
        a[e], a[e + 2] = c[e] + c[e + 2], mul_broot(c[e] - c[e + 2], 6, b)
    z = list(a)
    for e in range(4):
        z[e], z[e + 4] = a[e] + a[e + 4], a[e] - a[e + 4]
    return z


def fwd_blk8(x, tf, p, b, block, lane):
    a = omega_exp(block, lane)
    return dft8([x[0]] + [mulmod(x[t], tw_pow(tf, t * a), p) for t in range(1, 8)], b)


def inv_blk8(x, tf, p, b, block, lane):
    a = omega_exp(block, lane)
    z = idft8(x, b)
    return [z[0]] + [mulmod(z[t], tw_pow(tf, -t * a), p) for t in range(1, 8)]


# inverse block A (stride bits 6 .. 8): its last two stages' twiddles ti[1], ti[2 + hi] are b^6 and b^7, b^5
INV_A_K = {7: (7, 5), 8: (6,)}


def inv_blockA_short(x, ti, p, b, lane):
    x = list(x)
    for sb in (6, 7, 8):
        eb = sb - 6
        for e0 in range(8):
            if (e0 >> eb) & 1:
                continue
            e1 = e0 | (1 << eb)
            u, v = x[e0], x[e1]
            x[e0] = u + v
            if sb == 6:
                x[e1] = mulmod(u - v, ti[(N >> 7) + (jA(lane, e0) >> 7)], p)
            else:
                x[e1] = mul_broot(u - v, INV_A_K[sb][e0 >> (eb + 1)], b)
    return x


def _inputs(rnd, p, kind, big):
    half = p // 2
    if kind == "random":
        return [rnd.randint(-half, half) for _ in range(8)]
    if kind == "half":
        return [rnd.choice((-half, half)) for _ in range(8)]
    # the lazy maxima: the largest block input of part 2's bounds, either sign
    return [rnd.choice((-big, big, -half, half)) for _ in range(8)]


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_short_root_constants(field):
    b, gen = FIELDS[field]
    p, psi, tf, ti = tables(b, gen)
    assert pow(b, 4, p) == p - 1
    assert (ti[1] - b ** 6) % p == 0 and (ti[2] - b ** 7) % p == 0 and (ti[3] - b ** 5) % p == 0
    for k in (1, 2, 3, 5, 6, 7):
        for x in (0, 1, -1, p // 2, -(p // 2), 2 ** 53 - 1, -(2 ** 53 - 1), 123456789012345):
            r = mul_broot(x, k, b)
            assert (r - x * b ** k) % p == 0
            assert abs(r) <= p // 2 + abs(x) // b ** (4 - (k & 3)) + 2      # close to recentred


@pytest.mark.parametrize("field", sorted(FIELDS))
@pytest.mark.parametrize("kind", ["random", "half", "lazy"])
def test_blocks_equal_radix2_stages_for_every_lane(field, kind):
    b, gen = FIELDS[field]
    p, psi, tf, ti = tables(b, gen)
    rnd = random.Random(f"{field}:{kind}")
    for block in ("B", "C"):
        for lane in range(64):
            for _ in range(3):
                x = _inputs(rnd, p, kind, int(4.5 * p))   # forward block inputs: <= 4.4 p (block B's pure-sum class)
                want = fwd_radix2(x, tf, p, block, lane)
                got = fwd_blk8(x, tf, p, b, block, lane)
                assert all((g - w) % p == 0 for g, w in zip(got, want)), (block, lane)
                x = _inputs(rnd, p, kind, p)              # inverse block inputs: <= 0.95 p (LEAN8)
                want = inv_radix2(x, ti, p, block, lane)
                got = inv_blk8(x, tf, p, b, block, lane)
                assert all((g - w) % p == 0 for g, w in zip(got, want)), ("inverse", block, lane)
    for lane in range(64):
        x = _inputs(rnd, p, kind, p)
        want = inv_radix2(x, ti, p, "A", lane)
        got = inv_blockA_short(x, ti, p, b, lane)
        assert all((g - w) % p == 0 for g, w in zip(got, want)), ("inverse A", lane)


def _transform(X, blocks):
    X = list(X)
    for name, fn in blocks:
        j, _ = BLOCKS[name]
        for lane in range(64):
            idx = [j(lane, e) for e in range(8)]
            out = fn([X[i] for i in idx], name, lane)
            for i, v in zip(idx, out):
                X[i] = v
    return X


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_whole_transforms_agree_and_invert(field):
    """ntt_forward (block A radix-2, B and C in block form) and ntt_inverse (C, B in block form, A with short-root
    stages) against the all-radix-2 transforms, and inverse(forward(x)) = N x"""
    b, gen = FIELDS[field]
    p, psi, tf, ti = tables(b, gen)
    rnd = random.Random(9)
    X = [rnd.randint(-32, 31) for _ in range(N)]
    r2f = lambda x, blk, lane: fwd_radix2(x, tf, p, blk, lane)
    new_f = lambda x, blk, lane: r2f(x, blk, lane) if blk == "A" else fwd_blk8(x, tf, p, b, blk, lane)
    old = _transform(X, [("A", r2f), ("B", r2f), ("C", r2f)])
    new = _transform(X, [("A", r2f), ("B", new_f), ("C", new_f)])
    assert all((u - v) % p == 0 for u, v in zip(old, new))
    Y = [centred(v, p) for v in new]
    r2i = lambda x, blk, lane: inv_radix2(x, ti, p, blk, lane)
    new_i = lambda x, blk, lane: inv_blockA_short(x, ti, p, b, lane) if blk == "A" else inv_blk8(x, tf, p, b, blk, lane)
    old_i = _transform(Y, [("C", r2i), ("B", r2i), ("A", r2i)])
    new_i = _transform(Y, [("C", new_i), ("B", new_i), ("A", new_i)])
    assert all((u - v) % p == 0 and (v - N * x) % p == 0 for u, v, x in zip(old_i, new_i, X))


# ---- part 2: interval bounds of a CMUX step -----------------------------------------------------------------------
def mulmod_bound(a, p):
    assert a < LIMIT, "mulmod input not exact"
    return (0.5 + 0.75 * a / 2.0 ** 52) * p


def mul_broot_bound(x, k, b):
    assert x < LIMIT, "mul_broot input not exact"
    j = k & 3
    return (b ** 4) / 2 + x * (b ** j * 2.0 ** -52 + 1.0 / b ** (4 - j)) + 1


def _add(u, v, peak):
    s = u + v
    assert s < LIMIT, "sum not exact"
    peak[0] = max(peak[0], s)
    return s


def fwd_blk8_bound(m, p, b, peak, x0_recentred=False):
    z = [p / 2 + 2 if x0_recentred else m[0]] + [mulmod_bound(m[t], p) for t in range(1, 8)]
    a = [0.0] * 8
    for e in range(4):
        a[e] = a[e + 4] = _add(z[e], z[e + 4], peak)
    c = list(a)
    for e in (0, 1):
        c[e] = c[e + 2] = _add(a[e], a[e + 2], peak)
    for e in (4, 5):
        c[e] = c[e + 2] = _add(a[e], mul_broot_bound(a[e + 2], 2, b), peak)
    y = list(c)
    for q in range(4):
        t = c[2 * q + 1] if q == 0 else mul_broot_bound(c[2 * q + 1], FWD_K3[q], b)
        y[2 * q] = y[2 * q + 1] = _add(c[2 * q], t, peak)
    return y


def inv_blk8_bound(m, p, b, peak):
    c = list(m)
    for q in range(4):
        s = _add(m[2 * q], m[2 * q + 1], peak)
        c[2 * q] = s
        c[2 * q + 1] = s if q == 0 else mul_broot_bound(s, INV_K3[q], b)
    a = list(c)
    for e in (0, 1):
        a[e] = a[e + 2] = _add(c[e], c[e + 2], peak)
    for e in (4, 5):
        s = _add(c[e], c[e + 2], peak)
        a[e], a[e + 2] = s, mul_broot_bound(s, 6, b)
    z = list(a)
    for e in range(4):
        z[e] = z[e + 4] = _add(a[e], a[e + 4], peak)
    return [z[0]] + [mulmod_bound(z[t], p) for t in range(1, 8)]


def inv_blockA_bound(m, p, b, peak):
    x = list(m)
    for eb in range(3):
        new = list(x)
        for e0 in range(8):
            if (e0 >> eb) & 1:
                continue
            e1 = e0 | (1 << eb)
            s = _add(x[e0], x[e1], peak)
            new[e0], new[e1] = s, mulmod_bound(s, p) if eb == 0 else mul_broot_bound(s, 5, b)
        x = new
    return x


def transpose(m, recentre, half):
    """a transpose hands a lane the eight values of ONE slot class of the block before: the next block's inputs are
    bounded by the largest class left unreduced"""
    return [max(half if e in recentre else m[e] for e in range(8))] * 8


# the recentrings ntt_inverse's LEAN form keeps with the block form: slot 0 (the pure sum) at each transpose
LEAN8_RECENTRE = (0,)


@pytest.mark.parametrize("name,field,k,l,logB", [
    ("boolean_default", "FpG", 2, 3, 6),
    ("k = 2, l = 3 with the largest digits the lazy field takes (logB 12)", "FpG", 2, 3, 12),
    ("k = 1, l = 3", "FpG", 1, 3, 12),
    ("largest digits the lazy field is chosen for", "FpG", 1, 2, 12),
])
def test_cmux_step_bounds_with_block_form(name, field, k, l, logB):
    b, _ = FIELDS[field]
    p = b ** 4 + 1
    half = p / 2 + 2
    peak = [0.0]
    # block A: fwd_top2_digits on digits, then one Cooley-Tukey stage (stride bit 6)
    d = 2.0 ** (logB - 1)
    top2 = d * (1 + b * b) + d * (b + b ** 3)
    mA = _add(top2, mulmod_bound(top2, p), peak)
    # blocks B and C in block form, no recentring at the transposes (lazy field); block C recentres its one input that
    # no diagonal twiddle multiplies (x0): otherwise the pure-sum class of block B (4.4 p) would pass into every output
    mB = fwd_blk8_bound([mA] * 8, p, b, peak)
    mC = fwd_blk8_bound(transpose(mB, (), half), p, b, peak, x0_recentred=True)
    out = max(mC)
    prod = mulmod_bound(out, p)
    column = (k + 1) * l * prod          # all (k+1) l products of a column summed raw
    assert column < LIMIT, (name, column / p)
    # the inverse from recentred column sums
    m1 = inv_blk8_bound([half] * 8, p, b, peak)
    m2 = inv_blk8_bound(transpose(m1, LEAN8_RECENTRE, half), p, b, peak)
    m3 = inv_blockA_bound(transpose(m2, LEAN8_RECENTRE, half), p, b, peak)
    assert max(m3) < LIMIT                # the final recentring's input
    print(f"\n{name} [{field}]: forward <= {out / p:.2f} p, product <= {prod / p:.2f} p, column sum <= {column / p:.2f} p, "
          f"inverse classes {max(m1[1:]) / p:.2f} / {max(m2[1:]) / p:.2f} p, final <= {max(m3) / p:.2f} p, "
          f"largest sum {peak[0] / p:.2f} p of 2^53 = {LIMIT / p:.2f} p")
    if logB == 6:
        # the figures ntt_fp64.h and DESIGN.md 4.2 quote for the flagship set
        assert out / p < 7.4 and column / p < 11.9 and max(m3) / p < 10.7


def test_lean8_recentring_is_needed_and_sufficient():
    """with slot 0 recentred at both transposes the inverse stays exact; leaving slot 0 unreduced would not"""
    b, _ = FIELDS["FpG"]
    p = b ** 4 + 1
    half = p / 2 + 2
    m1 = inv_blk8_bound([half] * 8, p, b, [0.0])
    assert m1[0] / p > 3.9 and max(m1[1:]) / p < 0.95     # pure sum 8 x p/2; every other slot a fresh product
    with pytest.raises(AssertionError):
        m2 = inv_blk8_bound(transpose(m1, (), half), p, b, [0.0])
        inv_blockA_bound(transpose(m2, (), half), p, b, [0.0])
