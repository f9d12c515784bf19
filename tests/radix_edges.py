"""Helpers of tests/test_radix_edges_model.py (CPU) and tests/test_gpu_radix_edges.py (GPU): the radix operators of arithmetic
mode (helm::RadixEngine, helm_amd/csrc/host/shortint_circuit.cpp) at the ends of their block contracts.

  catalogue   operands per operator kind and block count nb (M = 4^nb), each with its Python-integer answer
  decoder     a look-up polynomial (helm_si_make_lut / helm_si_make_many_lut) read back into its entries over one period of
              the plaintext space, and the table families of RadixEngine's constructor restated as functions of v < 16
  scratch     the row consumption of one level (RadixEngine::walk and what it calls: the "take" walk) restated, beside the
              closed form that scratch_rows() used before it became the walk's own dry run

No GPU and no library here: plain integers."""

# helm_radix_kind (include/helm_host.h)
COPY, ADD, SUB, MUL, DIV, SHL, SHR, ADD_SCALAR, SUB_SCALAR, MUL_SCALAR, DIV_SCALAR, SHL_SCALAR, SHR_SCALAR = range(13)
KIND_NAMES = ["copy", "add", "sub", "mul", "div", "shl", "shr", "add_scalar", "sub_scalar", "mul_scalar", "div_scalar",
              "shl_scalar", "shr_scalar"]
SCALAR_KINDS = (ADD_SCALAR, SUB_SCALAR, MUL_SCALAR, DIV_SCALAR, SHL_SCALAR, SHR_SCALAR)
SEAMS = (3, 4, 5, 15, 16, 17, 63, 64)   # both sides of the 4 / 16 / 64-block group seams of carry propagation


# ---------------------------------------------------------------------------------------------------------------------
# catalogue
# ---------------------------------------------------------------------------------------------------------------------
def digits(x, nb):
    return [(x >> (2 * i)) & 3 for i in range(nb)]


def from_digits(d):
    return sum(int(v) << (2 * i) for i, v in enumerate(d))


def rep(digit_pattern, nb):
    """The integer whose blocks repeat `digit_pattern` (least significant first)."""
    return from_digits([digit_pattern[i % len(digit_pattern)] for i in range(nb)])


def answer(kind, nb, a, b):
    """What the operator yields on nb blocks: a, b Python integers (b the scalar of a scalar form, taken as the engine takes
    it: mod 4^nb, a shift amount mod the bit count)."""
    M, bits = 4 ** nb, 2 * nb
    if kind == COPY:
        return a
    if kind in (ADD, ADD_SCALAR):
        return (a + b) % M
    if kind in (SUB, SUB_SCALAR):
        return (a - b) % M
    if kind in (MUL, MUL_SCALAR):
        return (a * b) % M
    if kind in (DIV, DIV_SCALAR):
        return M - 1 if b % M == 0 else a // (b % M)
    if kind in (SHL, SHL_SCALAR):
        return (a << (b % bits)) % M
    if kind in (SHR, SHR_SCALAR):
        return a >> (b % bits)
    raise ValueError(kind)


def seam_pairs(nb):
    """(s, e): a carry generated at block s, propagated through block e - 1, absorbed at block e (e = nb: it leaves the integer)."""
    pts = sorted({p for p in (0,) + SEAMS if p <= nb})
    return [(s, e) for s in pts for e in pts if s < e and s < nb]


def add_chain(nb, s, e):
    """Block sums of a + b: 4 at s (generates), 3 at s + 1 .. e - 1 (propagate), 0 elsewhere (absorb)."""
    a = [0] * nb
    b = [0] * nb
    a[s], b[s] = 3, 1
    for i in range(s + 1, min(e, nb)):
        a[i] = 3
    return from_digits(a), from_digits(b)


def sub_chain(nb, s, e):
    """Block sums of a + ~b + 1 (a_i + 3 - b_i, + 1 at block 0): 4 (5 at block 0) at s, 3 at s + 1 .. e - 1, 2 elsewhere -
    but 3 at block 0 when s > 0, which propagates a carry that never comes."""
    a = [0] * nb
    b = [1] * nb
    a[s], b[s] = 1, 0
    for i in range(s + 1, min(e, nb)):
        a[i] = b[i] = 2
    return from_digits(a), from_digits(b)


def block_sums(kind, nb, a, b):
    """The block sums that propagate() sees for an add / sub (stage 1 of the level)."""
    da, db = digits(a, nb), digits(b % 4 ** nb, nb)
    if kind in (ADD, ADD_SCALAR):
        return [x + y for x, y in zip(da, db)]
    return [x + 3 - y + (1 if i == 0 else 0) for i, (x, y) in enumerate(zip(da, db))]


def catalogue(kind, nb):
    """[(a, b, want)] for one operator kind; b is the second operand or the scalar."""
    M, bits = 4 ** nb, 2 * nb
    x5, xa, x3 = rep([1, 1], nb), rep([2, 2], nb), rep([3, 0], nb)   # 0x55.., 0xAA.., 0x33..
    top = 1 << (bits - 1)
    some = rep([1, 2, 3, 0, 2], nb) | 1
    if kind in (ADD, SUB, ADD_SCALAR, SUB_SCALAR):
        pairs = [(M - 1, 1), (M - 1, M - 1), (x5, xa), (M - 1, 0), (0, 1), (0, M - 1), (some, some)]
        chain = add_chain if kind in (ADD, ADD_SCALAR) else sub_chain
        pairs += [chain(nb, s, e) for s, e in seam_pairs(nb)]
        if kind in SCALAR_KINDS:
            pairs += [(some, 0), (x5, M + 5), (M - 1, M + M - 1)]
    elif kind == MUL:
        pairs = [(M - 1, M - 1), (M - 1, 1), (0, some), (x3, x3), (3 * 4 ** (nb - 1), 3), (some, x5)]
    elif kind == MUL_SCALAR:
        scal = [M - 1, xa, x5, x3, 0, 1, 2, 1 << (bits - 1), 1 << bits, 1 << (bits + 1), M + 7]
        pairs = [(M - 1, s) for s in scal] + [(some, M - 1), (some, x3)]
    elif kind in (SHL, SHR, SHL_SCALAR, SHR_SCALAR):
        amounts = [0, 1, 2, 3, bits - 1, bits, bits + 1]
        if kind in (SHL, SHR):
            amounts = [s for s in amounts if s < M] + [M - 1]
        pairs = [(x, s) for x in (M - 1, 1, top) for s in amounts]
    elif kind in (DIV, DIV_SCALAR):
        pairs = [(some % (M - 1), M - 1), (some, some), (M - 1, 1), (M - 1, 2), (M - 1, 3), (M - 1, M - 1), (M - 1, top),
                 (M - 1, top + 1), (0, some), (some, 0), (top, top), (top - 1, top)]
        pairs = [(a % M, b % M) for a, b in pairs]
    elif kind == COPY:
        pairs = [(M - 1, 0), (some, 0)]
    else:
        raise ValueError(kind)
    out, seen = [], set()
    for a, b in pairs:
        if (a, b) not in seen:
            seen.add((a, b))
            out.append((a, b, answer(kind, nb, a, b)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# table decoder
# ---------------------------------------------------------------------------------------------------------------------
def decode_table(poly, t, delta):
    """helm_si_make_lut's polynomial -> its 2 t entries over one period of the plaintext space, each mod 2 t: entry v < t is the
    box of v read at its first coefficient past the half-box rotation; v in [t, 2 t) is the negacyclic wrap, minus entry v - t."""
    box = len(poly) // t
    low = []
    for v in range(t):
        q, r = divmod(int(poly[v * box]), delta)
        if r:
            raise ValueError("a table coefficient is no multiple of delta")
        low.append(q % (2 * t))
    return low + [(-e) % (2 * t) for e in low]


def decode_many_table(poly, t, delta, n_out):
    """helm_si_make_many_lut's polynomial -> n_out tables over their t / M inputs (M the power of two >= n_out)."""
    M = 1 << max(0, n_out - 1).bit_length()
    per = t // M
    low = decode_table(poly, t, delta)[:t]
    return [low[x * per:(x + 1) * per] for x in range(n_out)]


def _state(v):
    return 2 if v >= 4 else 1 if v == 3 else 0


# RadixEngine's constructor, restated: name -> f(v), v < 16, an entry > 16 meaning entry - 32 (t = 16's own encoding)
_RAW = {"msg": lambda v: v & 3, "carry": lambda v: v >> 2, "resolve": lambda v: 4 if v >= 8 else 0,
            "final": lambda v: ((v & 3) + (1 if (v >> 2) >= 2 else 0)) & 3, "cout": lambda v: 1 if v >= 8 else 0,
            "mul_lo": lambda v: ((v >> 2) * (v & 3)) & 3, "mul_hi": lambda v: ((v >> 2) * (v & 3)) >> 2,
            "mul2_lo": lambda v: (2 * (v >> 2) * (v & 3)) & 3, "mul2_hi": lambda v: (2 * (v >> 2) * (v & 3)) >> 2,
            "bit0": lambda v: v & 1, "bit1": lambda v: (v >> 1) & 1,
            "shl1": lambda v: (((v >> 2) << 1) & 3) | ((v & 3) >> 1), "shr1": lambda v: ((v >> 2) >> 1) | (((v & 3) & 1) << 1),
        "sel": lambda v: (v & 3) if (v >> 2) else 0,
        "q3": lambda v: 0 if v == 15 else 32 - 4, "gc3": lambda v: 32 - 2}
for _p in range(4):
    _RAW["t%d" % _p] = lambda v, p=_p: _state(v) << p
    _RAW["s%d" % _p] = lambda v, p=_p: 0 if v == 15 else 32 - (1 << p)
for _i in range(3):
    _RAW["gc%d" % _i] = lambda v, i=_i: 4 if v >= (2 << i) else 0
    _RAW["q%d" % _i] = lambda v, i=_i: 8 if v >= (2 << i) else 4 if v == (2 << i) - 1 else 0
# the auditor knows a table by its content, and three pairs of the constructor's 30 tables have the same content: they are one
# family here, named after both (resolve/gc2, q3/s2, t2/q1)
FAMILIES = {}
for _name, _f in _RAW.items():
    _same = [n for n, g in FAMILIES.items() if [g(v) for v in range(16)] == [_f(v) for v in range(16)]]
    if _same:
        FAMILIES[_same[0] + "/" + _name] = FAMILIES.pop(_same[0])
    else:
        FAMILIES[_name] = _f
V3_FAMILIES = ("s0", "s1", "q3/s2", "s3", "gc3")   # read on V_3 <= 30: the tables with negative entries


def family_entries(name, t):
    """The 2 t entries helm's add_lut writes for the family: the signed entry below 16, and at t = 32 what the negacyclic
    wrap of t = 16 gave at v in [16, 32) in the table's upper half."""
    sv = [(e - 32 if e > 16 else e) for e in (FAMILIES[name](v) for v in range(16))]
    low = [0] * t
    for v in range(16):
        low[v] = sv[v] % (2 * t)
        if t == 32:
            low[v + 16] = (-sv[v]) % (2 * t)
    return low + [(-e) % (2 * t) for e in low]


def family_of(entries, t):
    """The family whose table this is (by content: the auditor needs no table ids), or None."""
    for name in FAMILIES:
        if family_entries(name, t) == list(entries):
            return name
    return None


def has_negative_entry(entries, t):
    """One of the sixteen entries the layer's t = 16 machine defines is negative (above t as a residue mod 2 t; t itself, the
    weighted state 16 at t = 16, is its own negative and counts as positive)."""
    return any(e > t for e in entries[:16])


# ---------------------------------------------------------------------------------------------------------------------
# scratch restatement: the "take" walk of RadixEngine::walk / propagate / carries / shift_encrypted / divide
# ---------------------------------------------------------------------------------------------------------------------
class Op:
    """What the walk looks at: the kind, the scalar, whether a Mul is a square, and the carry-save forms."""

    def __init__(self, kind, scalar=0, square=False, a2=False, b2=False, out2=False):
        self.kind, self.scalar, self.square, self.a2, self.b2, self.out2 = kind, scalar, square, a2, b2, out2


def prop_rows(W):
    return 5 * W + 16


def carries_take(G, n, need):
    if need <= 0:
        return 0
    if n <= 4:
        return G * need
    ng = (n + 3) // 4
    rows = G * n + G * ng                                   # vbase, sbase
    gneed = n // 4 - 1 if (need == n and n % 4 == 0) else need // 4
    rows += carries_take(G, ng, gneed)
    return rows + G * need                                   # cbase


def propagate_take(G, W, flags):
    """Rows propagate() really takes of the prop_rows(W) * G it is given."""
    if G == 0:
        return 0
    need = W if flags else W - 1
    return G * W + carries_take(G, W, need)


def reduce_terms(nb, terms):
    """The term-reduction loop of the walk on one operator's terms [(low, maxv)] -> (vectors taken, rounds, largest group sum,
    final terms)."""
    vectors = rounds = top = 0
    T = 5
    while len(terms) > 2 or sum(m for _, m in terms) > 6:
        rounds += 1
        terms = sorted(terms, key=lambda x: x[0])            # std::sort on low; the bounds of equal lows are what counts
        nxt, q = [], 0
        while q < len(terms):
            e, s = q, 0
            while e < len(terms) and e - q < T and s + terms[e][1] <= 15:
                s += terms[e][1]
                e += 1
            if e - q == 1 and s <= 3:
                nxt.append(terms[q])
                q = e
                continue
            if e == q:
                raise ValueError("a term bounded above 15 cannot be reduced")
            top = max(top, s)
            low = terms[q][0]
            vectors += 1
            nxt.append((low, 3))
            if low + 1 < nb:
                vectors += 1
                nxt.append((low + 1, 3))
            q = e
        terms = nxt
    return vectors, rounds, top, terms


def op_terms(nb, op):
    """-> (vectors taken for the terms, [(low, maxv)]) of a multiplication or a carry-save sum, or None."""
    M = 4 ** nb
    if op.kind == MUL_SCALAR:
        s = op.scalar % M
        if s >= 2 and s & (s - 1) == 0:
            return None                                       # a power of two is a shift
        t = [(j, 3 * ((s >> (2 * j)) & 3)) for j in range(nb) if (s >> (2 * j)) & 3]
        return len(t), t
    if op.kind == MUL and op.square:
        t, v = [], 0
        for j in range((nb + 1) // 2):
            t.append((2 * j, 3))
            v += 1
            if 2 * j + 1 < nb:
                t.append((2 * j + 1, 4))
                v += 1
        return v, t
    if op.kind == MUL:
        t, v = [], 0
        for j in range(nb):
            t.append((j, 3))
            v += 1
            if j + 1 < nb:
                t.append((j + 1, 3))
                v += 1
        return v, t
    if op.kind in (ADD, SUB) and (op.a2 or op.b2 or op.out2):
        t = [(0, 3)] + ([(0, 3)] if op.a2 else [])
        if op.kind == ADD:
            return 0, t + [(0, 3)] + ([(0, 3)] if op.b2 else [])
        nc = 2 if op.b2 else 1
        return nc, t + [(0, 3 + nc)] + ([(0, 3)] if nc == 2 else [])
    return None


def level_take(nb, ops):
    """One level -> (rows the walk takes = what scratch_rows() declares, rows really written, largest term-group sum)."""
    rows = props = top = 0
    M = 4 ** nb
    for op in ops:
        plain = op.kind in (ADD, SUB, ADD_SCALAR, SUB_SCALAR) and not (op.a2 or op.b2 or op.out2)
        if plain:
            props += 1
            continue
        got = op_terms(nb, op)
        if got is None:
            continue
        v, terms = got
        v2, _, s, final = reduce_terms(nb, terms)
        rows += (v + v2) * nb
        top = max(top, s)
        if not op.out2 and sum(m for _, m in final) > 3:
            props += 1
    used = rows + propagate_take(props, nb, False)
    rows += prop_rows(nb) * props
    sh = sum(1 for op in ops if op.kind in (SHL, SHR))
    if sh:
        nbits = 0
        while (1 << nbits) < 2 * nb:
            nbits += 1
        rows += sh * nbits + 4 * sh * nb
        used += sh * nbits + 4 * sh * nb
    dv = sum(1 for op in ops if op.kind in (DIV, DIV_SCALAR))
    if dv:
        W, bits = nb + 1, 2 * nb
        rows += 2 * dv * bits + 5 * dv * W
        used += 2 * dv * bits + 5 * dv * W + propagate_take(dv, W, True)
        rows += prop_rows(W) * dv
    return rows, used, top


def closed_form_rows(nb, ops):
    """scratch_rows() as it was before it ran the walk: a closed form per operator (kept to show what it missed)."""
    rows = 0
    for op in ops:
        rows += prop_rows(nb)
        if op.kind in (MUL, MUL_SCALAR):
            rows += (4 * nb + 4) * nb
        if op.kind in (ADD_SCALAR, SUB_SCALAR):
            rows += nb
        if op.a2 or op.b2 or (op.kind in (ADD, SUB) and op.out2):
            rows += 6 * nb
        if op.kind in (SHL, SHR):
            rows += 4 * nb + 8
        if op.kind in (DIV, DIV_SCALAR):
            rows += 4 * 2 * nb + 5 * (nb + 1) + prop_rows(nb + 1)
    return rows


def scalar_patterns(nb):
    """The structured scalar digit patterns: all 3, all 2, all 1, alternating 3 / 0 and 0 / 3, one digit, the mixed 3 / 2 / 1."""
    return {"all3": rep([3], nb), "all2": rep([2], nb), "all1": rep([1], nb), "alt30": rep([3, 0], nb), "alt03": rep([0, 3], nb),
            "top3": 3 * 4 ** (nb - 1), "mix321": rep([3, 2, 1], nb), "mix3312": rep([3, 3, 1, 2], nb), "three": 3, "zero": 0, "one": 1}
