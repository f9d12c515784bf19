"""The radix operators of arithmetic mode (helm::RadixEngine) at the ends of their block contracts, audited per look-up.

tests/radix_edges.py's catalogue goes through helm_host_radix_level_ex, every pair of a case in ONE level, on si_toy_512
(t = 16) - also with HELM_RADIX_MANY_LUT - and on si_toy_4096 under SiServerKey(generic="large") (t = 32, where the negacyclic
table families are written into the table's upper half).  For every case:

  values   every result equals the Python integer and every result block decrypts below 4
  audit    (SiServerKey.set_audit) for every look-up of every batch: the input's value v = round(phase / delta) mod 2 t is
           <= 15, or <= 30 where the table has a negative entry; the table is decoded from the record's own polynomial; the
           output decrypts to table(v) under the padding-bit rule; |phase - v delta| / (delta / 2) is recorded per family;
           every linear step is recomputed exactly; a term-reduction sum (the five-term linear steps) is <= 15
  reach    asserted from what the audit saw: state tables read at 7 (block 0) and 6, V_3 tables at 30 and at v >= 16 under both
           encodings, lut_s_ at all four weights, packed product operands of 15, lut_sel_ at 7, every family read
  scratch  the table is a bystander integer + the integers + helm_host_radix_scratch_rows() + a guard band of fresh
           encryptions: bystander and guard are word for word what was uploaded

Whole circuits (ArithCircuit.evaluate_encrypted: the carry-save forms a2 / b2 / out2 and the lanes) and one u8 case at the
full-size shortint_m2c2, which writes down the measured margin per family, follow."""
import ctypes as C
import os
import sys
import threading
import time
from collections import defaultdict

import numpy as np
import pytest

import helm_amd
from helm_amd import ArithCircuit, Circuit, PtxtType, verilog_parser
from helm_amd import _host as H

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radix_edges as E  # noqa: E402

pytestmark = pytest.mark.gpu
MANY_LUT = 1


class Op(C.Structure):   # helm_radix_op
    _fields_ = [("kind", C.c_int32), ("a", C.c_int32), ("b", C.c_int32), ("out", C.c_int32),
                ("scalar_lo", C.c_uint64), ("scalar_hi", C.c_uint64)]


# ---- keys: one pair per encoding for the whole file ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy16():
    ck, sk = helm_amd.gen_keys_shortint("si_toy_512", seed=5)
    assert ck.t == 16
    yield ck, sk
    sk.close()


@pytest.fixture(scope="module")
def toy32():
    p, lwe_std, glwe_std = helm_amd.si_named_params("si_toy_4096")   # the keys of tests/test_gpu_large_n.py
    p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = 1, 22, 3, 5
    ck = helm_amd.SiClientKey(p, lwe_std, glwe_std, seed=7)
    sk = helm_amd.SiServerKey(ck, generic="large")
    assert ck.t == 32 and sk.kernel_class() == "large"
    yield ck, sk
    sk.close()


@pytest.fixture
def enc(request, toy16, toy32):
    return toy16 if request.param == 16 else toy32


# ---- the audit --------------------------------------------------------------------------------------------------------------
class RadixAudit:
    """fn for SiServerKey.set_audit: every look-up against the table decoded from its own record, every linear step exactly."""

    def __init__(self, ck):
        self.ck, self.t, self.delta = ck, ck.t, ck.delta
        self.lock = threading.Lock()
        self.reads = defaultdict(set)     # family -> input values read
        self.first = defaultdict(set)     # the same, first look-up batch after reset_level() only (round 1 of a propagation)
        self.margin = defaultdict(float)  # family -> largest |phase - v delta| / (delta / 2) of an input
        self.bad = []
        self.luts = self.lin = self.lut_batches = self.max_sum = 0
        self.pair_rows = self.pair_states = 0   # rotations with a two-function table, and their second outputs checked
        self.tables = {}

    def reset_level(self):
        self.lut_batches = 0

    def values(self, rows):
        ph = self.ck.phase(rows)
        d = np.uint64(self.delta)
        with np.errstate(over="ignore"):
            v = (ph + np.uint64(self.delta // 2)) // d          # 2 t delta = 2^64: the wrap is the reduction mod 2 t
            err = (ph - v * d).view(np.int64)
        return v.astype(np.int64) % (2 * self.t), np.abs(err) / (self.delta / 2)

    def table(self, poly):
        ent = tuple(E.decode_table(poly, self.t, self.delta))
        if ent not in self.tables:
            self.tables[ent] = E.family_of(ent, self.t) or "unknown"
        return self.tables[ent], ent

    def __call__(self, rec):
        with self.lock:
            if rec["kind"] == "lincomb":
                self.lincomb(rec)
            elif rec["kind"] == "luts":
                self.look_ups(rec)
            else:
                self.pairs(rec)
        return True

    def lincomb(self, rec):
        cnt, terms, _ = rec["in_rows"].shape
        acc = np.zeros_like(rec["out_rows"])
        with np.errstate(over="ignore"):
            for t in range(terms):
                use = rec["in_idx"][:, t] >= 0
                acc[use] += rec["coef"][use, t].astype(np.uint64)[:, None] * rec["in_rows"][use, t]
            if rec["const_add"] is not None:
                acc[:, -1] += rec["const_add"].astype(np.uint64) * np.uint64(self.delta)
        ok = np.all(acc == rec["out_rows"], axis=1)
        self.lin += cnt
        self.bad += [("lincomb", int(g)) for g in np.nonzero(~ok)[0]]
        if terms == 5:   # a term-reduction sum: its bound is the grouping rule's 15
            v, _ = self.values(rec["out_rows"])
            self.max_sum = max(self.max_sum, int(v.max()))
            self.bad += [("term sum", int(g), int(v[g])) for g in np.nonzero(v > 15)[0]]

    def look_ups(self, rec):
        first = self.lut_batches == 0
        self.lut_batches += 1
        vin, margin = self.values(rec["in_rows"])
        vout, _ = self.values(rec["out_rows"])
        self.luts += len(vin)
        for li in np.unique(rec["lut_idx"]):
            fam, ent = self.table(rec["luts"][li])
            sel = rec["lut_idx"] == li
            v, o = vin[sel], vout[sel]
            bound = 30 if E.has_negative_entry(ent, self.t) else 15
            want = np.array(ent, dtype=np.int64)[v]
            for g in np.nonzero((v > bound) | (o != want))[0]:
                self.bad.append(("luts", fam, int(v[g]), int(o[g]), int(want[g])))
            self.reads[fam] |= {int(x) for x in np.unique(v)}
            if first:
                self.first[fam] |= {int(x) for x in np.unique(v)}
            self.margin[fam] = max(self.margin[fam], float(margin[sel].max()))

    def pairs(self, rec):
        first = self.lut_batches == 0
        self.lut_batches += 1
        vin, margin = self.values(rec["in_rows"])
        self.luts += len(vin)
        n_out = rec["n_out"]
        one = {}
        for li in np.unique(rec["lut_idx"]):
            poly = rec["luts"][li]
            tabs = E.decode_many_table(poly, self.t, self.delta, n_out)
            p = [q for q in range(4) if tabs[1] == [E._RAW["t%d" % q](v) for v in range(self.t // 2)]]
            if tabs[0] == [v & 3 for v in range(self.t // 2)] and len(p) == 1:   # a two-function table: message, weighted state
                one[li] = ("pair%d" % p[0], tabs, self.t // 2 - 1)
            else:                                              # a plain look-up riding in a pair launch
                fam, ent = self.table(poly)
                one[li] = (fam, [list(ent)], 30 if E.has_negative_entry(ent, self.t) else 15)
        for g in range(len(vin)):
            fam, tabs, bound = one[rec["lut_idx"][g]]
            v = int(vin[g])
            self.reads[fam].add(v)
            if first:
                self.first[fam].add(v)
            self.margin[fam] = max(self.margin[fam], float(margin[g]))
            if v > bound:
                self.bad.append(("many_luts", fam, v))
                continue
            self.pair_rows += len(tabs) > 1
            for x in range(min(n_out, len(tabs))):
                got = rec["out_rows"][g, x]
                # the record carries no output rows' indices: a skipped output is known by its all-zero result row (a written
                # ciphertext has a random mask), so a state wrongly left out would pass HERE - the tests that run pair launches
                # therefore count the states checked against the ones the propagation needs (pair_states)
                if not got.any():
                    continue
                self.pair_states += x == 1
                o = int(self.values(got[None, :])[0][0])
                if o != tabs[x][v] % (2 * self.t):
                    self.bad.append(("many_luts", fam, x, v, o, tabs[x][v]))


# ---- one level through the C entry point ---------------------------------------------------------------------------------------
def _blocks(x, nb):
    return np.array(E.digits(x, nb), dtype=np.uint64)


def _cost(kind, nb):
    """Rows of an operator's largest look-up batch, roughly: the audit copies every batch's operand and result rows to the
    host, so what a level may hold is bounded (rounds cost nothing here: a division's batches are small)."""
    if kind in (E.MUL, E.MUL_SCALAR):
        return 2 * nb * nb
    return 3 * (nb + 1)


def run_level(ck, sk, nb, ops, flags=0, audit=None):
    """ops: [(kind, a, b)] or [(kind, a, b, True)] for a Mul whose two operands are the SAME rows (a square) -> values.
    Table: bystander | a, b, out of every operator | scratch | guard; bystander and guard must come back untouched."""
    n = len(ops)
    cops = (Op * n)()
    for i, op in enumerate(ops):
        kind, a, b = op[0], op[1], op[2]
        base = (1 + 3 * i) * nb
        if kind in E.SCALAR_KINDS or kind == E.COPY:
            cops[i] = Op(kind, base, -1, base + 2 * nb, b & (2 ** 64 - 1), (b >> 64) & (2 ** 64 - 1))
        else:
            cops[i] = Op(kind, base, base if len(op) > 3 and op[3] else base + nb, base + 2 * nb, 0, 0)
    scratch = int(H.host.helm_host_radix_scratch_rows(sk._h, nb, C.cast(cops, C.c_void_p), n))
    # the budget is the level's own walk: every level run here pins the C++ walk to its restatement, whatever it holds
    model = [E.Op(op[0], op[2] & (2 ** 128 - 1) if op[0] in E.SCALAR_KINDS else 0, square=len(op) > 3 and bool(op[3])) for op in ops]
    assert scratch == E.level_take(nb, model)[0], (nb, [E.KIND_NAMES[op[0]] for op in ops], scratch, E.level_take(nb, model))
    ints, guard = (1 + 3 * n) * nb, 16 * nb + 8   # wider than any overrun the closed-form budget allowed (933 rows at 64 blocks)
    w = sk.wires(ints + scratch + guard)
    by = ck.encrypt(_blocks(E.rep([2, 1, 3], nb), nb))
    gd = ck.encrypt(np.arange(guard, dtype=np.uint64) % 4)
    w.upload(np.arange(nb), by)
    w.upload(np.arange(ints + scratch, ints + scratch + guard), gd)
    for i, op in enumerate(ops):
        base = (1 + 3 * i) * nb
        w.upload(np.arange(base, base + nb), ck.encrypt(_blocks(op[1], nb)))
        if not (op[0] in E.SCALAR_KINDS or op[0] == E.COPY):
            w.upload(np.arange(base + nb, base + 2 * nb), ck.encrypt(_blocks(op[2], nb)))
    pbs, rounds = C.c_int64(), C.c_int64()
    if audit is not None:
        audit.reset_level()
        sk.set_audit(audit)
    try:
        H.check(H.host.helm_host_radix_level_ex(sk._h, w._h, nb, C.cast(cops, C.c_void_p), n, ints, C.byref(pbs), C.byref(rounds),
                                                flags))
        sk.sync()
    finally:
        if audit is not None:
            sk.set_audit(None)
    assert np.array_equal(w.download(np.arange(nb)), by), "the bystander integer in front of the operands was written"
    assert np.array_equal(w.download(np.arange(ints + scratch, ints + scratch + guard)), gd), "the guard band behind the scratch was written"
    vals = []
    for i in range(n):
        d = ck.decrypt_message_and_carry(w.download(np.arange((3 * i + 3) * nb, (3 * i + 4) * nb)))
        assert all(int(v) < 4 for v in d), (i, list(d))
        vals.append(E.from_digits(d))
    return vals


def run_cases(ck, sk, nb, ops, want, flags=0, audit=None):
    """The operators in as few levels as the look-up budget of a level allows (one, except for wide products and divisions)."""
    budget = 8192 if ck.t == 16 else 2048
    at = 0
    while at < len(ops):
        end, cost = at, 0
        while end < len(ops) and (end == at or cost + _cost(ops[end][0], nb) <= budget):
            cost += _cost(ops[end][0], nb)
            end += 1
        got = run_level(ck, sk, nb, ops[at:end], flags, audit)
        for op, g, wv in zip(ops[at:end], got, want[at:end]):
            assert g == wv, (E.KIND_NAMES[op[0]], nb, hex(op[1]), hex(op[2]), "got", hex(g), "want", hex(wv))
        at = end
    if audit is not None:
        assert not audit.bad, audit.bad[:8]


def _ops(kind, nb):
    cases = E.catalogue(kind, nb)
    ops = [(kind, a, b) for a, b, _ in cases]
    want = [wv for _, _, wv in cases]
    if kind == E.MUL:   # the squares: both operands the same rows
        sq = [a for a, b, _ in cases if a == b]
        ops += [(kind, a, a, True) for a in sq]
        want += [a * a % 4 ** nb for a in sq]
    return ops, want


def _report(name, aud, t0):
    print(f"{name}: {aud.luts} look-ups, {aud.lin} linear rows, largest term sum {aud.max_sum}, {time.perf_counter() - t0:.2f} s; margins " +
          ", ".join(f"{k} {v:.3f}" for k, v in sorted(aud.margin.items())))


ENCODINGS = [(16, 0), (16, MANY_LUT), (32, 0)]
WIDTHS = (1, 2, 3, 4, 5, 8, 16, 17, 32, 64)


@pytest.mark.parametrize("nb", WIDTHS)
@pytest.mark.parametrize("kinds", [(E.ADD, E.SUB), (E.ADD_SCALAR, E.SUB_SCALAR)], ids=["encrypted", "scalar"])
@pytest.mark.parametrize("enc,flags", ENCODINGS, indirect=["enc"], ids=["t16", "t16-many", "t32"])
def test_add_and_sub_and_their_scalar_forms(enc, flags, kinds, nb):
    ck, sk = enc
    t0, aud = time.perf_counter(), RadixAudit(ck)
    first = defaultdict(set)
    for kind in kinds:
        ops, want = _ops(kind, nb)
        run_cases(ck, sk, nb, ops, want, flags, aud)
        for k, v in aud.first.items():
            first[k] |= v
    _report(f"{E.KIND_NAMES[kinds[0]]}/{E.KIND_NAMES[kinds[1]]} nb={nb} t={ck.t} flags={flags}", aud, t0)
    # reach: a level of additions alone starts with round 1 of the propagation - the state tables, read at 7 on block 0
    # (x - 0 with x all ones) and at 6 elsewhere (all ones + all ones)
    state = ["pair%d" % p for p in range(4)] if flags else ["t0", "t1", "t2/q1", "t3"]
    if nb >= 2:
        assert 7 in first[state[0]] and max(first[state[0]]) == 7, first
        for p in range(1, min(nb - 1, 4)):
            assert max(first[state[p]]) == 6, (p, first)
    if flags:        # every integer: nb rotations, a state beside the message for all blocks but the top one
        assert aud.pair_rows > 0 and aud.pair_rows % nb == 0 and aud.pair_states == aud.pair_rows // nb * (nb - 1), (aud.pair_rows, aud.pair_states)
    if nb >= 5:      # V_3 of a full group: 30 when its four blocks generate, and beyond the padding bit's 16
        v3 = set().union(*(aud.reads[f] for f in E.V3_FAMILIES))
        assert 30 in v3 and any(16 <= v < 30 for v in v3), aud.reads
    if nb == 32:     # eight groups: the group states S_0 .. S_6 take the weights 1, 2, 4, 8 (no lut_q3_ without a carry out)
        for f in ("s0", "s1", "q3/s2", "s3"):
            assert {0, 15, 30} <= aud.reads[f], (f, aud.reads[f])
    if nb >= 17:
        assert aud.reads["resolve/gc2"]
    assert "unknown" not in aud.reads


@pytest.mark.parametrize("nb", WIDTHS)
@pytest.mark.parametrize("kind", [E.MUL, E.MUL_SCALAR], ids=["encrypted", "scalar"])
@pytest.mark.parametrize("enc,flags", ENCODINGS, indirect=["enc"], ids=["t16", "t16-many", "t32"])
def test_products(enc, flags, kind, nb):
    ck, sk = enc
    t0, aud = time.perf_counter(), RadixAudit(ck)
    ops, want = _ops(kind, nb)
    run_cases(ck, sk, nb, ops, want, flags, aud)
    _report(f"{E.KIND_NAMES[kind]} nb={nb} t={ck.t} flags={flags}", aud, t0)
    if kind == E.MUL:
        assert 15 in aud.reads["mul_lo"] and (nb < 2 or 15 in aud.reads["mul_hi"])   # packed product operands 4 * 3 + 3
        if nb >= 3:
            assert 15 in aud.reads["mul2_lo"] and 15 in aud.reads["mul2_hi"]
        assert aud.max_sum <= 15
    elif nb >= 2:
        assert aud.reads["carry"] and 9 <= aud.max_sum <= 15, aud.max_sum            # a digit-3 term alone is a sum of 9
    assert "unknown" not in aud.reads


@pytest.mark.parametrize("nb", (32, 64))
def test_the_all_three_scalar_product_stays_inside_its_scratch(toy16, nb):
    """x * (4^nb - 1): every digit term is reduced alone, the most vectors a level takes.  A case of its own - nothing else in
    the table, so a row past the declared scratch is a guard row."""
    ck, sk = toy16
    M = 4 ** nb
    for x in (M - 1, E.rep([1, 2, 3, 0, 2], nb)):
        assert run_level(ck, sk, nb, [(E.MUL_SCALAR, x, M - 1)]) == [x * (M - 1) % M]
    cop = (Op * 1)(Op(E.MUL_SCALAR, 0, -1, nb, 2 ** 64 - 1, 2 ** 64 - 1))
    declared = int(H.host.helm_host_radix_scratch_rows(sk._h, nb, C.cast(cop, C.c_void_p), 1))
    assert declared == E.level_take(nb, [E.Op(E.MUL_SCALAR, M - 1)])[0] > E.closed_form_rows(nb, [E.Op(E.MUL_SCALAR, M - 1)])


@pytest.mark.parametrize("nb", (4, 8, 16))
@pytest.mark.parametrize("enc,flags", [(16, 0), (32, 0)], indirect=["enc"], ids=["t16", "t32"])
def test_shifts_by_plain_and_encrypted_amounts(enc, flags, nb):
    ck, sk = enc
    t0, aud = time.perf_counter(), RadixAudit(ck)
    ops, want = [], []
    for kind in (E.SHL, E.SHR, E.SHL_SCALAR, E.SHR_SCALAR):
        o, wv = _ops(kind, nb)
        ops, want = ops + o, want + wv
    run_cases(ck, sk, nb, ops, want, flags, aud)      # the four kinds in ONE level
    _report(f"shifts nb={nb} t={ck.t}", aud, t0)
    assert 7 in aud.reads["sel"] and 15 in aud.reads["shl1"] and 15 in aud.reads["shr1"]
    assert aud.reads["bit0"] and aud.reads["bit1"] and "unknown" not in aud.reads


@pytest.mark.parametrize("nb", (3, 4, 7, 8, 16))
@pytest.mark.parametrize("part", (0, 1), ids=["first", "second"])
@pytest.mark.parametrize("kind", (E.DIV, E.DIV_SCALAR), ids=["encrypted", "scalar"])
@pytest.mark.parametrize("enc,flags", ENCODINGS, indirect=["enc"], ids=["t16", "t16-many", "t32"])
def test_division(enc, flags, kind, part, nb):
    """W = nb + 1 blocks of remainder: nb = 3 is the shape that reads lut_gc3_ on the n <= 4 path (the carry out of four blocks),
    nb = 7 the one that reads lut_q3_ (W = 8: the last group is full and its carry out is wanted).  The catalogue in two halves:
    a level costs the rounds of one division whatever it holds, and at t = 32 a round is a launch at N = 4096."""
    ck, sk = enc
    t0, aud = time.perf_counter(), RadixAudit(ck)
    ops, want = _ops(kind, nb)
    run_cases(ck, sk, nb, ops[part::2], want[part::2], flags, aud)
    _report(f"{E.KIND_NAMES[kind]} nb={nb} t={ck.t} flags={flags} half {part}", aud, t0)
    assert 7 in aud.reads["sel"] and aud.reads["cout"] and "unknown" not in aud.reads
    # the remainder's top block is the one the divisor lacks, and R < 2 B keeps it from generating together with the blocks
    # below it: V_3 = 30 is out of a division's reach (the additions reach it), past the padding bit's 16 is not
    if nb == 3:
        assert max(aud.reads["gc3"]) >= 16, aud.reads["gc3"]
    if nb == 7:      # group 0's state is lut_s_[0]; the s2 content here can only be lut_q3_
        assert max(aud.reads["q3/s2"]) >= 16, aud.reads["q3/s2"]
    print("V_3 reads of the carry out:", sorted(aud.reads["gc3"] | aud.reads["q3/s2"]))


def test_every_table_family_is_read_and_several_operators_share_a_level(toy16):
    """Three small levels of mixed operators reach every table of the constructor (the decoder names them by content)."""
    ck, sk = toy16
    aud = RadixAudit(ck)
    for nb in (3, 7, 32):
        M = 4 ** nb
        a, b = M - 1, E.rep([3, 1, 2], nb)
        kinds = (E.ADD, E.SUB, E.COPY) if nb == 32 else range(13)
        # shift amounts below the bit count: beyond it an encrypted amount is taken mod 2^ceil(log2(bits)), which is the bit
        # count only at the integer widths
        ops = [(k, a, 3 if k in (E.SHL, E.SHR, E.SHL_SCALAR, E.SHR_SCALAR) else b) for k in kinds] + [(E.MUL, b, b, True)]
        want = [E.answer(op[0], nb, op[1], op[2]) for op in ops]
        run_cases(ck, sk, nb, ops, want, 0, aud)
    missing = [f for f in E.FAMILIES if not aud.reads[f]]
    assert not missing and "unknown" not in aud.reads, (missing, sorted(aud.reads))


def test_the_block_count_the_entry_points_accept(toy16):
    """include/helm_host.h: 1 .. 64 blocks; 0 and 65 are errors at both entry points, not a walk with a scalar shifted by 128."""
    ck, sk = toy16
    cop = (Op * 1)(Op(E.ADD_SCALAR, 0, -1, 1, 3, 0))
    assert int(H.host.helm_host_radix_scratch_rows(sk._h, 1, C.cast(cop, C.c_void_p), 1)) > 0
    assert int(H.host.helm_host_radix_scratch_rows(sk._h, 64, C.cast(cop, C.c_void_p), 1)) > 0
    w = sk.wires(256)
    for blocks in (0, 65, -4):
        assert int(H.host.helm_host_radix_scratch_rows(sk._h, blocks, C.cast(cop, C.c_void_p), 1)) == -1
        with pytest.raises(helm_amd.HelmError, match="outside 1 .. 64"):
            H.check(H.host.helm_host_radix_level_ex(sk._h, w._h, blocks, C.cast(cop, C.c_void_p), 1, 130, None, None, 0))
        with pytest.raises(helm_amd.HelmError, match="outside 1 .. 64"):
            H.check(H.host.helm_host_radix_level(sk._h, w._h, blocks, C.cast(cop, C.c_void_p), 1, 130, None, None))


# ---- whole circuits: the carry-save forms and the lanes -------------------------------------------------------------------------
def _circuit(text):
    gs, ws, ins, outs, d, _, _ = verilog_parser.read_verilog_text(text, True)
    c = Circuit(gs, ins, outs, d)
    c.sort_circuit()
    c.compute_levels()
    return c, ws


def _int(ck, rows):
    vals = ck.decrypt_message_and_carry(rows)
    assert all(int(v) < 4 for v in vals), list(vals)
    return E.from_digits(vals)


CHAIN = """input A, B, C, D, E;
output X, S, T;
mult g0(A, B, t0);
mult g1(C, D, t1);
sub g2(t0, t1, X);
add g3(t0, t1, s0);
add g4(s0, E, s1);
sub g5(s1, A, s2);
add g6(s2, s0, S);
add g7(A, B, q0);
sub g8(q0, C, q1);
add g9(q1, D, q2);
add g10(q2, q2, T);
"""


@pytest.mark.parametrize("width", (8, 16))
@pytest.mark.parametrize("lazy", (True, False), ids=["lazy", "eager"])
def test_carry_save_circuits_at_all_ones(toy16, width, lazy):
    """mult, mult, sub and the addition chain of tests/test_gpu_modes.py with every input all ones, and with the subtrahend
    the larger product: every wire compared, audit on."""
    ck, sk = toy16
    m = 1 << width
    mk = {8: PtxtType.U8, 16: PtxtType.U16}[width]
    c, ws = _circuit(CHAIN)
    for a, b, cc, d, e in ((m - 1,) * 5, (3, 5, m - 1, m - 1, m - 1), (m - 1, m - 1, m - 1, 1, 0)):
        want = {"t0": a * b % m, "t1": cc * d % m}
        want["X"] = (want["t0"] - want["t1"]) % m
        want["s0"] = (want["t0"] + want["t1"]) % m
        want["s1"] = (want["s0"] + e) % m
        want["s2"] = (want["s1"] - a) % m
        want["S"] = (want["s2"] + want["s0"]) % m
        want["q0"] = (a + b) % m
        want["q1"] = (want["q0"] - cc) % m
        want["q2"] = (want["q1"] + d) % m
        want["T"] = 2 * want["q2"] % m
        aud = RadixAudit(ck)
        sk.set_audit(aud)   # before the evaluator forks its lanes
        try:
            ac = ArithCircuit(ck, sk, c)
            ac.set_lanes(1)
            ac.set_lazy_carries(lazy)
            out = ac.evaluate_encrypted(ac.encrypt_inputs(ws, {n: mk(v) for n, v in zip("ABCDE", (a, b, cc, d, e))}), 1, f"u{width}")
        finally:
            sk.set_audit(None)
        got = {wire: _int(ck, out[wire]) for wire in want}
        assert got == want, (lazy, (a, b, cc, d, e), got, want)
        assert not aud.bad and aud.luts == ac.pbs_per_cycle() and aud.max_sum <= 15, (aud.bad[:8], aud.max_sum)
        print(f"u{width} lazy={lazy}: {aud.luts} look-ups, largest term sum {aud.max_sum}")


def test_two_u64_sub_circuits_on_two_lanes(toy16):
    """A product by 2^32 - 1 (a netlist's plaintext operand is a u32, as the reference's: sixteen digit-3 terms, each reduced
    alone) beside a division, each on its own lane with its own scratch region next to the other's: right values, and word
    for word what set_lanes(1) computes."""
    ck, sk = toy16
    m = 1 << 64
    c, ws = _circuit("input A, B, C;\noutput P, Q;\nmult g0(A, 4294967295, P);\ndiv g1(B, C, Q);\n")
    a, b, d = m - 1, m - 1, (1 << 63) + 1
    ac = ArithCircuit(ck, sk, c)
    enc_in = ac.encrypt_inputs(ws, {"A": PtxtType.U64(a), "B": PtxtType.U64(b), "C": PtxtType.U64(d)})
    ac.set_lanes(1)
    one = ac.evaluate_encrypted(enc_in, 1, "u64")
    ac.set_lanes(2)
    two = ac.evaluate_encrypted(enc_in, 2, "u64")
    assert "2 independent sub-circuit(s)" in ac.log()
    for out in (one, two):
        assert (_int(ck, out["P"]), _int(ck, out["Q"])) == (a * (2 ** 32 - 1) % m, b // d)
    for wire in one.keys():
        assert np.array_equal(one[wire], two[wire]), wire


# ---- the measured margin at a real parameter set --------------------------------------------------------------------------------
def test_noise_margin_at_the_full_size_set():
    """u8 at shortint_m2c2: the product of all ones and divisions by a divisor with its top bit set.  Written down, per table
    family: the largest |phase - v delta| / (delta / 2) over the look-up inputs (1 would be a wrong look-up)."""
    ck, sk = helm_amd.gen_keys_shortint("shortint_m2c2", seed=1)
    aud = RadixAudit(ck)
    t0 = time.perf_counter()
    ops = [(E.MUL, 0xFF, 0xFF), (E.MUL, 0xFF, 0xFF, True), (E.MUL_SCALAR, 0xFF, 0xFF), (E.DIV, 0xFF, 0x80), (E.DIV, 0xFF, 0x81),
           (E.DIV_SCALAR, 0xFE, 0xFF), (E.SUB, 0xFF, 0)]
    want = [0x01, 0x01, 0x01, 1, 1, 0, 0xFF]
    try:
        run_cases(ck, sk, 4, ops, want, 0, aud)
    finally:
        sk.close()
    _report("shortint_m2c2 u8", aud, t0)
    # 1 would be a wrong look-up.  The ceiling asserted is 0.5: the set's failure probability per look-up, 2^-43,
    # puts the half-box at 7.6 standard deviations of ALL the noise a look-up sees - input, keyswitch, modulus switch - so the
    # input's share alone stays below 4 of them = 0.53 over a thousand samples with room to spare; above it margin has been lost
    assert aud.margin and max(aud.margin.values()) < 0.5, dict(aud.margin)
