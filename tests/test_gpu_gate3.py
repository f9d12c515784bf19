"""The three-input gates MAJ3 / XOR3 / XNOR3 (op-codes 20 / 21 / 22) on the GPU.

Reference of every ciphertext: the three-operand combination formed HERE in numpy with uint32 wrap-around
(l + r + c, 0 - 2 (l + r + c), 2 (l + r + c) on every word, no constant), then Oracle.bootstrap_noks with the gates' test
vector (all +1/8) and Oracle.keyswitch - in order 1 the keyswitch first, as tests/ks_first.py composes it.  oracle.lincomb
is not extended.

  every build     one level of 48 gates (3 ops x 8 input combinations, on fresh encryptions and on trivial rows) and one of
                  crafted operand triples on every context tests/test_gpu_rotation_edges.py enumerates (lockstep, wide, duo,
                  trio / tri10, generic, two-prime admitted and forced), and the 48 gates on the keyswitch-first sets of
                  tests/test_gpu_ks_first.py on both keyswitch paths; word for word, decrypted, the build asserted
  mixed levels    AND, MUX, MAJ3, NOT, XOR3, XNOR3 interleaved at widths 1, 5, 160 and launch quantum + 1 (the size dispatch),
                  a gate that overwrites its own third operand; eval_gate_level, a program, a packed program, two ranks
  refusals        op 20 without in2, op 23
  counting build  zero violations on tuned contexts
  GateCircuit     the fused adders end to end"""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helm_amd
import oracle
from helm_amd import Circuit, GateCircuit, PtxtType, verilog_parser
from helm_amd.distributed import pack_levels
from helm_amd.netlists import ripple_adder, two_bit_adder
from helm_amd.verilog_parser import fuse3

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rotation_edges as RE  # noqa: E402
import saturation as S  # noqa: E402
import test_gpu_eight_ranks as T8  # noqa: E402
import test_gpu_ks_first as TKF  # noqa: E402
import test_gpu_rotation_edges as TRE  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AND, MUX, NOT, MAJ3, XOR3, XNOR3 = 0, 3, 6, 20, 21, 22
OPS3 = (MAJ3, XOR3, XNOR3)
PT_TRUE, PT_FALSE = np.uint32(1 << 29), np.uint32(7 << 29)
TRUTH = {MAJ3: lambda a, b, c: a + b + c >= 2, XOR3: lambda a, b, c: (a + b + c) % 2 == 1,
         XNOR3: lambda a, b, c: (a + b + c) % 2 == 0}


def lin3(op, l, r, c):
    """The row a three-input gate bootstraps: the same formula on every word, uint32 wrap-around, no constant."""
    with np.errstate(over="ignore"):
        s = (l.astype(np.uint32) + r.astype(np.uint32) + c.astype(np.uint32)).astype(np.uint32)
        if op == MAJ3:
            return s
        if op == XNOR3:
            return (np.uint32(2) * s).astype(np.uint32)
        assert op == XOR3
        return (np.uint32(0) - np.uint32(2) * s).astype(np.uint32)


def ref_gate3(orc, op, l, r, c, order=0):
    tv = np.full(orc.p.N, PT_TRUE, dtype=np.uint32)
    row = np.ascontiguousarray(lin3(op, l, r, c))
    if order == 1:
        return orc.bootstrap_noks(orc.keyswitch(row), tv)
    return orc.keyswitch(orc.bootstrap_noks(row, tv))


def level48(fresh, dim):
    """Rows 0..5: fresh encryptions of (F, T) for operand 0, 1 and 2; rows 6, 7: trivial F, T.  -> (wires [56, dim + 1], ops,
    in0, in1, in2, out, truth): 3 ops x 8 combinations on the fresh rows, then the same on the trivial ones."""
    wires = np.zeros((56, dim + 1), dtype=np.uint32)
    wires[:6] = fresh
    wires[6, dim], wires[7, dim] = PT_FALSE, PT_TRUE
    ops, i0, i1, i2, truth = [], [], [], [], []
    for trivial in (False, True):
        for op in OPS3:
            for a, b, c in itertools.product((0, 1), repeat=3):
                ops.append(op)
                rows = (6 + a, 6 + b, 6 + c) if trivial else (a, 2 + b, 4 + c)
                i0.append(rows[0]); i1.append(rows[1]); i2.append(rows[2])
                truth.append(bool(TRUTH[op](a, b, c)))
    a32 = lambda v: np.array(v, dtype=np.int32)  # noqa: E731
    return wires, a32(ops), a32(i0), a32(i1), a32(i2), np.arange(8, 56, dtype=np.int32), np.array(truth)


def crafted_triples(n, N, rng):
    """Operand triples solved so that the gate's own combination is a chosen row (tests/rotation_edges.py's construction for
    the two-input gates): every mask word switches to t, the body to the next t, for t in 0, 1, N - 1, N, N + 1, 2N - 1 in
    the flavours exact / below / tie; the parities in both pre-images of the doubling; l and c are drawn from the top
    quarter so that l + r + c passes 2^32 twice in most words.  -> dict(op, l, r, c, want, twice {op: words})"""
    targets = [0, 1, N - 1, N, N + 1, 2 * N - 1]
    ops, ls, rs, cs, wants, twice = [], [], [], [], [], {op: 0 for op in OPS3}
    for op in OPS3:
        for ti, t in enumerate(targets):
            body_t = targets[(ti + 1) % len(targets)]
            for f in RE.FLAVOURS:
                for top in ((0, 1) if op != MAJ3 else (-1,)):
                    want = [RE.word_for(t, N, 32, f)] * n + [RE.word_for(body_t, N, 32, f)]
                    if op != MAJ3:  # the doubling reaches even words only
                        want = [RE._even_word(w, a, N)[0] for w, a in zip(want, [t] * n + [body_t])]
                    l = [int(v) for v in rng.integers(3 << 30, 1 << 32, n + 1)]
                    c = [int(v) for v in rng.integers(3 << 30, 1 << 32, n + 1)]
                    r = []
                    for i in range(n + 1):
                        if op == MAJ3:
                            s = want[i]
                        elif op == XNOR3:     # 2 s = want: s = want / 2 or want / 2 + 2^31
                            s = want[i] // 2 + (top << 31)
                        else:                 # -2 s = want
                            s = (-(want[i] // 2)) % (1 << 31) + (top << 31)
                        r.append((s - l[i] - c[i]) % RE.MOD32)
                        twice[op] += (l[i] + r[i] + c[i]) >> 32 == 2
                        if op != MAJ3:
                            assert ((l[i] + r[i] + c[i]) % RE.MOD32) >> 31 == top
                    assert [S.modswitch(w, N, 32) for w in want] == [t] * n + [body_t]
                    for lst, v in zip((ops, ls, rs, cs, wants), (op, l, r, c, want)):
                        lst.append(v)
    u32 = lambda rows: np.array(rows, dtype=np.uint32)  # noqa: E731
    G = dict(op=np.array(ops, dtype=np.int32), l=u32(ls), r=u32(rs), c=u32(cs), want=u32(wants), twice=twice)
    assert all(v > 0 for v in twice.values()), twice
    for q in range(len(ops)):
        assert np.array_equal(lin3(int(G["op"][q]), G["l"][q], G["r"][q], G["c"][q]), G["want"][q])
    return G


# ------------------------------------------------------------------------------------------------------------------
# every build
# ------------------------------------------------------------------------------------------------------------------
_sets = {}


def _set(which):
    """The two workloads of a key and their references: computed once, read by every build of the set."""
    if which not in _sets:
        ck = TRE._bool_key(which)
        p = ck.params
        orc = oracle.Oracle(p.as_tuple7(), ck.bsk, ck.ksk, use_ntt=True)
        wires, ops, i0, i1, i2, out, truth = level48(ck.encrypt([False, True] * 3), p.n)
        want = np.stack([ref_gate3(orc, int(ops[g]), wires[i0[g]], wires[i1[g]], wires[i2[g]]) for g in range(48)])
        assert np.array_equal(ck.decrypt(want), truth)
        G = crafted_triples(p.n, p.N, np.random.default_rng(p.n + p.N))
        gwant = np.stack([ref_gate3(orc, int(G["op"][q]), G["l"][q], G["r"][q], G["c"][q]) for q in range(len(G["op"]))])
        _sets[which] = dict(ck=ck, level=(wires, ops, i0, i1, i2, out, truth), want=want, G=G, gwant=gwant)
    return _sets[which]


def run_build(case, crafted=True, check_build=False):
    st = _set(case[0])
    wires, ops, i0, i1, i2, out, truth = st["level"]
    sk = TRE._bool_context(case)            # asserts kernel_class() and field_bits() of the build that runs
    try:
        if check_build:
            sk.bound_violations(reset=True)
        w = sk.wires(56)
        w.upload(np.arange(8), wires[:8])
        w.eval_gate_level(ops, i0, i1, i2, out)
        got = w.download()
        bad = np.flatnonzero((got[8:] != st["want"]).any(axis=1))
        assert len(bad) == 0, "%s: gates %s (op, in0, in1, in2) differ" % (
            TRE._bool_id(case), [(int(ops[g]), int(i0[g]), int(i1[g]), int(i2[g])) for g in bad[:6]])
        assert np.array_equal(st["ck"].decrypt(got[8:]), truth)
        assert np.array_equal(got[:8], wires[:8])
        if crafted:
            G = st["G"]
            count = len(G["op"])
            ar = np.arange(count, dtype=np.int32)
            w = sk.wires(4 * count)
            w.upload(np.arange(3 * count), np.concatenate([G["l"], G["r"], G["c"]]))
            w.eval_gate_level(G["op"], ar, count + ar, 2 * count + ar, 3 * count + ar)
            bad = np.flatnonzero((w.download(3 * count + ar) != st["gwant"]).any(axis=1))
            assert len(bad) == 0, "%s: crafted gates %s differ (ops %s)" % (TRE._bool_id(case), bad[:8], G["op"][bad[:8]])
        assert sk.field_bits() == case[4] and sk.kernel_class() == case[5]
        return sk.bound_violations() if check_build else None
    finally:
        sk.close()


@pytest.mark.parametrize("case", TRE.BOOL_CASES, ids=[TRE._bool_id(c) for c in TRE.BOOL_CASES])
def test_three_input_gates_on_every_build(case):
    run_build(case)


@pytest.mark.parametrize("name", list(TKF.SETS))
def test_three_input_gates_keyswitch_first(name):
    """pbs_order = 1: combination over k N + 1 words -> keyswitch -> bootstrap, on the matrix-core and the vector-ALU
    keyswitch (k_ks_gate_digits / k_keyswitch_gate form the combination as they read the rows)."""
    k = TKF.keys(name)
    wires, ops, i0, i1, i2, out, truth = level48(k.ck.encrypt([False, True] * 3), k.kN)
    want = np.stack([ref_gate3(k.ref.orc, int(ops[g]), wires[i0[g]], wires[i1[g]], wires[i2[g]], order=1) for g in range(48)])
    assert np.array_equal(k.ck.decrypt(want), truth)
    for ks_mfma in ([None, 0] if k.mfma else [None]):
        sk = k.server(ks_mfma)
        try:
            assert sk.kernel_class() == TKF.CLASS.get(name, "tuned") and sk.wire_words() == k.kN + 1
            w = sk.wires(56)
            w.upload(np.arange(8), wires[:8])
            w.eval_gate_level(ops, i0, i1, i2, out)
            got = w.download()
            bad = np.flatnonzero((got[8:] != want).any(axis=1))
            assert len(bad) == 0, (name, ks_mfma, bad[:8], ops[bad[:8]])
            assert np.array_equal(k.ck.decrypt(got[8:]), truth)
        finally:
            sk.close()


# ------------------------------------------------------------------------------------------------------------------
# mixed levels
# ------------------------------------------------------------------------------------------------------------------
MIX = [AND, MUX, MAJ3, NOT, XOR3, XNOR3]
N_IN = 8


def _ref_level(orc, src, ops, i0, i1, i2, out):
    """One level on a copy of `src`: the two-input gates, MUX and NOT by Oracle.eval_level, the three-input ones by the
    composition above; every gate reads the table as it was before the level."""
    dst = src.copy()
    old = np.flatnonzero(~np.isin(ops, OPS3))
    if len(old):
        orc.eval_level(dst, ops[old], i0[old], i1[old], i2[old], out[old])
    for g in np.flatnonzero(np.isin(ops, OPS3)):
        dst[out[g]] = ref_gate3(orc, int(ops[g]), src[i0[g]], src[i1[g]], src[i2[g]])
    return dst


def _plain_level(v, ops, i0, i1, i2, out):
    r = v.copy()
    for g in range(len(ops)):
        a, b, c = bool(v[i0[g]]), bool(v[max(i1[g], 0)]), bool(v[max(i2[g], 0)])
        op = int(ops[g])
        r[out[g]] = (TRUTH[op](a, b, c) if op in OPS3 else a and b if op == AND else (a if c else b) if op == MUX else not a)
    return r


@pytest.fixture(scope="module")
def mixed():
    """quantum + 1 gates of MIX interleaved over 8 input rows (a launch of `count` gates is the pool's first `count`): the
    reference rows of the widest launch; gate 4 (XOR3) writes the row of its own third operand."""
    ck = helm_amd.ClientKey.generate("toy_k2", seed=31)
    sk = helm_amd.ServerKey(ck, device=0)
    assert sk.kernel_class() == "tuned"
    quantum = sk.launch_quantum()
    sk.close()
    total = quantum + 1
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2, N_IN).astype(bool)
    ct = ck.encrypt(bits)
    ops = np.array([MIX[g % 6] for g in range(total)], dtype=np.int32)
    i0, i1, i2 = (rng.integers(0, N_IN, total).astype(np.int32) for _ in range(3))
    i1[ops == NOT] = -1
    i2[np.isin(ops, (AND, NOT))] = -1
    out = np.arange(N_IN, N_IN + total, dtype=np.int32)
    out[4], i2[4] = 7, 7                    # XOR3 in place: out = in2 = row 7
    for g in range(total):                  # (nobody else reads or writes row 7: no hazard between gates)
        if g != 4:
            for arr in (i0, i1, i2):
                if arr[g] == 7:
                    arr[g] = 6
    assert ops[4] == XOR3
    orc = oracle.Oracle(ck.params.as_tuple7(), ck.bsk, ck.ksk, use_ntt=True)
    src = np.zeros((N_IN + total, ck.params.n + 1), dtype=np.uint32)
    src[:N_IN] = ct
    want = _ref_level(orc, src, ops, i0, i1, i2, out)
    plain = np.zeros(N_IN + total, dtype=bool)
    plain[:N_IN] = bits
    rows = np.concatenate([np.arange(N_IN), out])    # (row N_IN + 4 is never written: gate 4 writes row 7)
    assert np.array_equal(ck.decrypt(want[rows]), _plain_level(plain, ops, i0, i1, i2, out)[rows])
    return dict(ck=ck, ct=ct, arrays=(ops, i0, i1, i2, out), src=src, want=want, quantum=quantum, total=total)


def _want_prefix(m, count):
    """The table after the first `count` gates alone (rows of the others as they were)."""
    ops, i0, i1, i2, out = m["arrays"]
    w = m["src"].copy()
    w[out[:count]] = m["want"][out[:count]]
    return w


def test_mixed_level_at_the_dispatch_widths(mixed):
    m = mixed
    ops, i0, i1, i2, out = m["arrays"]
    sk = helm_amd.ServerKey(m["ck"], device=0)
    try:
        for count in (1, 5, 160, m["total"]):   # ascending: the context's buffers grow between launches
            w = sk.wires(len(m["src"]))
            w.upload(np.arange(N_IN), m["ct"])
            w.eval_gate_level(ops[:count], i0[:count], i1[:count], i2[:count], out[:count])
            assert np.array_equal(w.download(), _want_prefix(m, count)), count
            w.free()
    finally:
        sk.close()


def test_mixed_level_as_a_program_and_packed(mixed):
    """One level of 160 gates as a program; the same gates in two dependent levels (the second reads the first's outputs)
    packed at quantum 32 - launches cut by bootstrap weight - against the level schedule's table."""
    m = mixed
    ops, i0, i1, i2, out = (a[:160] for a in m["arrays"])
    sk = helm_amd.ServerKey(m["ck"], device=0)
    try:
        prog = helm_amd.Program(sk, ops, i0, i1, i2, out, np.array([0, 160], dtype=np.int64))
        assert prog.level_pbs(0) == int(np.sum(np.where(ops == MUX, 2, np.where(ops == NOT, 0, 1))))
        w = sk.wires(len(m["src"]))
        w.upload(np.arange(N_IN), m["ct"])
        prog.run(w)
        assert np.array_equal(w.download(), _want_prefix(m, 160))
        prog.destroy()
        # level 2: 60 three-input gates on level-1 outputs
        orc = oracle.Oracle(m["ck"].params.as_tuple7(), m["ck"].bsk, m["ck"].ksk, use_ntt=True)
        rng = np.random.default_rng(8)
        ops2 = np.array([OPS3[g % 3] for g in range(60)], dtype=np.int32)
        j0, j1, j2 = (rng.integers(N_IN + 8, N_IN + 160, 60).astype(np.int32) for _ in range(3))
        out2 = np.arange(N_IN + m["total"], N_IN + m["total"] + 60, dtype=np.int32)
        src = np.concatenate([_want_prefix(m, 160), np.zeros((60, m["src"].shape[1]), dtype=np.uint32)])
        want = _ref_level(orc, src, ops2, j0, j1, j2, out2)
        cat = lambda a, b: np.concatenate([a, b])  # noqa: E731
        arrays = (cat(ops, ops2), cat(i0, j0), cat(i1, j1), cat(i2, j2), cat(out, out2))
        off = np.array([0, 160, 220], dtype=np.int64)
        packed = pack_levels(*arrays, off, 32)
        assert packed[6] and len(packed[5]) > 3
        for arrs in (arrays + (off,), packed[:6]):
            prog = helm_amd.Program(sk, *arrs)
            w = sk.wires(len(src))
            w.upload(np.arange(N_IN), m["ct"])
            prog.run(w)
            assert np.array_equal(w.download(), want)
            prog.destroy()
    finally:
        sk.close()


def test_mixed_level_over_two_ranks(mixed):
    """Two rank threads over the in-process transport: the level of 160 gates is cut by bootstrap weight (shard_rule.h:
    MAJ3 / XOR3 / XNOR3 weigh 1), every rank ends with the unsharded table."""
    m = mixed
    arrays = tuple(a[:160] for a in m["arrays"]) + (np.array([0, 160], dtype=np.int64),)
    tables, stats, sharded = T8._run_world(2, arrays, len(m["src"]), np.arange(N_IN, dtype=np.int32), m["ct"], m["ck"], 4, False)
    assert sharded == 1 and stats[0] == stats[1] == 1
    for r in range(2):
        assert np.array_equal(tables[r], _want_prefix(m, 160)), r


# ------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    ck = helm_amd.ClientKey.generate("toy", seed=1)
    sk = helm_amd.ServerKey(ck, device=0)
    try:
        w = sk.wires(4)
        w.upload([0, 1, 2], ck.encrypt([True, False, True]))
        a32 = lambda v: np.array(v, dtype=np.int32)  # noqa: E731
        for op in OPS3:
            with pytest.raises(helm_amd.HelmError, match="gate 0: missing operand"):
                w.eval_gate_level(a32([op]), a32([0]), a32([1]), a32([-1]), a32([3]))
        with pytest.raises(helm_amd.HelmError, match="op 23 can't be mixed with Boolean gates"):
            w.eval_gate_level(a32([23]), a32([0]), a32([1]), a32([2]), a32([3]))
        with pytest.raises(helm_amd.HelmError, match="missing operand"):
            helm_amd.Program(sk, a32([MAJ3]), a32([0]), a32([1]), a32([-1]), a32([3]), np.array([0, 1], dtype=np.int64))
        w.eval_gate_level(a32([MAJ3]), a32([0]), a32([1]), a32([2]), a32([3]))      # and the context still works
        assert ck.decrypt(w.download([3]))[0]
    finally:
        sk.close()


# ------------------------------------------------------------------------------------------------------------------
# the counting build
# ------------------------------------------------------------------------------------------------------------------
CHECK_CASES = [c for c in TRE.BOOL_CASES if c[5] == "tuned" and c[1] is None and c[2] is None and c[3] is None]


def child_main():
    """Runs in the child process of test_counting_build_counts_nothing."""
    res = {TRE._bool_id(case): run_build(case, crafted=False, check_build=True) for case in CHECK_CASES}
    print("RESULT " + json.dumps(res))


def test_counting_build_counts_nothing():
    """The 48-gate level on every tuned set under libhelm_hip_check.so: word for word, every counter zero.  One child."""
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    assert {c[0] for c in CHECK_CASES} >= {"toy_k2", "toy", "toy_1024"}
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_gate3 as T; T.child_main()" % (ROOT, os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HELM_HIP_LIB=lib), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res == {TRE._bool_id(c): [0] * 8 for c in CHECK_CASES}, res


# ------------------------------------------------------------------------------------------------------------------
# GateCircuit end to end
# ------------------------------------------------------------------------------------------------------------------
def _circuit(text):
    gates, wire_set, inputs, outputs, dffs, _, _ = verilog_parser.read_verilog_text(text, False)
    c = Circuit(gates, inputs, outputs, dffs)
    c.sort_circuit()
    c.compute_levels()
    return c, wire_set, inputs


def _end_to_end(ck, sk, text, cases, n_pbs):
    circuit, wire_set, inputs = _circuit(text)
    gc = GateCircuit(ck, sk, circuit)
    for vals in cases:
        ptxt = {x: PtxtType.None_() for x in wire_set}
        ptxt.update({k: PtxtType.Bool(v) for k, v in vals.items()})
        ptxt = circuit.evaluate(ptxt)
        enc = gc.evaluate_encrypted(gc.encrypt_inputs(wire_set, {k: PtxtType.Bool(v) for k, v in vals.items()}), 1, "bool")
        for name in sorted(ptxt):
            assert ck.decrypt(enc[name]) == bool(ptxt[name].value), (name, vals)
        assert gc.pbs_per_cycle() == n_pbs
    return ptxt


def _adder_inputs(nbits, a, b, cin):
    v = {f"a[{i}]": bool((a >> i) & 1) for i in range(nbits)}
    v.update({f"b[{i}]": bool((b >> i) & 1) for i in range(nbits)})
    v["cin"] = bool(cin)
    return v


def test_fused_adders_through_gate_circuit_toy():
    ck = helm_amd.ClientKey.generate("toy_k2", seed=3)
    sk = helm_amd.ServerKey(ck, device=0)
    try:
        golden = verilog_parser.read_input_wires(os.path.join(ROOT, "tests", "golden", "2-bit-adder.inputs.csv"), "bool")
        k2 = {k: bool(v.value) for k, v in golden.items()}
        _end_to_end(ck, sk, fuse3(two_bit_adder())[0], [_adder_inputs(2, 3, 3, 1), k2], 4)
        rng = np.random.default_rng(12)
        cases = [_adder_inputs(8, int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 2))) for _ in range(4)]
        cases[0] = _adder_inputs(8, 255, 1, 0)      # the carry runs through every maj
        out = _end_to_end(ck, sk, ripple_adder(8, fused=True), cases, 16)
        a = sum(int(cases[-1][f"a[{i}]"]) << i for i in range(8))
        b = sum(int(cases[-1][f"b[{i}]"]) << i for i in range(8))
        assert sum(out[f"sum[{i}]"].value << i for i in range(8)) + (out["cout"].value << 8) == a + b + int(cases[-1]["cin"])
    finally:
        sk.close()


def test_fused_ripple_adder_at_boolean_default():
    client_key, server_key = helm_amd.gen_keys("boolean_default", seed=2)
    try:
        _end_to_end(client_key, server_key, ripple_adder(8, fused=True), [_adder_inputs(8, 0xB5, 0x6E, 1)], 16)
    finally:
        server_key.close()
