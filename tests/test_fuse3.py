"""Three-input gates of gates mode (HELM_GATE_MAJ3 / XOR3 / XNOR3, keywords maj / xor3 / xnor3) and the opt-in fusion
pass that writes them (helm_host_fuse3, helm_amd/csrc/host/fuse3.cpp), on the CPU: the plaintext evaluator's truth tables,
the parser, the linear formulas on exact encodings, the pass on the repository's generators (exact gate counts, caps on
bootstraps and bootstrapped levels, wire-for-wire equivalence), its guards on handwritten netlists, the bootstrap weights
the launch packing and the shard cut give the new ops, and the noise budget of the new operands per boolean set."""
import itertools
import math

import numpy as np
import pytest

import helm_amd
from helm_amd import Circuit, PtxtType, verilog_parser
from helm_amd import _host as H
from helm_amd.distributed import pack_levels
from helm_amd.gates import GateType
from helm_amd.netlists import aes128, aes128_reference_encrypt, alu_c880_class, ripple_adder, two_bit_adder
from helm_amd.verilog_parser import fuse3

T, F = 1 << 29, 7 << 29  # +1/8, -1/8 (include/helm_hip.h)
AND, MUX, NOT, MAJ3, XOR3, XNOR3 = 0, 3, 6, 20, 21, 22
TRUTH = {"maj": lambda a, b, c: a + b + c >= 2, "xor3": lambda a, b, c: (a + b + c) % 2 == 1,
         "xnor3": lambda a, b, c: (a + b + c) % 2 == 0}


class Netlist:
    """A parsed and levelled netlist; values(bits) -> plaintext value of every wire."""

    def __init__(self, text):
        gates, self.wire_set, self.inputs, self.outputs, dffs, _, _ = verilog_parser.read_verilog_text(text, False)
        self.gates = list(gates)
        self.circuit = Circuit(gates, self.inputs, self.outputs, dffs)
        self.circuit.sort_circuit()
        self.circuit.compute_levels()

    def values(self, bits):
        m = {w: PtxtType.None_() for w in self.wire_set}
        m.update({w: PtxtType.Bool(bits[w]) for w in self.inputs})
        return {k: int(v.value) for k, v in self.circuit.evaluate(m).items()}

    def keywords(self):
        count = {}
        for g in self.gates:
            count[g.gate_type.name] = count.get(g.gate_type.name, 0) + 1
        return count


def _module(body, inputs="a, b, c, d", outputs="y"):
    return (f"module m({inputs}, {outputs});\n  input {inputs};\n  output {outputs};\n" +
            "".join(f"  {line}\n" for line in body) + "endmodule\n")


def _gate_lines(text):
    return [l.strip() for l in text.splitlines() if l.strip() and l.split()[0] not in ("module", "endmodule", "input", "output", "wire")]


def _assert_equivalent(original, fused, cases):
    a, b = Netlist(original), Netlist(fused)
    assert set(b.inputs) == set(a.inputs) and b.outputs == a.outputs
    assert set(b.wire_set) <= set(a.wire_set)
    for bits in cases:
        va, vb = a.values(bits), b.values(bits)
        for w in list(b.wire_set) + list(b.inputs):
            assert vb[w] == va[w], w
    return a, b


# ---------------------------------------------------------------------------------------------- the three gate types
@pytest.mark.parametrize("kw", ["maj", "xor3", "xnor3"])
def test_truth_tables_through_the_plaintext_evaluator(kw):
    nl = Netlist(_module([f"{kw} g0(a, b, c, y);"], inputs="a, b, c"))
    assert [g.gate_type for g in nl.gates] == [{"maj": GateType.Maj3, "xor3": GateType.Xor3, "xnor3": GateType.Xnor3}[kw]]
    assert int(nl.gates[0].gate_type) == {"maj": 20, "xor3": 21, "xnor3": 22}[kw]
    assert nl.gates[0].input_wires == ["a", "b", "c"] and nl.gates[0].output_wire == "y"
    for a, b, c in itertools.product((0, 1), repeat=3):
        assert nl.values({"a": a, "b": b, "c": c})["y"] == int(TRUTH[kw](a, b, c)), (a, b, c)


def test_parser_accepts_maj_and_refuses_a_wrong_arity():
    verilog_parser.read_verilog_text(_module(["maj g0(a, b, c, y);"]), False)  # `Invalid gate type "maj"` without the feature
    for kw in ("maj", "xor3", "xnor3"):
        for args in ("a, b, y", "a, b, c, d, y", "a, y"):
            with pytest.raises(H.Panic, match="exactly three inputs"):
                verilog_parser.read_verilog_text(_module([f"{kw} g0({args});"]), False)
    with pytest.raises(H.Panic, match='Invalid gate type "maj3"'):
        verilog_parser.read_verilog_text(_module(["maj3 g0(a, b, c, y);"]), False)


def test_linear_formulas_on_exact_encodings():
    """l + r + c (MAJ3), 0 - 2 (l + r + c) (XOR3), 2 (l + r + c) (XNOR3) mod 2^32 on +-1/8: the sign of the phase is the
    truth value (true <=> phase < 1/2), and the phase is +-1/8 {1, 3} for MAJ3, +-2/8 for the parities - never 0 or 1/2."""
    for a, b, c in itertools.product((0, 1), repeat=3):
        s = np.uint32(0)
        with np.errstate(over="ignore"):
            for bit in (a, b, c):
                s = np.uint32(s + np.uint32(T if bit else F))
            phases = {"maj": s, "xor3": np.uint32(np.uint32(0) - np.uint32(np.uint32(2) * s)), "xnor3": np.uint32(np.uint32(2) * s)}
        for kw, ph in phases.items():
            ph = int(ph)
            assert (ph < (1 << 31)) == TRUTH[kw](a, b, c), (kw, a, b, c)
            signed = ph if ph < (1 << 31) else ph - (1 << 32)
            assert abs(signed) in ({1 << 29, 3 << 29} if kw == "maj" else {2 << 29}), (kw, a, b, c)


# ---------------------------------------------------------------------------------------------- the pass on the generators
@pytest.mark.parametrize("n", [1, 8, 32])
def test_ripple_adder_becomes_xor3_and_maj_alone(n):
    fused, stats = fuse3(ripple_adder(n))
    assert Netlist(fused).keywords() == {"Xor3": n, "Maj3": n}
    assert stats == (5 * n, 2 * n, 2 * n + 1, n)
    assert ripple_adder(n, fused=True) == fused


def test_two_bit_adder_is_four_gates_and_equivalent_on_all_inputs():
    original = two_bit_adder()
    fused, stats = fuse3(original)
    assert _gate_lines(fused) == ["xor3 g1(a[0], b[0], cin, sum[0]);", "maj g4(a[0], b[0], cin, i4);",
                                  "xor3 g6(a[1], b[1], i4, sum[1]);", "maj g9(a[1], b[1], i4, cout);"]
    assert stats == (10, 4, 5, 2)
    names = ["a[0]", "a[1]", "b[0]", "b[1]", "cin"]
    _assert_equivalent(original, fused, [dict(zip(names, v)) for v in itertools.product((0, 1), repeat=5)])


def test_c880_class_caps_and_equivalence():
    original = alu_c880_class()
    fused, stats = fuse3(original)
    assert stats[0] == 372 and stats[2] == 22
    assert stats[1] <= 289 and stats[3] <= 13           # the caps of the greedy prototype
    assert stats == (372, 289, 22, 13)                  # this pass, exactly
    rng = np.random.default_rng(880)
    inputs = Netlist(original).inputs
    _assert_equivalent(original, fused, [{w: int(rng.integers(0, 2)) for w in inputs} for _ in range(64)])
    assert fuse3(fused) == (fused, (289, 289, 13, 13))


def _bus_bits(name, data):
    v = int.from_bytes(data, "big")
    return {f"{name}[{i}]": (v >> i) & 1 for i in range(8 * len(data))}


def test_aes128_caps_and_equivalence():
    original = aes128()
    fused, stats = fuse3(original)
    assert stats[0] == 32464 and stats[2] == 207
    assert stats[1] <= 26203 and stats[3] <= 200        # the caps of the greedy prototype
    assert stats == (32464, 26203, 207, 200)            # this pass, exactly
    rng = np.random.default_rng(128)
    pairs = [(bytes(range(16)), bytes.fromhex("00112233445566778899aabbccddeeff"))]  # FIPS-197 C.1
    pairs += [(bytes(rng.integers(0, 256, 16, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))) for _ in range(3)]
    cases = [{**_bus_bits("key", k), **_bus_bits("pt", p)} for k, p in pairs]
    _, b = _assert_equivalent(original, fused, cases)
    out = b.values(cases[0])
    assert sum(out[f"ct[{i}]"] << i for i in range(128)).to_bytes(16, "big") == bytes.fromhex("69c4e0d86a7b0430d8cdb78070b4c55a")
    k, p = pairs[1]
    out = b.values(cases[1])
    assert sum(out[f"ct[{i}]"] << i for i in range(128)).to_bytes(16, "big") == aes128_reference_encrypt(k, p)
    assert fuse3(fused)[0] == fused


def test_a_netlist_without_the_patterns_comes_back_byte_for_byte():
    text = _module(["and g0(a, b, n0);", "nand g1(n0, c, n1);", "mux g2(n0, n1, d, y);"]).replace("endmodule\n", "endmodule")
    assert fuse3(text) == (text, (4, 4, 3, 3))


# ---------------------------------------------------------------------------------------------- guards
def test_an_inner_wire_that_is_a_module_output_is_not_fused():
    text = _module(["xor g0(a, b, z);", "xor g1(z, c, y);"], outputs="y, z")
    assert fuse3(text) == (text, (2, 2, 2, 2))
    text = _module(["xor g0(a, b, x);", "and g1(a, b, p);", "and g2(x, c, q);", "or g3(p, q, y);"], outputs="y, p")
    assert fuse3(text) == (text, (4, 4, 3, 3))


def test_an_inner_wire_read_twice_is_not_fused():
    text = _module(["xor g0(a, b, n0);", "xor g1(n0, c, y);", "and g2(n0, d, z);"], outputs="y, z")
    assert fuse3(text) == (text, (3, 3, 2, 2))
    text = _module(["xor g0(a, b, x);", "and g1(a, b, p);", "and g2(x, c, q);", "or g3(p, q, y);", "not g4(q, z);"], outputs="y, z")
    assert fuse3(text) == (text, (4, 4, 3, 3))


def test_an_inner_wire_read_by_a_dff_or_a_mux_is_not_fused():
    text = _module(["xor g0(a, b, n0);", "xor g1(n0, c, y);", "dff g2(n0, q);"], outputs="y, q")
    assert fuse3(text)[0] == text
    text = _module(["xor g0(a, b, n0);", "xor g1(n0, c, y);", "mux g2(a, b, n0, z);"], outputs="y, z")
    assert fuse3(text)[0] == text


@pytest.mark.parametrize("inner,outer,want", [("xor", "xor", "xor3"), ("xnor", "xor", "xnor3"), ("xor", "xnor", "xnor3"),
                                              ("xnor", "xnor", "xor3")])
@pytest.mark.parametrize("inner_first", [True, False])
def test_parity_combinations(inner, outer, want, inner_first):
    ops = "n0, c" if inner_first else "c, n0"
    text = _module([f"{inner} g0(a, b, n0);", f"{outer} g1({ops}, y);"])
    fused, stats = fuse3(text)
    assert _gate_lines(fused) == [f"{want} g1(a, b, c, y);"] and stats == (2, 1, 2, 1)
    _assert_equivalent(text, fused, [dict(zip("abcd", v)) for v in itertools.product((0, 1), repeat=4)])


@pytest.mark.parametrize("x_kw", ["xor", "or"])
@pytest.mark.parametrize("or_ops", ["p, q", "q, p"])
@pytest.mark.parametrize("q_ops", ["x, c", "c, x"])
@pytest.mark.parametrize("x_ops", ["a, b", "b, a"])
def test_carry_rule_operand_orders_and_both_forms_of_x(x_kw, or_ops, q_ops, x_ops):
    text = _module([f"{x_kw} g0({x_ops}, x);", "and g1(a, b, p);", f"and g2({q_ops}, q);", f"or g3({or_ops}, y);", "not g4(x, z);"],
                   outputs="y, z")
    fused, stats = fuse3(text)
    assert _gate_lines(fused) == [f"{x_kw} g0({x_ops}, x);", "maj g3(a, b, c, y);", "not g4(x, z);"]  # x stays
    assert stats == (4, 2, 3, 1)
    _assert_equivalent(text, fused, [dict(zip("abcd", v)) for v in itertools.product((0, 1), repeat=4)])


def test_a_fused_gate_reads_three_different_wires():
    """xor(xor(a, b), a) would become xor3(a, b, a): a enters the sum twice, 5 v instead of 3 v before the doubling, outside
    the noise budget stated for XOR3.  Such pairs, and a carry whose c is a or b, stay as they are."""
    for text in (_module(["xor g0(a, b, n0);", "xor g1(n0, a, y);"]), _module(["xnor g0(a, b, n0);", "xor g1(b, n0, y);"]),
                 _module(["xor g0(a, a, n0);", "xor g1(n0, c, y);"]),
                 _module(["xor g0(a, b, x);", "and g1(a, b, p);", "and g2(x, a, q);", "or g3(p, q, y);", "not g4(x, z);"],
                         outputs="y, z")):
        assert fuse3(text)[0] == text
    for text in (aes128(), alu_c880_class()):
        for line in _gate_lines(fuse3(text)[0]):
            if line.split()[0] in ("maj", "xor3", "xnor3"):
                ins = [a.strip() for a in line[line.index("(") + 1:line.rindex(")")].split(",")][:3]
                assert len(set(ins)) == 3, line


def test_untouched_gate_kinds_and_a_second_run():
    """and-or over something that is no xor / or of the same operands, nand / nor, mux and constants stay; the output of a
    run is a fixed point."""
    text = _module(["and g0(a, b, p);", "and g1(n9, c, q);", "nand g9(a, b, n9);", "or g2(p, q, y);",
                    "xor g3(a, b, n3);", "xor g4(n3, c, n4);", "xor g5(n4, d, z);", "cone g6(one);", "xor g7(one, a, w);"],
                   outputs="y, z, w")
    fused, stats = fuse3(text)
    assert _gate_lines(fused) == ["and g0(a, b, p);", "and g1(n9, c, q);", "nand g9(a, b, n9);", "or g2(p, q, y);",
                                  "xor3 g4(a, b, c, n4);", "xor g5(n4, d, z);", "cone g6(one);", "xor g7(one, a, w);"]
    assert fuse3(fused) == (fused, (stats[1], stats[1], stats[3], stats[3]))
    _assert_equivalent(text, fused, [dict(zip("abcd", v)) for v in itertools.product((0, 1), repeat=4)])


# ---------------------------------------------------------------------------------------------- bootstrap weights
def _host_shard_bounds(ops, world):
    import ctypes as C
    ops = np.ascontiguousarray(ops, dtype=np.int32)
    bounds = np.zeros(world + 1, dtype=np.int64)
    rows = H.host.helm_host_shard_bounds(ops.ctypes.data_as(C.POINTER(C.c_int32)), len(ops), world,
                                         bounds.ctypes.data_as(C.POINTER(C.c_int64)))
    return bounds.tolist(), int(rows)


def test_shard_cut_weighs_the_three_input_gates_as_one_bootstrap():
    """ops 0, 3, 6, 20, 21, 22 weigh 1, 2, 0, 1, 1, 1: bounds[r] is the first gate at which the bootstraps before it reach
    r / world of the total (shard_rule.h), worked out here from those weights."""
    weight = {AND: 1, MUX: 2, NOT: 0, MAJ3: 1, XOR3: 1, XNOR3: 1}
    for ops in ([AND, MUX, NOT, MAJ3, XOR3, XNOR3], [MAJ3, XOR3, XNOR3] * 5, [NOT, MAJ3, NOT, XNOR3, MUX, XOR3, AND] * 3):
        for world in (2, 3, 6):
            before = np.concatenate([[0], np.cumsum([weight[o] for o in ops])])
            want = [0] + [int(np.argmax(before * world >= before[-1] * r)) for r in range(1, world)] + [len(ops)]
            got, rows = _host_shard_bounds(ops, world)
            assert got == want and rows == max(np.diff(want)), (ops, world)
    assert _host_shard_bounds([AND, MUX, NOT, MAJ3, XOR3, XNOR3], 6)[0] == [0, 1, 2, 2, 4, 5, 6]


def test_launch_packing_weighs_the_three_input_gates_as_one_bootstrap():
    """One level of ops 0, 3, 6, 20, 21, 22 on rows of their own, quantum 4: the first launch takes 1 + 2 + 1 bootstraps -
    AND, MUX, MAJ3 - and the free NOT, the second XOR3 and XNOR3.  Five gates of one op at quantum 3: three and two for a
    one-bootstrap op (everything at once for a free one, four and one for a two-bootstrap one)."""
    ops = np.array([AND, MUX, NOT, MAJ3, XOR3, XNOR3], np.int32)
    i0, i1, i2 = np.zeros(6, np.int32), np.ones(6, np.int32), np.full(6, 2, np.int32)
    out = np.arange(3, 9, dtype=np.int32)
    packed = pack_levels(ops, i0, i1, i2, out, np.array([0, 6]), 4)
    assert packed[0].tolist() == ops.tolist() and packed[5].tolist() == [0, 4, 6]
    for op, want in ((MAJ3, [0, 3, 5]), (XOR3, [0, 3, 5]), (XNOR3, [0, 3, 5]), (AND, [0, 3, 5]), (NOT, [0, 5]), (MUX, [0, 4, 5])):
        packed = pack_levels(np.full(5, op, np.int32), i0[:5], i1[:5], i2[:5], out[:5], np.array([0, 5]), 3)
        assert packed[5].tolist() == want, op


# ---------------------------------------------------------------------------------------------- noise budget
def _variances(p, s_lwe, s_glwe):
    """The formulas of tests/test_gpu_noise.py (torus units, binary keys, balanced digits of variance (B^2 + 2) / 12):
    blind rotation, keyswitch, modulus switch."""
    B, Bk = 2.0 ** p.pbs_logB, 2.0 ** p.ks_logB
    br = p.n * (p.pbs_l * (p.k + 1) * p.N * ((B * B + 2) / 12) * s_glwe ** 2 + (1 + p.k * p.N / 2) / (24 * B ** (2 * p.pbs_l)))
    ks = p.k * p.N * p.ks_l * ((Bk * Bk + 2) / 12) * s_lwe ** 2 + p.k * p.N / (24 * Bk ** (2 * p.ks_l))
    ms = (1 + p.n / 2) / (48 * p.N * p.N)
    return br, ks, ms


def _log2_pfail(margin, variance):
    """two-sided Gaussian tail beyond `margin` as log2; erfc underflows near 2^-1070, the asymptotic form takes over"""
    x = margin / math.sqrt(2 * variance)
    v = math.erfc(x)
    return math.log2(v) if v > 0 else (-x * x - math.log(x * math.sqrt(math.pi))) / math.log(2)


def three_input_budget(name):
    p, s_lwe, s_glwe = helm_amd.named_params(name)
    br, ks, ms = _variances(p, s_lwe, s_glwe)
    v = br + ks
    return {"gate2": _log2_pfail(0.125, 2 * v + ms),      # a two-input gate on two gate outputs (the existing worst operand)
            "maj3": _log2_pfail(0.125, 3 * v + ms),       # MAJ3 on three gate outputs: margin 1/8
            "xor3": _log2_pfail(0.25, 12 * v + ms),       # XOR3 / XNOR3: the doubled sum of three, margin 1/4
            "v": v, "ms": ms}


@pytest.mark.parametrize("name", ["boolean_default", "helm_cuda", "boolean_tfhe_lib", "boolean_default_ks_pbs"])
def test_noise_budget_of_the_three_input_operands(name):
    b = three_input_budget(name)
    print(f"\n{name}: V_br + V_ks {b['v']:.3e}, V_ms {b['ms']:.3e}; failure probability 2-input gate 2^{b['gate2']:.1f}, "
          f"MAJ3 2^{b['maj3']:.1f}, XOR3 2^{b['xor3']:.1f}")
    assert b["maj3"] > b["gate2"] and b["maj3"] < 0 and b["xor3"] < 0  # one more term at the same margin costs something
    if name == "boolean_default":
        assert b["maj3"] < -100 and b["xor3"] < -100  # the sanity bound of the measured noise test
