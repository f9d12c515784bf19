"""The two-prime blind-rotate kernel of the boolean engine (k_pbs_crt, helm_amd/csrc/helm_pbs_crt.inc), reached through
ServerKey(crt="allow" | "force") = helm_hip_ctx_create_ex: boolean shapes beyond the single-prime capacity bound - few, wide
decomposition levels - word for word against the oracle's EXACT route (tests/crt_shapes.py: the Goldilocks route is wrong
beyond column sums of 2^63, which these shapes reach), the same kernel forced onto single-prime shapes against the default
dispatch, crafted keys whose column sums pass 2^63 against the integer reference of tests/saturation.py, the launch edges, a
circuit through GateCircuit and through a device program, and the refusals."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helm_amd
import oracle
from helm_amd import Circuit, GateCircuit, PtxtType, verilog_parser
from helm_amd.distributed import level_arrays

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crt_shapes as X  # noqa: E402
import saturation as S  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = os.path.join(ROOT, "tests", "netlists")


def _bootstraps_word_for_word(ck, sk, orc, seed, cts=11, row0=None):
    """cts bootstraps through pbs_batch: an encryption of True (row0: a given one - every call of encrypt draws fresh
    randomness), an all-zero mask, random rows, two test vectors."""
    p = ck.params
    rng = np.random.default_rng(seed)
    lwe = rng.integers(0, 2**32, size=(cts, p.n + 1), dtype=np.uint32)
    lwe[0] = ck.encrypt(True) if row0 is None else row0
    lwe[3, :] = 0
    tvs = rng.integers(0, 2**32, size=(2, p.N), dtype=np.uint32)
    idx = (np.arange(cts) % 2).astype(np.int32)
    got = sk.pbs_batch(lwe, tvs, idx)
    for g in range(cts):
        assert np.array_equal(got[g], orc.bootstrap_noks(lwe[g], tvs[idx[g]])), g
    return got


@pytest.mark.parametrize("shape", X.SHAPES, ids=X.IDS)
def test_crt_shape_end_to_end(shape):
    ck = X.toy_key(shape)
    p = ck.params
    sk = helm_amd.ServerKey(ck, crt="allow")   # "capacity" without the flag; no such entry point before this kernel
    assert sk.kernel_class() == "crt" and sk.field_bits() == 98 and sk.short_root_stages() == 0
    qn, d = (p.k + 1) * p.pbs_l, sk.digit_batch()
    assert 1 <= d <= min(4, max(1, 1024 // p.N), qn)                     # tp_batch's cap
    if shape in X.PARTIAL_BATCH:
        assert d > 1 and qn % d != 0, (d, qn)                            # the partial last batch runs here
    rng = np.random.default_rng(1)
    polys = rng.integers(0, 2**32, size=(5, p.N), dtype=np.uint32)
    polys[3, :] = 0x80000000
    polys[4, ::2], polys[4, 1::2] = 0x7FFFFFFF, 0x80000000
    assert np.array_equal(sk.ntt_roundtrip(polys), polys)

    orc = X.exact_oracle(p, ck.bsk, ck.ksk)
    big = _bootstraps_word_for_word(ck, sk, orc, seed=shape[1] + shape[0])
    got = sk.keyswitch_batch(big)
    for g in range(len(big)):
        assert np.array_equal(got[g], orc.keyswitch(big[g])), g

    # one level: all six binary gates and MUX over both select values, word for word
    bits = np.array([0, 1, 0, 1, 0, 0, 1, 1, 1, 0], dtype=bool)
    ops = [oracle.AND, oracle.NAND, oracle.OR, oracle.NOR, oracle.XOR, oracle.XNOR, oracle.MUX, oracle.MUX]
    i0 = [0, 2, 4, 6, 0, 2, 4, 5]
    i1 = [1, 3, 5, 7, 3, 5, 6, 7]
    i2 = [-1] * 6 + [8, 9]   # select True, then False
    out = np.arange(10, 18, dtype=np.int32)
    w = sk.wires(18)
    ct = ck.encrypt(bits)
    w.upload(np.arange(10), ct)
    w.eval_gate_level(ops, i0, i1, i2, out)
    got = w.download()
    ref = np.zeros_like(got)
    ref[:10] = ct
    orc.eval_level(ref, ops, i0, i1, i2, out)
    assert np.array_equal(got, ref)
    # the truth table only where the ORACLE's rows decrypt to it (a shape with too few decomposition bits for its toy
    # noise - (1, 2048, 1, 9) has 9 - is word-for-word only)
    a, b = bits[i0], bits[i1]
    want = [a[0] & b[0], not (a[1] & b[1]), a[2] | b[2], not (a[3] | b[3]), a[4] ^ b[4], not (a[5] ^ b[5]),
            a[6] if bits[8] else b[6], a[7] if bits[9] else b[7]]
    if [bool(x) for x in ck.decrypt(ref[10:18])] == [bool(x) for x in want]:
        assert [bool(x) for x in ck.decrypt(got[10:18])] == [bool(x) for x in want]
    else:
        assert shape[2] * shape[3] < 12, "the oracle's own rows do not decrypt at a shape with 12 bits or more"
    assert sk.kernel_class() == "crt" and sk.field_bits() == 98
    sk.close()


FORCED = ["toy", "toy_k2", "toy_1024", "toy_1024_l2", (2, 512, 2, 7, 16)]


@pytest.mark.parametrize("which", FORCED, ids=[x if isinstance(x, str) else "k%d_N%d_l%d_B%d_n%d" % x for x in FORCED])
def test_forced_crt_kernel_on_single_prime_shapes(which):
    """crt="force" runs k_pbs_crt on shapes a single-prime kernel serves: the same rows as the default dispatch and as the
    oracle; the class still reflects the shape, the field is the pair."""
    ck = helm_amd.ClientKey.generate(which, seed=11) if isinstance(which, str) else X.toy_key(which)
    p = ck.params
    orc = X.exact_oracle(p, ck.bsk, ck.ksk)
    cls = "tuned" if isinstance(which, str) else "generic"
    sk = helm_amd.ServerKey(ck, crt="force")
    assert sk.kernel_class() == cls and sk.field_bits() == 98 and sk.short_root_stages() == 0
    row0 = ck.encrypt(True)
    forced = _bootstraps_word_for_word(ck, sk, orc, seed=50, row0=row0)
    polys = np.random.default_rng(2).integers(0, 2**32, size=(3, p.N), dtype=np.uint32)
    assert np.array_equal(sk.ntt_roundtrip(polys), polys)
    sk.close()
    for crt in (None, "allow"):   # "allow" changes nothing for a shape that fits the single prime
        sk = helm_amd.ServerKey(ck, crt=crt)
        assert sk.kernel_class() == cls and sk.field_bits() != 98
        default = _bootstraps_word_for_word(ck, sk, orc, seed=50, row0=row0)
        sk.close()
        assert np.array_equal(forced, default)


@pytest.mark.parametrize("sign", [+1, -1], ids=["pos", "neg"])
@pytest.mark.parametrize("shape", [(1, 256, 1, 31, 16), (2, 1024, 1, 23, 16), (3, 1024, 2, 15, 16)],
                         ids=["k1_N256_l1_B31", "k2_N1024_l1_B23", "k3_N1024_l2_B15"])
def test_at_the_bound(shape, sign):
    """tests/saturation.py: a key and a row under which one coefficient of every column sum reaches what the capacity bound
    allows, all terms of one sign.  For the first two shapes that passes 2^63 - the case a 64-bit lift or a Goldilocks
    reference gets wrong; the reference is the integer arithmetic of saturation.bootstrap_exact."""
    ck = X.toy_key(shape)
    p = ck.params
    case = S.saturating_case(S.shape_of(p), 32, sign=sign, base_key=ck.bsk)
    print("peak 2^%.2f of capacity bound 2^%.2f" % (np.log2(float(case["peak"])), np.log2(float(S.capacity_bound(S.shape_of(p), 32)))))
    if shape[:4] in ((1, 256, 1, 31), (2, 1024, 1, 23)):   # by construction: the bounds are 2^70 and 2^64.6
        assert case["peak"] > 1 << 63
    assert case["peak"] <= S.capacity_bound(S.shape_of(p), 32) < X.P0 * X.P1 // 2
    school = X.exact_oracle(p, case["bsk"], ck.ksk, saturating=True)
    assert np.array_equal(school.bootstrap_noks(case["lwe"], case["tv"]), case["ref"])
    sk = helm_amd.ServerKey(params=p, bsk=case["bsk"], ksk=ck.ksk, crt="allow")
    assert sk.kernel_class() == "crt" and sk.field_bits() == 98
    rng = np.random.default_rng(17)
    lwe = rng.integers(0, 2**32, size=(3, p.n + 1), dtype=np.uint32)   # controls: honest rows under the crafted key
    lwe[0] = case["lwe"]
    tvs = np.stack([case["tv"], rng.integers(0, 2**32, size=p.N, dtype=np.uint32)])
    idx = np.array([0, 1, 0], dtype=np.int32)
    got = sk.pbs_batch(lwe, tvs, idx)
    sk.close()
    bad = np.nonzero(got[0] != case["ref"])[0]
    assert len(bad) == 0, f"saturating row: {len(bad)} words differ, first at {bad[:4]}"
    for g in (1, 2):
        assert np.array_equal(got[g], school.bootstrap_noks(lwe[g], tvs[idx[g]])), g


def test_launch_edges():
    """count = 1, a full resident round, and one bootstrap more (a second round on one compute unit), at the LDS edge shape:
    eight distinct rows repeated, every output row checked against the oracle's eight."""
    shape = (3, 1024, 2, 15, 16)
    ck = X.toy_key(shape)
    p = ck.params
    sk = helm_amd.ServerKey(ck, crt="allow")
    q = sk.launch_quantum()
    import torch
    assert q > 0 and q % torch.cuda.get_device_properties(0).multi_processor_count == 0
    c = sk.launch_costs()
    assert c[3] == 1.0 and all(0 < c[i] <= c[i + 1] for i in range(3)), c
    orc = X.exact_oracle(p, ck.bsk, ck.ksk)
    rng = np.random.default_rng(8)
    base = rng.integers(0, 2**32, size=(8, p.n + 1), dtype=np.uint32)
    base[0] = ck.encrypt(False)
    tvs = rng.integers(0, 2**32, size=(2, p.N), dtype=np.uint32)
    want = np.stack([orc.bootstrap_noks(base[g], tvs[g % 2]) for g in range(8)])
    for count in (1, q, q + 1):
        rows = np.arange(count) % 8
        got = sk.pbs_batch(base[rows], tvs, (rows % 2).astype(np.int32))
        bad = np.nonzero((got != want[rows]).any(axis=1))[0]
        assert len(bad) == 0, f"count {count}: {len(bad)} rows differ, first {bad[:8]}"
    sk.close()


def test_two_bit_adder_under_toy_crt():
    """GateCircuit and a device program (helm_hip_program_run) on the two-prime kernel: every wire equal to the oracle's level
    evaluation, and decrypting to the plaintext evaluator's value."""
    ck = helm_amd.ClientKey.generate("toy_crt", seed=13)
    sk = helm_amd.ServerKey(ck, crt="allow")
    assert sk.kernel_class() == "crt"
    gates, wire_set, inputs, outputs, dffs, _, _ = verilog_parser.read_verilog_file(os.path.join(NET, "2-bit-adder.v"), False)
    circuit = Circuit(gates, inputs, outputs, dffs)
    circuit.sort_circuit()
    circuit.compute_levels()
    vals = {"a[0]": True, "a[1]": False, "b[0]": True, "b[1]": True, "cin": True}
    ptxt = {x: PtxtType.None_() for x in wire_set}
    ptxt.update({x: PtxtType.Bool(v) for x, v in vals.items()})
    ptxt = circuit.evaluate(ptxt)
    gc = GateCircuit(ck, sk, circuit)
    enc = gc.evaluate_encrypted(gc.encrypt_inputs(wire_set, {x: PtxtType.Bool(v) for x, v in vals.items()}), 1, "bool")
    names = list(inputs) + sorted(wire_set)
    index = {w: i for i, w in enumerate(names)}
    host = np.zeros((len(names), ck.params.n + 1), dtype=np.uint32)
    for wname in inputs:
        host[index[wname]] = enc[wname]
    # the oracle, level by level, from the evaluator's own input ciphertexts
    orc = X.exact_oracle(ck.params, ck.bsk, ck.ksk)
    ops, i0, i1, i2, out, off = level_arrays(circuit, index)
    dev = sk.wires(len(names))
    dev.upload(np.arange(len(names)), host)
    prog = helm_amd.Program(sk, ops, i0, i1, i2, out, off)
    prog.run(dev)
    for lv in range(len(off) - 1):
        s = slice(off[lv], off[lv + 1])
        orc.eval_level(host, ops[s], i0[s], i1[s], i2[s], out[s])
    got = dev.download()
    for wname in sorted(ptxt):
        assert np.array_equal(got[index[wname]], host[index[wname]]), wname        # program == oracle
        assert np.array_equal(enc[wname], host[index[wname]]), wname               # GateCircuit == oracle
        assert ck.decrypt(enc[wname]) == bool(ptxt[wname].value), wname            # == plaintext evaluator
    sk.close()


@pytest.mark.parametrize("k,N,l,logB", X.REFUSED_TODAY + [(2, 1024, 1, 23), (3, 512, 2, 10)])
def test_without_the_flag_the_shapes_are_refused_on_the_device(k, N, l, logB):
    ck = X.toy_key((k, N, l, logB, 16))
    with pytest.raises(helm_amd.HelmError, match="capacity"):
        helm_amd.ServerKey(ck)
    with pytest.raises(ValueError):
        helm_amd.ServerKey(ck, crt="yes")


@pytest.mark.parametrize("variant", [4, 5, 10])
def test_single_prime_variants_are_refused_on_a_crt_context(variant, monkeypatch):
    ck = X.toy_key((1, 256, 2, 12, 1))
    monkeypatch.setenv("HELM_HIP_PBS_VARIANT", str(variant))
    for crt in ("allow", "force"):
        with pytest.raises(helm_amd.HelmError, match="names a single-prime build"):
            helm_amd.ServerKey(ck, crt=crt)
    monkeypatch.setenv("HELM_HIP_PBS_VARIANT", "0")
    sk = helm_amd.ServerKey(ck, crt="allow")
    assert sk.kernel_class() == "crt"
    sk.close()


CHILD = r"""
import json, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import helm_amd
import crt_shapes as X
res = {}
ck = X.toy_key((1, 256, 2, 12, 1))
for crt in ("allow", "force"):
    try:
        helm_amd.ServerKey(ck, crt=crt)      # creation only: nothing is launched in this build
        res[crt] = "created"
    except helm_amd.HelmError as e:
        res[crt] = str(e)
ck2 = helm_amd.ClientKey.generate("toy", seed=1)
try:
    helm_amd.ServerKey(params=ck2.params, crt="force")
    res["force-toy"] = "created"
except helm_amd.HelmError as e:
    res["force-toy"] = str(e)
sk = helm_amd.ServerKey(params=ck2.params, crt="allow")   # a single-prime shape under "allow": an ordinary context
res["allow-toy"] = [sk.kernel_class(), sk.field_bits()]
sk.close()
print("RESULT " + json.dumps(res))
"""


def test_check_build_refuses_a_crt_context_at_creation():
    """The bound-counting build (libhelm_hip_check.so) does not run k_pbs_crt: it is built like k_pbs64_generic, whose
    counting build faulted for a cause not found.  The refusal comes at creation, before any launch, and says why."""
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    env = dict(os.environ, HELM_HIP_LIB=lib)
    p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for key in ("allow", "force", "force-toy"):
        assert "not available in the bound-checking build" in res[key] and "CRT" in res[key], res
    assert res["allow-toy"][0] == "tuned" and res["allow-toy"][1] in (49, 51)
