"""The generic blind-rotate kernel (k_pbs_generic, helm_amd/csrc/helm_pbs_generic.inc): k and pbs_l at run time, so any
boolean shape with N in {256, 512, 1024, 2048}, (k+1) N <= 8192 and the single-prime capacity bound runs - not only the five
(N, k, pbs_l) shapes of the tuned builds.  Each shape below is outside that whitelist; each has at least 12 bits of
decomposition precision so that the truth tables decrypt.  Bit-exact against the oracle (its NTT routes are shape-generic),
and the same kernel forced onto the tuned shapes (HELM_HIP_PBS_VARIANT=10) against the oracle and the default dispatch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helm_amd
import oracle
from helm_amd import Circuit, GateCircuit, PtxtType, verilog_parser

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = os.path.join(ROOT, "tests", "netlists")

# (k, N, pbs_l, pbs_logB): bound (k+1) l N 2^(logB-1) 2^31 below p/2 = 2^49.6 for p = 6432^4 + 1
SHAPES = [(3, 256, 2, 8),    # 2^49.0  small N, k = 3
          (4, 256, 3, 6),    # 2^47.9  the largest k at N = 256
          (2, 512, 2, 7),    # 2^48.6  a tuned N with an untuned (k, l)
          (2, 1024, 2, 6),   # 2^48.6  k = 2 at N = 1024
          (1, 2048, 3, 5),   # 2^48.6  N = 2048
          # logB (l-1) >= 24: the carried decomposition state passes 2^23, where a 24-bit digit multiply goes wrong
          (1, 1024, 5, 6),   # 2^49.3  logB (l-1) = 24
          (1, 256, 13, 2),   # 2^45.7  logB (l-1) = 24
          (1, 256, 31, 1)]   # 2^45.0  logB l = 31, the decomposition's limit
IDS = [f"k{k}_N{N}_l{l}_B{b}" for k, N, l, b in SHAPES]
TUNED = ["toy", "toy_k2", "toy_1024", "toy_1024_l2"]


def toy_params(k, N, l, logB, n=16):
    p, _, _ = helm_amd.named_params("toy")
    p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = n, k, N, l, logB, 4, 4
    return p


def toy_key(shape, seed=7):
    return helm_amd.ClientKey(toy_params(*shape), 1e-7, 1e-9, seed=seed)


def n_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _bootstraps_bit_exact(ck, sk, seed, cts=11):
    """cts bootstraps through pbs_batch: an encryption of True, an all-zero mask, random rows, both test vectors."""
    p = ck.params
    orc = oracle.Oracle(p.as_tuple7(), ck.bsk, ck.ksk, use_ntt=True)
    rng = np.random.default_rng(seed)
    lwe = rng.integers(0, 2**32, size=(cts, p.n + 1), dtype=np.uint32)
    lwe[0] = ck.encrypt(True)
    lwe[3, :] = 0
    tvs = rng.integers(0, 2**32, size=(2, p.N), dtype=np.uint32)
    idx = (np.arange(cts) % 2).astype(np.int32)
    got = sk.pbs_batch(lwe, tvs, idx)
    for g in range(cts):
        assert np.array_equal(got[g], orc.bootstrap_noks(lwe[g], tvs[idx[g]])), g
    return orc, got


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_generic_shape_end_to_end(shape):
    ck = toy_key(shape)
    p = ck.params
    sk = helm_amd.ServerKey(ck)  # refused as "unsupported" before the generic kernel existed
    assert sk.kernel_class() == "generic"
    assert sk.field_bits() == 51
    rng = np.random.default_rng(1)
    polys = rng.integers(0, 2**32, size=(5, p.N), dtype=np.uint32)
    assert np.array_equal(sk.ntt_roundtrip(polys), polys)

    orc, big = _bootstraps_bit_exact(ck, sk, seed=shape[1] + shape[0])
    got = sk.keyswitch_batch(big)
    for g in range(len(big)):
        assert np.array_equal(got[g], orc.keyswitch(big[g])), g

    # one level: all six binary gates and MUX over both select values, bit-exact and decrypting to the truth tables
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
    a, b = bits[i0], bits[i1]
    want = [a[0] & b[0], not (a[1] & b[1]), a[2] | b[2], not (a[3] | b[3]), a[4] ^ b[4], not (a[5] ^ b[5]),
            a[6] if bits[8] else b[6], a[7] if bits[9] else b[7]]
    assert [bool(x) for x in ck.decrypt(got[10:18])] == [bool(x) for x in want]
    assert sk.field_bits() == 51
    sk.close()


@pytest.mark.parametrize("name", TUNED)
def test_generic_kernel_on_tuned_shapes(name, monkeypatch):
    """HELM_HIP_PBS_VARIANT=10 runs the generic kernel on a tuned shape (its own key layout, FpH); the class still says
    "tuned" - it reflects the shape."""
    monkeypatch.setenv("HELM_HIP_PBS_VARIANT", "10")
    ck = helm_amd.ClientKey.generate(name, seed=11)
    sk = helm_amd.ServerKey(ck)
    assert sk.kernel_class() == "tuned"
    assert sk.field_bits() == 51
    _bootstraps_bit_exact(ck, sk, seed=50)
    polys = np.random.default_rng(2).integers(0, 2**32, size=(3, ck.params.N), dtype=np.uint32)
    assert np.array_equal(sk.ntt_roundtrip(polys), polys)
    sk.close()


@pytest.mark.parametrize("name", ["boolean_default", "helm_cuda"])
def test_full_size_variant_10_equals_default_dispatch(name, monkeypatch):
    """One launch of 3 CUs + 5 bootstraps (a lockstep round plus remainder builds under the default dispatch): the generic
    kernel gives the same rows."""
    ck = helm_amd.ClientKey.generate(name, seed=21)
    p = ck.params
    count = 3 * n_cus() + 5
    rng = np.random.default_rng(4)
    lwe = rng.integers(0, 2**32, size=(count, p.n + 1), dtype=np.uint32)
    lwe[:16] = ck.encrypt(rng.integers(0, 2, size=16).astype(bool))
    tvs = rng.integers(0, 2**32, size=(2, p.N), dtype=np.uint32)
    idx = rng.integers(0, 2, size=count).astype(np.int32)
    sk = helm_amd.ServerKey(ck)
    want = sk.pbs_batch(lwe, tvs, idx)
    sk.close()
    monkeypatch.setenv("HELM_HIP_PBS_VARIANT", "10")
    sk10 = helm_amd.ServerKey(ck)
    got = sk10.pbs_batch(lwe, tvs, idx)
    sk10.close()
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} rows differ, first {bad[:8]}"


def test_full_size_generic_shape_against_the_fp_oracle():
    """n = 722, k = 2, N = 1024, l = 2, logB = 6 (bound 2^48.6) with boolean_default's keyswitch and noise: one launch of
    3 CUs + 5 bootstraps (more than one resident round of the generic kernel: launch_quantum() is its occupancy x CUs).
    Checked rows: 64 - the first 16, the last 16 (inside the launch's last, partial round) and 32 spread over the rest -
    against the oracle's fp route (exact in its 51-bit prime for this set)."""
    p, lwe_std, glwe_std = helm_amd.named_params("boolean_default")
    p.k, p.N, p.pbs_l, p.pbs_logB = 2, 1024, 2, 6
    ck = helm_amd.ClientKey(p, lwe_std, glwe_std, seed=31)
    sk = helm_amd.ServerKey(ck)
    assert sk.kernel_class() == "generic" and sk.field_bits() == 51
    count = 3 * n_cus() + 5
    assert count > sk.launch_quantum()
    rng = np.random.default_rng(9)
    bits = rng.integers(0, 2, size=count).astype(bool)
    lwe = ck.encrypt(bits)
    lwe[5, :] = 0
    tv = np.full(p.N, 0x20000000, dtype=np.uint32)
    got = sk.pbs_batch(lwe, tv[None, :])
    sk.close()
    rows = np.unique(np.concatenate([np.arange(16), np.arange(count - 16, count), np.linspace(16, count - 17, 32).astype(int)]))
    assert len(rows) == 64
    orc = oracle.Oracle(p.as_tuple7(), ck.bsk, ck.ksk, use_ntt=False, use_fp=True)
    want = orc.bootstrap_noks_fp(lwe[rows], tv)
    for r, g in enumerate(rows):
        assert np.array_equal(got[g], want[r]), g
    # the bootstrapped rows decrypt under the big key to the input bits (test vector +1/8 everywhere: the sign of the
    # output's phase is the input's; the all-zero row has phase 0 -> +1/8)
    bits[5] = True
    ph = ck.phase(got[rows], big=True).view(np.int32)
    assert np.array_equal(ph > 0, bits[rows])


def _circuit(path):
    gates, wire_set, inputs, outputs, dffs, _, _ = verilog_parser.read_verilog_file(path, False)
    c = Circuit(gates, inputs, outputs, dffs)
    c.sort_circuit()
    c.compute_levels()
    return c, wire_set, inputs


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=[IDS[1], IDS[3]])
def test_circuits_on_generic_shapes(shape):
    ck = toy_key(shape, seed=13)
    sk = helm_amd.ServerKey(ck)
    q = sk.launch_quantum()
    assert q > 0 and q % n_cus() == 0
    c = sk.launch_costs()
    assert c[3] == 1.0 and all(0 < c[i] <= c[i + 1] for i in range(3)), c
    rng = np.random.default_rng(3)
    for net in ("2-bit-adder.v", "8-bit-adder.v"):
        circuit, wire_set, inputs = _circuit(os.path.join(NET, net))
        vals = {x: bool(rng.integers(0, 2)) for x in inputs}
        ptxt = {x: PtxtType.None_() for x in wire_set}
        ptxt.update({x: PtxtType.Bool(v) for x, v in vals.items()})
        ptxt = circuit.evaluate(ptxt)
        gc = GateCircuit(ck, sk, circuit)
        enc = gc.evaluate_encrypted(gc.encrypt_inputs(wire_set, {x: PtxtType.Bool(v) for x, v in vals.items()}), 1, "bool")
        for name in sorted(ptxt):
            assert ck.decrypt(enc[name]) == bool(ptxt[name].value), (net, name)
    sk.close()


@pytest.mark.parametrize("name", ["toy", "toy_k2", "toy_1024", "toy_1024_l2", "boolean_default", "helm_cuda"])
def test_tuned_shapes_keep_the_tuned_class(name):
    ck = helm_amd.ClientKey.generate(name, seed=1)
    sk = helm_amd.ServerKey(ck)
    assert sk.kernel_class() == "tuned"
    assert sk.launch_quantum() == 4 * n_cus()
    sk.close()


CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, %r)
import helm_amd, oracle
SHAPES = %r
res = {}
def key(k, N, l, b):
    p, _, _ = helm_amd.named_params("toy")
    p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = 16, k, N, l, b, 4, 4
    return helm_amd.ClientKey(p, 1e-7, 1e-9, seed=3)
for shape in SHAPES:
    ck = key(*shape)
    sk = helm_amd.ServerKey(ck)
    sk.bound_violations(reset=True)
    p = ck.params
    rng = np.random.default_rng(1)
    B = 9
    # one launch wider than a resident round for the k = 2, N = 1024 shape
    if shape == (2, 1024, 2, 6):
        B = sk.launch_quantum() + 5
    lwe = rng.integers(0, 2**32, size=(B, p.n + 1), dtype=np.uint32)
    lwe[0] = ck.encrypt(True)
    lwe[1, :] = 0
    tvs = rng.integers(0, 2**32, size=(2, p.N), dtype=np.uint32)
    idx = (np.arange(B) %% 2).astype(np.int32)
    got = sk.pbs_batch(lwe, tvs, idx)
    polys = rng.integers(0, 2**32, size=(3, p.N), dtype=np.uint32)
    rt = bool(np.array_equal(sk.ntt_roundtrip(polys), polys))
    orc = oracle.Oracle(p.as_tuple7(), ck.bsk, ck.ksk, use_ntt=True)
    exact = all(np.array_equal(got[g], orc.bootstrap_noks(lwe[g], tvs[idx[g]])) for g in (0, 1, 2, B - 1))
    res[str(shape)] = {"count": int(B), "exact": bool(exact), "roundtrip": rt, "violations": sk.bound_violations(),
                       "class": sk.kernel_class()}
    sk.close()
print("RESULT " + json.dumps(res))
"""


@pytest.mark.parametrize("variant", [4, 5, 6, 7, 9])
def test_tuned_variants_are_refused_on_generic_shapes(variant, monkeypatch):
    """HELM_HIP_PBS_VARIANT naming a tuned build has nothing to force on a shape without one: an error, not a silent
    substitute; 10 (the generic kernel) is accepted.  A generic context reports no short-root stages (plain radix-2)."""
    ck = toy_key(SHAPES[0])
    monkeypatch.setenv("HELM_HIP_PBS_VARIANT", str(variant))
    with pytest.raises(helm_amd.HelmError, match="names a tuned build"):
        helm_amd.ServerKey(ck)
    monkeypatch.setenv("HELM_HIP_PBS_VARIANT", "10")
    sk = helm_amd.ServerKey(ck)
    assert sk.kernel_class() == "generic" and sk.short_root_stages() == 0
    sk.close()
    monkeypatch.delenv("HELM_HIP_PBS_VARIANT")
    ck = helm_amd.ClientKey.generate("toy_k2", seed=1)
    sk = helm_amd.ServerKey(ck)
    assert sk.short_root_stages() == 2
    sk.close()


def test_check_build_counts_no_violation_in_the_generic_kernel():
    """The check build (libhelm_hip_check.so, -DHELM_CHECK_BOUNDS: mulmod / reduce operands and lifted values counted by the
    kernels) over every shape of the table, one of them with a launch wider than a resident round: zero violations."""
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    env = dict(os.environ, HELM_HIP_LIB=lib)
    p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, SHAPES)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert len(res) == len(SHAPES)
    for shape, r in res.items():
        assert r["class"] == "generic" and r["exact"] and r["roundtrip"], (shape, r)
        assert r["violations"] == [0] * 8, (shape, r["violations"])
    assert res[str((2, 1024, 2, 6))]["count"] > 256
