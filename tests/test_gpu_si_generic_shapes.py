"""The 64-bit engine's generic blind-rotate kernel (k_pbs64_generic, helm_amd/csrc/helm_pbs64_generic.inc): k, pbs_l and
pbs_logB at run time, reached through SiServerKey(generic="allow" | "force") = helm_si_ctx_create_ex.  Untuned shapes
bit-exact against the oracle's exact NTT route; the same kernel forced onto the tuned shapes, bit-identical to their tuned
kernels; LUT-mode and arithmetic-mode circuits on untuned shapes; the WoP path's and the check build's refusals."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helm_amd
import oracle
from helm_amd import ArithCircuit, Circuit, EvalCircuit, LutCircuit, PtxtType, verilog_parser

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = os.path.join(ROOT, "tests", "netlists")

# (k, N, pbs_l, pbs_logB), none of them a tuned shape; logB l >= 20 so that look-ups decrypt
SHAPES = [(2, 512, 2, 12), (2, 1024, 2, 12),
          (4, 512, 1, 22), (7, 512, 1, 22), (15, 256, 1, 22),   # (k+1) N = 4096 at k = 7 and 15: the LDS edge
          (3, 1024, 1, 21), (1, 2048, 3, 8),                    # (1, 2048): the edge at N = 2048
          (1, 256, 6, 5), (1, 256, 15, 2)]
IDS = [f"k{k}_N{N}_l{l}_B{b}" for k, N, l, b in SHAPES]


def toy_params(k, N, l, logB, n=12, msg=4, carry=4):
    p, _, _ = helm_amd.si_named_params("si_toy_512")
    p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = n, k, N, l, logB, 4, 4
    p.message_modulus, p.carry_modulus = msg, carry
    return p


def toy_key(shape, seed=7, **kw):
    return helm_amd.SiClientKey(toy_params(*shape, **kw), 1e-9, 1e-16 if shape[1] == 2048 else 1e-15, seed=seed)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_untuned_shape_end_to_end(shape):
    ck = toy_key(shape)
    p = ck.params
    with pytest.raises(helm_amd.HelmError, match="unsupported"):
        helm_amd.SiServerKey(ck)  # the default entry point keeps refusing it
    sk = helm_amd.SiServerKey(ck, generic="allow")
    assert sk.kernel_class() == "generic"
    assert sk.field_bits() == 49
    orc = oracle.Oracle64(p.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
    rng = np.random.default_rng(shape[0] * 10000 + shape[1] + shape[2])

    # bootstraps: encryptions of known values (through the oracle's keyswitch), an all-zero mask, random rows; two LUTs
    vals = np.arange(ck.t, dtype=np.uint64)
    small = np.array([orc.keyswitch(c) for c in ck.encrypt(vals)], dtype=np.uint64)
    small = np.concatenate([small, rng.integers(0, 2**64, size=(6, p.n + 1), dtype=np.uint64)])
    small[ck.t + 1, :p.n] = 0
    luts = np.stack([sk.make_lut(lambda x: (3 * x + 1) % ck.t), sk.make_lut(lambda x: x * x % ck.t)])
    idx = (np.arange(len(small)) % 2).astype(np.int32)
    big = sk.pbs_batch(small, luts, idx)
    for g in range(len(small)):
        assert np.array_equal(big[g], orc.bootstrap(small[g], luts[idx[g]])), g
    f = [lambda x: (3 * x + 1) % ck.t, lambda x: x * x % ck.t]
    assert [int(v) for v in ck.decrypt_message_and_carry(big[:ck.t])] == [f[g % 2](g) for g in range(ck.t)]

    # keyswitch: the vector-ALU kernel (below 160 rows) and the matrix-core one (160 and more)
    for rows in (40, 192):
        src = np.concatenate([big] * (rows // len(big) + 1))[:rows].copy()
        src[len(big):] ^= rng.integers(0, 2**64, size=src[len(big):].shape, dtype=np.uint64)
        got = sk.keyswitch_batch(src)
        for g in list(range(0, rows, 7)) + [rows - 1]:
            assert np.array_equal(got[g], orc.keyswitch(src[g])), (rows, g)

    # keyswitch + bootstrap through the wire table: decrypts to f(x)
    w = sk.wires(2 * ck.t)
    w.upload(np.arange(ck.t), ck.encrypt(vals))
    w.apply_luts(np.arange(ck.t), luts[:1], np.arange(ck.t) + ck.t)
    assert [int(v) for v in ck.decrypt_message_and_carry(w.download(np.arange(ck.t) + ck.t))] == \
        [f[0](v) for v in range(ck.t)]

    # a lane gives the same rows
    lane = sk.fork()
    assert lane.kernel_class() == "generic" and lane.generic == "allow"
    assert np.array_equal(lane.pbs_batch(small, luts, idx), big)
    sk.close()


@pytest.mark.parametrize("name", ["si_toy_512", "si_toy_512_k3", "si_toy_1024_k2", "si_toy_2048",
                                  "shortint_m2c2", "shortint_m1c1", "shortint_m2c1"])
def test_forced_generic_on_tuned_shapes_is_bit_identical(name):
    ck = helm_amd.SiClientKey.generate(name, seed=3)
    p = ck.params
    tuned = helm_amd.SiServerKey(ck)
    forced = helm_amd.SiServerKey(ck, generic="force")
    assert tuned.kernel_class() == "tuned" and forced.kernel_class() == "generic"
    assert forced.field_bits() == 49
    rows = forced.round_capacity()  # one full round of the generic kernel
    assert rows > 0
    rng = np.random.default_rng(5)
    small = rng.integers(0, 2**64, size=(rows, p.n + 1), dtype=np.uint64)
    small[:ck.t] = tuned.keyswitch_batch(ck.encrypt(np.arange(ck.t, dtype=np.uint64)))
    small[ck.t, :p.n] = 0
    luts = np.stack([tuned.make_lut(lambda x: (5 * x + 2) % ck.t), tuned.make_lut(lambda x: x // 2)])
    idx = rng.integers(0, 2, size=rows).astype(np.int32)
    got = forced.pbs_batch(small, luts, idx)
    assert np.array_equal(got, tuned.pbs_batch(small, luts, idx))
    orc = oracle.Oracle64(p.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
    check = np.unique(np.concatenate([np.arange(ck.t + 1), np.linspace(0, rows - 1, 40).astype(int)]))
    assert len(check) >= 32
    for g in check:
        assert np.array_equal(got[g], orc.bootstrap(small[g], luts[idx[g]])), g
    forced.close()
    tuned.close()


def test_forced_generic_refuses_multi_bit():
    ck_params, _, _ = helm_amd.si_named_params("shortint_m2c2_multibit3")
    with pytest.raises(helm_amd.HelmError, match="multi-bit"):
        helm_amd.SiServerKey(params=ck_params, generic="force")


def _circuit_file(path, is_arith):
    gs, ws, ins, outs, d, _, _ = verilog_parser.read_verilog_file(path, is_arith)
    c = Circuit(gs, ins, outs, d)
    c.sort_circuit()
    c.compute_levels()
    return c, ws


def test_lut_netlist_on_an_untuned_shape():
    """The 8-bit LUT-3-1 adder (t = 8) on k = 3, N = 1024: every output wire equals the plaintext evaluator."""
    ck = toy_key((3, 1024, 1, 21), seed=9, msg=4, carry=2)
    sk = helm_amd.SiServerKey(ck, generic="allow")
    assert sk.kernel_class() == "generic"
    c, ws = _circuit_file(os.path.join(NET, "8-bit-adder-lut-3-1.v"), False)
    a, b, cin = 0xB7, 0x6E, 1
    inputs = {f"a[{i}]": PtxtType.Bool((a >> i) & 1) for i in range(8)}
    inputs.update({f"b[{i}]": PtxtType.Bool((b >> i) & 1) for i in range(8)})
    inputs["cin"] = PtxtType.Bool(cin)
    ptxt = c.evaluate(c.initialize_wire_map(ws, inputs, "bool"))
    lc = LutCircuit(ck, sk, c)
    enc = EvalCircuit.evaluate_encrypted(lc, EvalCircuit.encrypt_inputs(lc, ws, inputs), 1, "bool")
    for wire, want in ptxt.items():
        assert ck.decrypt(enc[wire]) == int(bool(want)), wire
    sk.close()


def test_fheuint8_known_answers_on_an_untuned_shape():
    """K-7-style FheUint8 answers through ArithCircuit on k = 4, N = 512 (message = carry = 4), and look-up batches
    recomputed by the oracle through the audit hook."""
    ck = toy_key((4, 512, 1, 22), seed=11)
    sk = helm_amd.SiServerKey(ck, generic="allow")
    orc = oracle.Oracle64(ck.params.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
    seen = {"luts": 0, "checked": 0, "bad": 0}

    def audit(rec):
        if rec["kind"] != "luts":
            return True
        seen["luts"] += 1
        if seen["luts"] <= 2:  # the first two look-up batches in full
            want = orc.apply_luts(rec["in_rows"], rec["luts"], rec["lut_idx"])
            seen["checked"] += len(want)
            seen["bad"] += int(np.sum(~np.all(want == rec["out_rows"], axis=1)))
        return True

    sk.set_audit(audit)
    text = """input [7:0] A, B;
output [7:0] S, D, P, Q, R;
add g0(A, B, S);
sub g1(B, A, D);
mult g2(A, B, P);
add g3(A, 7, Q);
sub g4(B, 3, R);
"""
    gs, ws, ins, outs, d, _, _ = verilog_parser.read_verilog_text(text, True)
    c = Circuit(gs, ins, outs, d)
    c.sort_circuit()
    c.compute_levels()
    ac = ArithCircuit(ck, sk, c)
    out = ac.decrypt_outputs(ac.evaluate_encrypted(ac.encrypt_inputs(ws, {"A": PtxtType.U8(10), "B": PtxtType.U8(20)}), 1, "u8"), True)
    sk.set_audit(None)
    assert {k: int(v.value) for k, v in out.items()} == {"S": 30, "D": 10, "P": 200, "Q": 17, "R": 17}
    assert seen["checked"] > 0 and seen["bad"] == 0, seen
    sk.close()


CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import helm_amd
res = {}
p, _, _ = helm_amd.si_named_params("si_toy_512")
p.n, p.k, p.N, p.pbs_l, p.pbs_logB = 6, 7, 512, 1, 22
for mode in ("allow", "force"):
    try:
        helm_amd.SiServerKey(params=p if mode == "allow" else helm_amd.si_named_params("si_toy_512")[0], generic=mode).close()
        res[mode] = "created"
    except helm_amd.HelmError as e:
        res[mode] = str(e)
sk = helm_amd.SiServerKey(params=helm_amd.si_named_params("si_toy_512")[0])  # the tuned class is unaffected
res["tuned"] = sk.kernel_class()
sk.close()
print("RESULT " + json.dumps(res))
"""


def test_check_build_refuses_generic_contexts_before_any_launch():
    """The bound-checking build (-O0) does not run the generic kernel yet: context creation refuses
    the generic class there with a clear error, and launches nothing."""
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    env = dict(os.environ, HELM_HIP_LIB=lib)
    p = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert "bound-checking build" in res["allow"] and "bound-checking build" in res["force"], res
    assert res["tuned"] == "tuned"


def test_wop_refuses_a_generic_pbs_side():
    from helm_amd import wopbs
    ck = helm_amd.SiClientKey.generate("si_toy_512", seed=5)
    wp, c, d = wopbs.wop_named_params("wop_toy_512")
    wk = wopbs.WopClientKey(ck, wp, c, d, seed=6)
    sk = helm_amd.SiServerKey(ck, generic="force")
    with pytest.raises(helm_amd.HelmError, match="generic"):
        wopbs.WopServerKey(sk, wk)
    sk.close()
    # the tuned context of the same key still builds one
    sk = helm_amd.SiServerKey(ck)
    wopbs.WopServerKey(sk, wk).close()
    sk.close()
