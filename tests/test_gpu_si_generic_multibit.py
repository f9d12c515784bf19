"""The multi-bit form of the 64-bit engine's generic blind-rotate kernel (k_pbs64_generic<LOGN, g>,
helm_amd/csrc/helm_pbs64_generic.inc), reached through SiServerKey(generic="allow+multibit" | "force+multibit") =
helm_si_ctx_create_ex with HELM_SI_CREATE_GENERIC_MULTIBIT.  Untuned multi-bit shapes bit-exact against the oracle's exact NTT
route, on rows that reach the group step's corners (no rotation at all, subset sums that wrap past 2N); the same kernel forced
onto the tuned multi-bit sets, bit-identical to k_pbs64s; the load-time capacity check; arithmetic mode on an untuned multi-bit
shape; the check build's refusal."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helm_amd
import oracle
from helm_amd import ArithCircuit, Circuit, PtxtType, verilog_parser
from helm_amd import _native as nv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (k, N, pbs_l, pbs_logB, grouping_factor): none of them served by the tuned multi-bit build (k = 1, pbs_l = 1, N >= 1024)
SHAPES = [(2, 512, 2, 12, 3),
          (3, 512, 1, 18, 2),    # the 1+1-bit family's shape
          (1, 256, 3, 7, 3),     # (k+1) l = 6 digit polynomials against D = 4: a partial digit batch
          (7, 512, 1, 22, 2),    # (k+1) N = 4096: the LDS edge
          (1, 2048, 2, 14, 2),   # D = 1; a tuned classical shape without a tuned multi-bit form
          (1, 512, 1, 20, 3)]    # likewise
IDS = [f"k{k}_N{N}_l{l}_B{b}_g{g}" for k, N, l, b, g in SHAPES]


def toy_params(k, N, l, logB, g, n=12, msg=4, carry=4):
    p, _, _ = helm_amd.si_named_params("si_toy_512")
    p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = n, k, N, l, logB, 4, 4
    p.message_modulus, p.carry_modulus, p.grouping_factor = msg, carry, g
    return p


def toy_key(shape, seed=7, **kw):
    return helm_amd.SiClientKey(toy_params(*shape, **kw), 1e-9, 1e-16 if shape[1] == 2048 else 1e-15, seed=seed)


def mask_word(a, N):
    """A mask word that modulus-switches to a (mod 2N)."""
    return np.uint64(a << (64 - (N.bit_length() - 1) - 1))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_untuned_multi_bit_shape_end_to_end(shape):
    ck = toy_key(shape)
    p = ck.params
    N, g, n = p.N, p.grouping_factor, p.n
    with pytest.raises(helm_amd.HelmError):
        helm_amd.SiServerKey(ck)  # the default entry point keeps refusing it
    with pytest.raises(helm_amd.HelmError, match="multi-bit"):
        helm_amd.SiServerKey(ck, generic="allow")
    sk = helm_amd.SiServerKey(ck, generic="allow+multibit")
    assert sk.kernel_class() == "generic"
    assert sk.field_bits() == 49
    assert sk.round_capacity() > 0
    orc = oracle.Oracle64(p.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
    rng = np.random.default_rng(shape[0] * 10000 + shape[1] + shape[2])

    vals = np.arange(ck.t, dtype=np.uint64)
    small = np.array([orc.keyswitch(c) for c in ck.encrypt(vals)], dtype=np.uint64)
    small = np.concatenate([small, rng.integers(0, 2**64, size=(7, n + 1), dtype=np.uint64)])
    t = ck.t
    small[t + 1, :n] = 0                       # every group has e = 0: no step is skipped
    small[t + 2, g:2 * g] = 0                  # one group without rotation between groups with
    small[t + 3, :n] = mask_word(2 * N - 1, N)  # subset sums wrap past 2N
    small[t + 4, :n] = np.resize([mask_word(N, N), mask_word(1, N), mask_word(2 * N - 1, N)], n)  # N, 1, 2N - 1 in a group
    fs = [lambda x: (3 * x + 1) % ck.t, lambda x: x * x % ck.t]
    luts = np.stack([sk.make_lut(f) for f in fs])
    idx = (np.arange(len(small)) % 2).astype(np.int32)
    big = sk.pbs_batch(small, luts, idx)
    for r in range(len(small)):
        assert np.array_equal(big[r], orc.bootstrap(small[r], luts[idx[r]])), r
    assert [int(v) for v in ck.decrypt_message_and_carry(big[:t])] == [fs[r % 2](r) for r in range(t)]

    # keyswitch + bootstrap through the wire table: decrypts to f(x)
    w = sk.wires(2 * t)
    w.upload(np.arange(t), ck.encrypt(vals))
    w.apply_luts(np.arange(t), luts[:1], np.arange(t) + t)
    assert [int(v) for v in ck.decrypt_message_and_carry(w.download(np.arange(t) + t))] == [fs[0](v) for v in range(t)]

    # a lane gives the same rows
    lane = sk.fork()
    assert lane.kernel_class() == "generic" and lane.generic == "allow+multibit"
    assert np.array_equal(lane.pbs_batch(small, luts, idx), big)
    sk.close()


def _forced_against_tuned(ck, oracle_rows):
    """One full round of the forced generic kernel against the tuned multi-bit kernel, row for row; `oracle_rows` rows spread
    over the round, the all-zero-mask row among them, against the oracle."""
    p = ck.params
    tuned = helm_amd.SiServerKey(ck, generic="allow+multibit")  # the tuned multi-bit build serves the shape: unchanged
    forced = helm_amd.SiServerKey(ck, generic="force+multibit")
    assert tuned.kernel_class() == "tuned" and forced.kernel_class() == "generic"
    assert forced.field_bits() == 49
    rows = forced.round_capacity()
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
    check = np.unique(np.concatenate([[ck.t, 0, rows - 1], np.linspace(0, rows - 1, oracle_rows).astype(int)]))
    assert len(check) >= oracle_rows
    for r in check:
        assert np.array_equal(got[r], orc.bootstrap(small[r], luts[idx[r]])), r
    assert [int(v) for v in ck.decrypt_message_and_carry(got[:ck.t])] == \
        [[(5 * x + 2) % ck.t, x // 2][idx[x]] for x in range(ck.t)]
    forced.close()
    tuned.close()


@pytest.mark.parametrize("name", ["si_toy_1024_mb2", "si_toy_2048_mb3"])
def test_forced_generic_on_tuned_multi_bit_sets_is_bit_identical(name):
    _forced_against_tuned(helm_amd.SiClientKey.generate(name, seed=3), 16)


def test_forced_generic_on_the_full_multibit3_set():
    """The reference's arithmetic-mode set at full size (n = 888, g = 3, 296 group steps): one round (256 bootstraps) of the
    forced generic kernel equals the tuned kernel on every row, four rows against the oracle.
    Measured on the MI355X box: 1.6 s for the whole test (the round takes 42 ms on the generic kernel and 7 ms on the tuned
    one; the rest is key generation, shared in kind with
    test_gpu_shortint.py::test_full_parameter_set_multibit3, and the four oracle rows)."""
    ck = helm_amd.SiClientKey.generate("shortint_m2c2_multibit3", seed=1)
    assert ck.params.grouping_factor == 3 and ck.params.n == 888
    _forced_against_tuned(ck, 4)


def test_load_time_capacity_check():
    """k = 1, N = 2048, g = 3 at pbs_logB = 22 passes the creation-time bound (2 x 2048 x 2^21 x 2^63 = 2^96), but a uniformly
    random key's group sums reach 16 x 2048 x 2^62 x 2^21 = 2^98 > p0 p1 / 2 = 2^97.49: the load refuses it, the context stays
    without a key and launches nothing.  At pbs_logB = 21 the same kind of key is at 0.71 of the limit, loads and runs
    bit-exact."""
    rng = np.random.default_rng(11)
    p = toy_params(1, 2048, 1, 22, 3, n=6)
    bsk = rng.integers(0, 2**64, size=(6 // 3) * 8 * 1 * 4 * 2048, dtype=np.uint64)
    ksk = rng.integers(0, 2**64, size=1 * 2048 * p.ks_l * (p.n + 1), dtype=np.uint64)
    sk = helm_amd.SiServerKey(params=p, generic="force+multibit")  # (the tuned multi-bit build serves this shape)
    assert sk.kernel_class() == "generic"
    rc = nv.hip.helm_si_load_bootstrap_key(sk._h, nv.as_u64p(bsk), bsk.size)
    assert rc == -1 and b"capacity" in nv.hip.helm_hip_last_error()
    small = rng.integers(0, 2**64, size=(3, p.n + 1), dtype=np.uint64)
    lut = sk.make_lut(lambda x: x)
    with pytest.raises(helm_amd.HelmError, match="error -4"):  # HELM_ERR_STATE: no key is loaded
        sk.pbs_batch(small, lut)
    sk.close()

    p = toy_params(1, 2048, 1, 21, 3, n=6)
    sk = helm_amd.SiServerKey(params=p, bsk=bsk, ksk=ksk, generic="force+multibit")
    assert sk.kernel_class() == "generic"
    orc = oracle.Oracle64(p.as_tuple(), bsk, ksk, use_ntt=True)
    small[1, :p.n] = 0
    big = sk.pbs_batch(small, lut)
    for r in range(len(small)):
        assert np.array_equal(big[r], orc.bootstrap(small[r], lut)), r
    sk.close()


def test_fheuint8_known_answers_on_an_untuned_multi_bit_shape():
    """K-7-style FheUint8 answers through ArithCircuit on k = 2, N = 1024, g = 3 (message = carry = 4), and the first two
    look-up batches recomputed by the oracle through the audit hook."""
    ck = toy_key((2, 1024, 1, 21, 3), seed=11)
    sk = helm_amd.SiServerKey(ck, generic="allow+multibit")
    assert sk.kernel_class() == "generic"
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
p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.grouping_factor = 6, 3, 512, 1, 18, 2
for mode, params in (("allow+multibit", p), ("force+multibit", helm_amd.si_named_params("si_toy_1024_mb2")[0])):
    try:
        helm_amd.SiServerKey(params=params, generic=mode).close()
        res[mode] = "created"
    except helm_amd.HelmError as e:
        res[mode] = str(e)
sk = helm_amd.SiServerKey(params=helm_amd.si_named_params("si_toy_1024_mb2")[0], generic="allow+multibit")
res["tuned"] = sk.kernel_class()  # the tuned multi-bit class is unaffected
sk.close()
print("RESULT " + json.dumps(res))
"""


def test_check_build_refuses_generic_multi_bit_contexts_before_any_launch():
    """The bound-checking build does not run the generic kernel, its multi-bit form included: context
    creation refuses there with a clear error, and launches nothing."""
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    env = dict(os.environ, HELM_HIP_LIB=lib)
    p = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert "bound-checking build" in res["allow+multibit"] and "bound-checking build" in res["force+multibit"], res
    assert res["tuned"] == "tuned"
