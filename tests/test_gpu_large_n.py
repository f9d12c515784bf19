"""The large-N blind-rotate kernel of the 64-bit engine (k_pbs64_large, helm_amd/csrc/helm_pbs64_large.inc over
helm_pbs64_large_core.inc): k = 1, N = 4096, reached through SiServerKey(generic="large") = helm_si_ctx_create_ex with HELM_SI_CREATE_LARGE_N.  N = 4096 is the
smallest size at which the kernel exists, so n stays at 12 and the batches small.  Every comparison is word for word against
oracle.Oracle64(..., use_ntt=True); tests/many_lut.py and tests/saturation.py are imported as they are."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import helm_amd
import oracle
from helm_amd import ArithCircuit, Circuit, EvalCircuit, LutCircuit, PtxtType, verilog_parser

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import many_lut as ML  # noqa: E402
import saturation as S  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = os.path.join(ROOT, "tests", "netlists")
N = 4096

_keys = {}


def toy_key(l=1, logB=22, ks=(3, 5), seed=7):
    """si_toy_4096 (n = 12, message 4 x carry 8: t = 32) with another PBS or keyswitch decomposition."""
    key = (l, logB, ks, seed)
    if key not in _keys:
        p, lwe_std, glwe_std = helm_amd.si_named_params("si_toy_4096")
        p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = l, logB, ks[0], ks[1]
        _keys[key] = helm_amd.SiClientKey(p, lwe_std, glwe_std, seed=seed)
    return _keys[key]


def mask_word(a):
    """A word that modulus-switches to a (mod 2N)."""
    return np.uint64(a << (64 - N.bit_length()))


def large_key(ck, mode="large"):
    sk = helm_amd.SiServerKey(ck, generic=mode)
    assert sk.kernel_class() == "large" and sk.field_bits() == 50
    return sk


@pytest.mark.parametrize("l,logB", [(1, 22), (2, 15), (3, 8)])
def test_bootstraps_word_for_word(l, logB):
    ck = toy_key(l, logB)
    p, t = ck.params, ck.t
    assert t == 32
    with pytest.raises(helm_amd.HelmError, match="unsupported"):
        helm_amd.SiServerKey(ck)                    # the default entry point keeps refusing N = 4096
    with pytest.raises(helm_amd.HelmError, match="generic kernel"):
        helm_amd.SiServerKey(ck, generic="allow")   # ... and so does the generic domain
    sk = large_key(ck)
    assert sk.round_capacity() > 0
    orc = oracle.Oracle64(p.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
    rng = np.random.default_rng(100 * l + logB)
    vals = np.arange(t, dtype=np.uint64)
    honest = np.array([orc.keyswitch(c) for c in ck.encrypt(vals)], dtype=np.uint64)
    zero = rng.integers(0, 2**64, size=(1, p.n + 1), dtype=np.uint64)
    zero[0, :p.n] = 0                               # no step is active
    rand = rng.integers(0, 2**64, size=(6, p.n + 1), dtype=np.uint64)
    # the modulus-switched mask words and body hit 0, 1, N - 1, N, N + 1, 2N - 1: one row per value, all words alike (low
    # bits random, below the rounding), and one row that walks through all of them
    edges = [0, 1, N - 1, N, N + 1, 2 * N - 1]
    craft = np.stack([np.full(p.n + 1, mask_word(a), dtype=np.uint64) for a in edges] +
                     [np.array([mask_word(edges[(i + 1) % 6]) for i in range(p.n + 1)], dtype=np.uint64)])
    craft |= rng.integers(0, 2**49, size=craft.shape, dtype=np.uint64)
    for row, a in zip(craft, edges):
        assert all(S.modswitch(int(w), N, 64) == a for w in row)
    assert [S.modswitch(int(w), N, 64) for w in craft[6]] == [edges[(i + 1) % 6] for i in range(p.n + 1)]
    small = np.concatenate([honest, zero, rand, craft])
    f = [lambda x: (3 * x + 1) % t, lambda x: x * x % t]
    luts = np.stack([sk.make_lut(f[0]), sk.make_lut(f[1])])
    idx = (np.arange(len(small)) % 2).astype(np.int32)
    big = sk.pbs_batch(small, luts, idx)
    for g in range(len(small)):
        assert np.array_equal(big[g], orc.bootstrap(small[g], luts[idx[g]])), g
    assert [int(v) for v in ck.decrypt_message_and_carry(big[:t])] == [f[g % 2](g) for g in range(t)]
    sk.close()


def test_through_the_wire_table_and_a_lane():
    ck = toy_key()
    t = ck.t
    sk = large_key(ck, "allow+large")
    f = lambda x: (5 * x + 3) % t
    lut = sk.make_lut(f)[None]
    w = sk.wires(2 * t)
    w.upload(np.arange(t), ck.encrypt(np.arange(t, dtype=np.uint64)))
    w.apply_luts(np.arange(t), lut, np.arange(t) + t)
    out = w.download(np.arange(t) + t)
    assert [int(v) for v in ck.decrypt_message_and_carry(out)] == [f(v) for v in range(t)]
    rng = np.random.default_rng(3)
    small = rng.integers(0, 2**64, size=(9, ck.params.n + 1), dtype=np.uint64)
    idx = np.zeros(9, dtype=np.int32)
    lane = sk.fork()
    assert lane.kernel_class() == "large" and lane.generic == "allow+large" and lane.field_bits() == 50
    assert np.array_equal(lane.pbs_batch(small, lut, idx), sk.pbs_batch(small, lut, idx))
    sk.close()


@pytest.mark.parametrize("ks", [(3, 5), (8, 3)], ids=["ks3x5", "ks8x3"])
def test_keyswitch_at_in_dim_4096(ks):
    """40 rows: the vector-ALU kernel (its digit buffer is 4096 x ks_l x 4 B unsliced); 192 rows: the matrix-core kernel."""
    ck = toy_key(ks=ks, seed=11)
    sk = large_key(ck)
    orc = oracle.Oracle64(ck.params.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
    rng = np.random.default_rng(ks[0])
    for rows in (40, 192):
        src = rng.integers(0, 2**64, size=(rows, ck.dim + 1), dtype=np.uint64)
        src[:8] = ck.encrypt(np.arange(8, dtype=np.uint64))
        got = sk.keyswitch_batch(src)
        for g in range(rows):
            assert np.array_equal(got[g], orc.keyswitch(src[g])), (rows, g)
    sk.close()


@pytest.mark.parametrize("n_out", [2, 4])
def test_many_lut_every_output(n_out):
    """pbs_many_batch against tests/many_lut.py: the mask words of every output from the oracle's coefficient-0 output,
    the bodies from the exact integer route (one honest row, one row with a single active step), the zero-mask closed form,
    the oracle (output 0) and decryption (every output of the t / M >= 8 honest inputs)."""
    ck = toy_key()
    p, t = ck.params, ck.t
    sk = large_key(ck)
    orc = oracle.Oracle64(p.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
    shape = S.shape_of(p)
    M = ML.chunks(n_out)
    per = t // M
    assert per >= 8
    funcs = [lambda v, x=x: (3 * v + 5 * x + 1) % t for x in range(n_out)]
    tv = ML.many_lut_poly([[fn(v) for v in range(per)] for fn in funcs], t, N)
    assert np.array_equal(sk.make_many_lut(funcs), tv)
    rng = np.random.default_rng(n_out)
    honest = np.array([orc.keyswitch(c) for c in ck.encrypt(np.arange(per, dtype=np.uint64))], dtype=np.uint64)
    rand = np.zeros((1, p.n + 1), dtype=np.uint64)     # one active step, a random body
    rand[0, p.n // 2] = mask_word(N + 3)
    rand[0, p.n] = rng.integers(0, 2**64, dtype=np.uint64)
    bts = [0, 1, N - 1, N, 2 * N - 1]
    zero = np.zeros((len(bts), p.n + 1), dtype=np.uint64)
    for q, bt in enumerate(bts):
        zero[q, p.n] = mask_word(bt)
    small = np.concatenate([honest, rand, zero])
    exact_rows = [per - 1, per]     # the integer route (seconds per row): the last honest row and the single-step one
    got = sk.pbs_many_batch(small, tv, n_out)
    assert got.shape == (len(small), n_out, N + 1)
    for r in range(len(small)):
        out0 = orc.bootstrap(small[r], tv)
        acc = ML.accumulator_exact(small[r], tv, ck.bsk, shape, 1) if r in exact_rows else None
        for x in range(n_out):
            h = ML.output_coefficient(x, n_out, N)
            assert h == x * N // M
            assert np.array_equal(got[r, x, :N], ML.masks_from_output0(out0, 1, N, h)), (r, x, "mask words")
            if r > per:
                assert not got[r, x, :N].any()
                assert got[r, x, N] == ML.zero_mask_body(tv, bts[r - per - 1], h), (r, x, "zero-mask body")
            elif acc is not None:
                assert np.array_equal(got[r, x], ML.extract_at(acc, h)), (r, x, "exact route")
            elif x == 0:
                assert got[r, x, N] == out0[N], (r, "body of output 0")
    dec = ck.decrypt_message_and_carry(got[:per].reshape(-1, N + 1)).reshape(per, n_out)
    assert [[int(v) for v in row] for row in dec] == [[fn(v) for fn in funcs] for v in range(per)]
    sk.close()


def test_at_the_exactness_bound_both_signs():
    """tests/saturation.py's construction for (k, N, l, logB) = (1, 4096, 1, 22), all columns, under one key: the positive
    extreme, the negative extreme and the one-column variant.  The largest exact column-sum coefficient of the saturating
    step is 2^21 x 2 x 4096 x (2^63 - 1) (key words 2^63 - 1, all signs aligned) resp. x 2^63 (key words -2^63): 0.5469 of
    p0 p1 / 2 for the pair (FpG, FpI), as exact fractions; the shape's ceiling, (k+1) l N B/2 2^63, is the second of them.
    The kernel equals the Python-integer reference word for word, no tolerance."""
    ck = toy_key()
    shape = S.shape_of(ck.params)
    assert shape == S.Shape(12, 1, N, 1, 22)
    case = S.launch_case(shape, 64, ck.bsk)
    half = Fraction(S.FPG * S.FPI, 2)
    ceiling = Fraction(S.capacity_bound(shape, 64)) / half
    assert ceiling == Fraction(2**98, S.FPG * S.FPI) and Fraction(546, 1000) < ceiling < Fraction(548, 1000)
    fractions = [Fraction(pk) / half for pk in case["peak"]]
    print("fractions of p0 p1 / 2:", [float(v) for v in fractions])
    assert fractions[0] == Fraction(2**21 * 2 * N * (2**63 - 1)) / half     # positive extreme
    assert fractions[1] == ceiling                                           # negative extreme: words of -2^63
    assert fractions[2] == fractions[0]                                      # one column saturated
    assert all(Fraction(1, 2) <= v <= ceiling for v in fractions)
    orc = oracle.Oracle64(ck.params.as_tuple(), case["bsk"], ck.ksk, use_ntt=True)
    rng = np.random.default_rng(17)
    lwe = np.concatenate([case["lwe"], rng.integers(0, 2**64, size=(3, shape.n + 1), dtype=np.uint64)])
    tvs = np.stack([case["tv"], rng.integers(0, 2**64, size=N, dtype=np.uint64)])
    idx = np.array([0, 0, 0, 1, 0, 1], dtype=np.int32)
    sk = helm_amd.SiServerKey(params=ck.params, bsk=case["bsk"], ksk=ck.ksk, generic="large")
    assert sk.kernel_class() == "large"
    got = sk.pbs_batch(lwe, tvs, idx)
    assert np.array_equal(got[:3], case["ref"]), "the saturating rows differ from the integer reference"
    for g in range(len(lwe)):  # the oracle agrees on the saturating rows, and holds the honest controls under the same key
        assert np.array_equal(got[g], orc.bootstrap(lwe[g], tvs[idx[g]])), g
    sk.close()


def test_the_lds_edge_in_n():
    """n = 1024: the modulus-switched input takes its 2050 B of LDS.  A random key and random rows (no key generation);
    two rows against the oracle."""
    p, _, _ = helm_amd.si_named_params("si_toy_4096")
    p.n = 1024
    rng = np.random.default_rng(1024)
    bsk = rng.integers(0, 2**64, size=p.n * p.pbs_l * 4 * N, dtype=np.uint64)
    ksk = rng.integers(0, 2**64, size=N * p.ks_l * (p.n + 1), dtype=np.uint64)
    sk = helm_amd.SiServerKey(params=p, bsk=bsk, ksk=ksk, generic="large")
    assert sk.kernel_class() == "large"
    orc = oracle.Oracle64(p.as_tuple(), bsk, ksk, use_ntt=True)
    small = rng.integers(0, 2**64, size=(4, p.n + 1), dtype=np.uint64)
    luts = rng.integers(0, 2**64, size=(2, N), dtype=np.uint64)
    idx = np.array([0, 1, 1, 0], dtype=np.int32)
    got = sk.pbs_batch(small, luts, idx)
    for g in (0, 3):
        assert np.array_equal(got[g], orc.bootstrap(small[g], luts[idx[g]])), g
    sk.close()


def _circuit(path_or_text, is_arith, text=False):
    read = verilog_parser.read_verilog_text if text else verilog_parser.read_verilog_file
    gs, ws, ins, outs, d, _, _ = read(path_or_text, is_arith)
    c = Circuit(gs, ins, outs, d)
    c.sort_circuit()
    c.compute_levels()
    return c, ws


@pytest.mark.parametrize("bits", [0b101101, 0b010011])
def test_lut_mode_five_input_gates(bits):
    """tests/netlists/lut5-two-levels.v: five 5-input and two 3-input LUT gates over two levels.  Every wire equals the
    plaintext evaluator; one blind rotation per gate, without a wide-LUT key; many_lut=True changes nothing (2^5 = t: no
    two 5-input gates can share a rotation, and 2^3 x 2 <= t pairs need identical inputs, which this netlist has not)."""
    ck = toy_key()
    sk = large_key(ck)
    c, ws = _circuit(os.path.join(NET, "lut5-two-levels.v"), False)
    inputs = {name: PtxtType.Bool((bits >> i) & 1) for i, name in enumerate("abcdef")}
    ptxt = c.evaluate(c.initialize_wire_map(ws, inputs, "bool"))
    results = []
    for many in (False, True):
        lc = LutCircuit(ck, sk, c, many_lut=many)
        sk.timing_enable(True)
        sk.timing(reset=True)
        enc = EvalCircuit.evaluate_encrypted(lc, EvalCircuit.encrypt_inputs(lc, ws, inputs), 1, "bool")
        sk.sync()
        assert int(sk.timing().pbs_count) == 7 == lc.pbs_per_cycle()
        for wire, want in ptxt.items():
            assert ck.decrypt(enc[wire]) == int(bool(want)), (many, wire)
        results.append({wire: ck.decrypt(enc[wire]) for wire in ptxt})
        lc.set_many_lut(False)
    assert results[0] == results[1]
    sk.close()


def test_arithmetic_mode_known_answers():
    """FheUint8 answers through ArithCircuit on si_toy_4096 (message 4, carry 8); the first two look-up batches are
    recomputed by the oracle through the audit hook."""
    ck = toy_key(seed=13)
    sk = large_key(ck)
    orc = oracle.Oracle64(ck.params.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
    seen = {"luts": 0, "checked": 0, "bad": 0}

    def audit(rec):
        if rec["kind"] != "luts":
            return True
        seen["luts"] += 1
        if seen["luts"] <= 2:
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
    c, ws = _circuit(text, True, text=True)
    ac = ArithCircuit(ck, sk, c)
    out = ac.decrypt_outputs(ac.evaluate_encrypted(ac.encrypt_inputs(ws, {"A": PtxtType.U8(10), "B": PtxtType.U8(20)}), 1, "u8"), True)
    sk.set_audit(None)
    assert {k: int(v.value) for k, v in out.items()} == {"S": 30, "D": 10, "P": 200, "Q": 17, "R": 17}
    assert seen["checked"] > 0 and seen["bad"] == 0, seen
    sk.close()


def test_sharded_world_one_with_a_callback():
    """helm_si_set_exchange, world 1 with a callback: apply_luts runs stage -> collective -> scatter, in three rounds, and
    leaves the table of the unsharded call."""
    import torch
    from helm_amd import _native as nv
    torch.cuda.set_device(0)
    ck = toy_key()
    t = ck.t
    sk = large_key(ck)
    lut = sk.make_lut(lambda x: (7 * x + 2) % t)[None]
    cts = ck.encrypt(np.arange(t, dtype=np.uint64))

    def run():
        w = sk.wires(2 * t)
        w.upload(np.arange(t), cts)
        w.apply_luts(np.arange(t), lut, np.arange(t) + t)
        return w.download()

    plain = run()
    dev = torch.device("cuda", 0)
    sk.set_stream(torch.cuda.current_stream().cuda_stream)
    cap = 12
    stage = torch.zeros((cap, sk.dim + 1), dtype=torch.int64, device=dev)
    gather = torch.zeros((cap, sk.dim + 1), dtype=torch.int64, device=dev)
    calls = []

    def exchange(_user, rows):
        calls.append(int(rows))
        gather[:rows].copy_(stage[:rows])
        return 0

    fn = nv.SI_EXCHANGE_FN(exchange)
    nv.hip_check(nv.hip.helm_si_set_exchange(sk._h, 0, 1, 2, nv.vp(stage.data_ptr()), nv.vp(gather.data_ptr()), cap, fn, None))
    sharded = run()
    nv.hip_check(nv.hip.helm_si_set_exchange(sk._h, 0, 1, 1, None, None, 1, nv.SI_EXCHANGE_FN(0), None))
    assert calls == [12, 12, 8]
    assert np.array_equal(sharded, plain)
    assert [int(v) for v in ck.decrypt_message_and_carry(sharded[t:])] == [(7 * v + 2) % t for v in range(t)]
    sk.close()


def test_wop_refuses_a_large_pbs_side():
    from helm_amd import wopbs
    ck = toy_key()
    sk = large_key(ck)
    wp, _, _ = wopbs.wop_named_params("wop_toy_512")
    with pytest.raises(helm_amd.HelmError, match="large-N bootstrap kernel"):
        wopbs.WopServerKey(sk, params=wp)
    sk.close()


CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import helm_amd
res = {}
p, _, _ = helm_amd.si_named_params("si_toy_4096")
for mode in ("large", "force+large"):
    try:
        helm_amd.SiServerKey(params=p, generic=mode).close()
        res[mode] = "created"
    except helm_amd.HelmError as e:
        res[mode] = str(e)
sk = helm_amd.SiServerKey(params=helm_amd.si_named_params("si_toy_512")[0], generic="large")  # the tuned class is unaffected
res["tuned"] = sk.kernel_class()
sk.close()
print("RESULT " + json.dumps(res))
"""


def test_check_build_refuses_large_contexts_before_any_launch():
    """The bound-checking build runs the tuned kernels only: context creation refuses class 2 there, and launches nothing."""
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    env = dict(os.environ, HELM_HIP_LIB=lib)
    p = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert "bound-checking build" in res["large"] and "bound-checking build" in res["force+large"], res
    assert res["tuned"] == "tuned"


def test_full_size_shortint_m2c3():
    """The one slow test: the full-size 5-bit set from a fixed seed.  One round of 64 look-ups decrypts to f(v); two of its
    rows equal the oracle (keyswitch and bootstrap, about 4 s each on the CPU)."""
    ck = helm_amd.SiClientKey.generate("shortint_m2c3", seed=5)
    p, t = ck.params, ck.t
    assert (p.n, p.N, t) == (1024, N, 32)
    sk = large_key(ck)
    f = lambda x: (11 * x + 5) % t
    lut = sk.make_lut(f)[None]
    vals = np.arange(64, dtype=np.uint64) % t
    cts = ck.encrypt(vals)
    w = sk.wires(128)
    w.upload(np.arange(64), cts)
    w.apply_luts(np.arange(64), lut, np.arange(64) + 64)
    out = w.download(np.arange(64) + 64)
    assert [int(v) for v in ck.decrypt_message_and_carry(out)] == [f(int(v)) for v in vals]
    orc = oracle.Oracle64(p.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
    for g in (5, 63):
        assert np.array_equal(out[g], orc.bootstrap(orc.keyswitch(cts[g]), lut[0])), g
    sk.close()
