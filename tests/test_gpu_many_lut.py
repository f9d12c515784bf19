"""Many-LUT bootstrap on the GPU (helm_si_make_many_lut / helm_si_pbs_many_batch / helm_si_apply_many_luts): several
functions of one input from ONE blind rotation, extracted at coefficients 0, N/M, 2N/M, ... of the rotated accumulator.

Per bootstrap kernel build, word for word (tests/many_lut.py is the reference, pinned on the CPU by
tests/test_many_lut_reference.py):
  mask words   every output's, every row's: determined by the oracle's coefficient-0 output of the same bootstrap
               (many_lut.masks_from_output0)
  bodies       B[h] from the exact integer route (many_lut.accumulator_exact) or, for rows with an all-zero mask, from the
               closed form +-tv[(h + b~) mod N] (classical sets; a multi-bit group step runs whatever its exponents, so there
               these rows take the exact route too); output 0's body is the oracle's own
  n_out = 1    equals pbs_batch
  honest rows  decrypt to f_x(v) for every x and every v < t / M
Rows of a launch: the t honest encryptions (the first t / M of them are inside the input bound), two random rows, zero-mask
rows with b~ in {0, 1, N - 1, N, 2N - 1}, one row with a single active step.  The exact route costs up to a second per row,
so at k = 1, N <= 1024 every honest row inside the bound and both random rows go through it, elsewhere the honest rows
v = 0 and v = t / M - 1 and the first random row (the other honest bodies there are held by decryption); the single-step
row always.  Then the wire-table call, its refusals, one full-size case and one launch on the bound-counting build."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helm_amd
import oracle
from helm_amd.shortint import SiWires

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import many_lut as ML  # noqa: E402
import saturation as S  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (id, key: a named set or (k, N, l, logB, g), generic mode, environment at creation, kernel class, field bits or None)
CASES = [
    ("si_toy_2048", "si_toy_2048", None, {}, "tuned", 49),
    ("si_toy_2048_l2", "si_toy_2048_l2", None, {}, "tuned", 49),
    ("si_toy_1024", "si_toy_1024", None, {}, "tuned", 49),
    ("si_toy_512", "si_toy_512", None, {}, "tuned", 49),
    ("si_toy_2048-k_pbs64", "si_toy_2048", None, {"HELM_SI_SPLIT": "0"}, "tuned", 49),
    ("si_toy_2048_l2-k_pbs64", "si_toy_2048_l2", None, {"HELM_SI_SPLIT": "0"}, "tuned", 49),
    ("si_toy_1024-k_pbs64", "si_toy_1024", None, {"HELM_SI_SPLIT": "0"}, "tuned", 49),
    ("si_toy_512_k3", "si_toy_512_k3", None, {}, "tuned", None),
    ("si_toy_512_k3-field49", "si_toy_512_k3", None, {"HELM_SI_FIELD": "49"}, "tuned", 49),
    ("si_toy_512_k2", "si_toy_512_k2", None, {}, "tuned", None),
    ("si_toy_1024_k2", "si_toy_1024_k2", None, {}, "tuned", 49),
    ("si_toy_1024_mb2", "si_toy_1024_mb2", None, {}, "tuned", 49),
    ("si_toy_2048_mb3", "si_toy_2048_mb3", None, {}, "tuned", 49),
    ("generic-forced-si_toy_512", "si_toy_512", "force", {}, "generic", 49),
    ("generic-k2_N512_l2_B12", (2, 512, 2, 12, 0), "allow", {}, "generic", 49),
    ("generic-k3_N512_l1_B18_g2", (3, 512, 1, 18, 2), "allow+multibit", {}, "generic", 49),
]
ROUTE_ALL = {"si_toy_1024", "si_toy_512", "si_toy_1024_mb2"}   # k = 1, N <= 1024: every body inside the bound by the exact route


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        os.environ.update(kv)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def mask_word(a, N):
    """A word that modulus-switches to a (mod 2N)."""
    return np.uint64(a << (64 - N.bit_length()))


def funcs(t, n):
    """n functions over [0, t): distinct, none constant."""
    return [lambda v, x=x: (3 * v + 5 * x + 1) % t for x in range(n)]


_keys, _refs = {}, {}


def _client_key(key):
    if key not in _keys:
        if isinstance(key, str):
            _keys[key] = helm_amd.SiClientKey.generate(key, seed=3)
        else:
            k, N, l, logB, g = key
            p, _, _ = helm_amd.si_named_params("si_toy_512")
            p.n, p.k, p.N, p.pbs_l, p.pbs_logB, p.ks_l, p.ks_logB = 12, k, N, l, logB, 4, 4
            p.message_modulus, p.carry_modulus, p.grouping_factor = 4, 4, g
            _keys[key] = helm_amd.SiClientKey(p, 1e-9, 1e-15, seed=7)
    return _keys[key]


def _reference(key):
    """Computed once per key and shared by every build that runs it; never modified.
    -> dict(ck, small [R, n+1], n_outs, luts {n_out: tv}, want {n_out: [R, n_out, kN+1]}, body_known {n_out: [R, n_out] bool})"""
    if key in _refs:
        return _refs[key]
    ck = _client_key(key)
    p = ck.params
    n, k, N, t = p.n, p.k, p.N, ck.t
    g = max(1, p.grouping_factor)
    shape = S.shape_of(p)
    orc = oracle.Oracle64(p.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
    rng = np.random.default_rng(41)
    honest = np.array([orc.keyswitch(c) for c in ck.encrypt(np.arange(t, dtype=np.uint64))], dtype=np.uint64)
    rand = rng.integers(0, 2**64, size=(2, n + 1), dtype=np.uint64)
    zero = np.zeros((5, n + 1), dtype=np.uint64)
    bts = [0, 1, N - 1, N, 2 * N - 1]
    for q, bt in enumerate(bts):
        zero[q, n] = mask_word(bt, N)
    single = np.zeros((1, n + 1), dtype=np.uint64)
    single[0, n // 2] = mask_word(N + 3, N)
    single[0, n] = rng.integers(0, 2**64, dtype=np.uint64)
    small = np.concatenate([honest, rand, zero, single])
    R = len(small)
    r_rand, r_zero, r_single = t, t + 2, t + 7
    want, known, luts = {}, {}, {}
    for n_out in (1, 2, 3, t):
        M = ML.chunks(n_out)
        per = t // M
        tv = ML.many_lut_poly([[f(v) for v in range(per)] for f in funcs(t, n_out)], t, N)
        luts[n_out] = tv
        w = np.zeros((R, n_out, k * N + 1), dtype=np.uint64)
        kn = np.zeros((R, n_out), dtype=bool)
        if n_out == 1:
            routed = []
        elif key in ROUTE_ALL:
            routed = list(range(per)) + [r_rand, r_rand + 1, r_single]
        else:
            routed = sorted({0, per - 1}) + [r_rand, r_single]
        if g > 1 and n_out > 1:   # multi-bit: a group step runs whatever its exponents, so a zero mask has no closed form
            routed = routed + list(range(r_zero, r_zero + 5))
        for r in range(R):
            out0 = orc.bootstrap(small[r], tv)
            acc = ML.accumulator_exact(small[r], tv, ck.bsk, shape, g) if r in routed else None
            for x in range(n_out):
                h = ML.output_coefficient(x, n_out, N)
                w[r, x, :k * N] = ML.masks_from_output0(out0, k, N, h)
                if r_zero <= r < r_zero + 5 and g == 1:
                    assert not w[r, x, :k * N].any()
                    w[r, x, k * N], kn[r, x] = ML.zero_mask_body(tv, bts[r - r_zero], h), True
                elif acc is not None:
                    assert np.array_equal(ML.extract_at(acc, h)[:-1], w[r, x, :k * N])   # the two references agree
                    w[r, x, k * N], kn[r, x] = acc[k][h], True
                elif x == 0:
                    w[r, x, k * N], kn[r, x] = out0[k * N], True
        want[n_out], known[n_out] = w, kn
    _refs[key] = dict(ck=ck, small=small, luts=luts, want=want, known=known, r_rand=r_rand, r_single=r_single)
    return _refs[key]


def _server_key(case):
    _, key, generic, env, klass, bits = case
    ck = _client_key(key)
    with _env(**env):
        sk = helm_amd.SiServerKey(ck, generic=generic)
    assert sk.kernel_class() == klass
    if bits is not None:
        assert sk.field_bits() == bits
    return sk


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_output_of_every_kernel_build_word_for_word(case):
    ref = _reference(case[1])
    ck, small = ref["ck"], ref["small"]
    k, N, t = ck.params.k, ck.params.N, ck.t
    sk = _server_key(case)
    try:
        routed_random = 0
        for n_out in (1, 2, 3, t):
            tv, want, known = ref["luts"][n_out], ref["want"][n_out], ref["known"][n_out]
            got = sk.pbs_many_batch(small, tv, n_out)
            assert got.shape == want.shape
            assert np.array_equal(got[:, :, :k * N], want[:, :, :k * N]), (n_out, "mask words")
            bad = [(r, x) for r, x in zip(*np.nonzero(known)) if got[r, x, k * N] != want[r, x, k * N]]
            assert not bad, (n_out, "bodies (row, output)", bad[:8])
            routed_random += int(n_out > 1 and known[ref["r_rand"], n_out - 1])
            if n_out == 1:
                assert known.all()
                assert np.array_equal(got[:, 0], sk.pbs_batch(small, tv))
            per = t // ML.chunks(n_out)
            dec = ck.decrypt_message_and_carry(got[:per].reshape(-1, k * N + 1)).reshape(per, n_out)
            assert [[int(v) for v in row] for row in dec] == [[f(v) for f in funcs(t, n_out)] for v in range(per)], n_out
        assert routed_random == 3   # the random-row bodies went through the exact route at every n_out > 1
    finally:
        sk.close()


def _apply_through(ctx, w, *args, **kw):
    """w.apply_many_luts(...) issued through another context (a lane of the table's owner, or a stranger)."""
    v = SiWires.__new__(SiWires)
    v.sk, v.n_rows, v._h = ctx, w.n_rows, w._h
    try:
        v.apply_many_luts(*args, **kw)
    finally:
        v._h = None   # the handle stays the owner's


@pytest.mark.parametrize("name", ["si_toy_2048", "si_toy_512_k3"])
def test_through_the_wire_table(name):
    ck = _client_key(name)
    sk = helm_amd.SiServerKey(ck)
    t, dim = ck.t, ck.dim
    n_out = 2
    cap = sk.round_capacity()
    count = cap + 3
    rng = np.random.default_rng(9)
    luts = np.stack([sk.make_many_lut(funcs(t, 2)), sk.make_many_lut([lambda v: (v * v) % t, lambda v: (t - 1 - v) % t])])
    vals = (np.arange(count) % (t // 2)).astype(np.uint64)
    cts = ck.encrypt(vals)
    rows = count * 3 + 4
    in_idx = np.arange(count, dtype=np.int32)
    out_idx = (count + np.arange(count * 2, dtype=np.int32)).reshape(count, 2)
    out_idx[1, 1] = -1                        # a skipped output
    out_idx[count - 2, 0] = -1
    out_idx[2, 0] = in_idx[2]                 # an output over its own input row
    out_idx[3, 1] = in_idx[5]                 # ... and over another ciphertext's input row
    lut_idx = (np.arange(count) % 2).astype(np.int32)
    sentinel = rng.integers(0, 2**64, size=(rows, dim + 1), dtype=np.uint64)

    def fill(w):
        w.upload(np.arange(rows), sentinel)
        w.upload(in_idx, cts)

    want_rows = sk.pbs_many_batch(sk.keyswitch_batch(cts), luts, n_out, lut_idx)
    seen = []
    sk.set_audit(lambda rec: seen.append(rec))
    sk.timing_enable(True)
    sk.timing(reset=True)
    w = sk.wires(rows)
    fill(w)
    w.apply_many_luts(in_idx, luts, out_idx, lut_idx)
    sk.sync()
    assert sk.timing().pbs_count == count     # blind rotations, not outputs
    sk.set_audit(None)
    expect = sentinel.copy()
    expect[in_idx] = cts
    for g in range(count):
        for x in range(n_out):
            if out_idx[g, x] >= 0:
                expect[out_idx[g, x]] = want_rows[g, x]
    got = w.download()
    assert np.array_equal(got, expect)        # the outputs, and every row no output names untouched
    dec = ck.decrypt_message_and_carry(got[out_idx[10]])
    fs = funcs(t, 2)
    assert [int(v) for v in dec] == [fs[0](int(vals[10])), fs[1](int(vals[10]))]
    # the audit record: kind 2, terms = n_out, the rows written (a skipped output: zeros), the inputs as they were before
    assert len(seen) == 1 and seen[0]["raw_kind"] == 2 and seen[0]["terms"] == n_out and seen[0]["kind"] == "many_luts"
    assert np.array_equal(seen[0]["in_rows"], cts) and np.array_equal(seen[0]["lut_idx"], lut_idx)
    a_out = seen[0]["out_rows"]
    assert a_out.shape == (count, n_out, dim + 1)
    assert not a_out[1, 1].any() and not a_out[count - 2, 0].any()
    keep = out_idx >= 0
    assert np.array_equal(a_out[keep], got[out_idx[keep]])
    # a lane gives the same rows
    lane = sk.fork()
    fill(w)
    sk.sync()
    _apply_through(lane, w, in_idx, luts, out_idx, lut_idx)
    lane.sync()
    assert np.array_equal(w.download(), expect)
    # count 1
    fill(w)
    w.apply_many_luts(in_idx[4:5], luts, out_idx[4:5], lut_idx[4:5])
    one = sentinel.copy()
    one[in_idx] = cts
    one[out_idx[4]] = want_rows[4]
    assert np.array_equal(w.download(), one)
    # n_out = 1 gives the rows of apply_luts
    w.apply_many_luts(in_idx[:7], luts, count + np.arange(7), lut_idx[:7])
    a = w.download(count + np.arange(7))
    w.apply_luts(in_idx[:7], luts, count + np.arange(7), lut_idx[:7])
    assert np.array_equal(a, w.download(count + np.arange(7)))
    sk.close()


def test_refusals_leave_the_context_usable():
    ck = _client_key("si_toy_512")
    sk, other = helm_amd.SiServerKey(ck), helm_amd.SiServerKey(ck)
    t = ck.t
    w, foreign = sk.wires(16), other.wires(16)
    w.upload(np.arange(4), ck.encrypt(np.arange(4, dtype=np.uint64)))
    lut = sk.make_many_lut(funcs(t, 2))
    small = sk.keyswitch_batch(ck.encrypt(np.arange(2, dtype=np.uint64)))
    bad = [lambda: w.apply_many_luts([0, 1], lut, np.zeros((2, 0), dtype=np.int32)),                 # n_out = 0
           lambda: w.apply_many_luts([0], lut, np.arange(4, 4 + t + 1).reshape(1, -1) % 16),       # M > t
           lambda: w.apply_many_luts([0, 1], lut, [[4, 5], [6, 4]]),                                 # one row named twice
           lambda: w.apply_many_luts([0, 1], lut, [[4, 5], [6, 16]]),                                # an output out of range
           lambda: w.apply_many_luts([0, 16], lut, [[4, 5], [6, 7]]),                                # an input out of range
           lambda: w.apply_many_luts([0, 1], lut, [[4, 5], [6, -2]]),
           lambda: w.apply_many_luts([0, 1], lut, [[4, 5], [6, 7]], lut_idx=[0, 1]),                 # a table that is not there
           lambda: _apply_through(sk, foreign, [0, 1], lut, [[4, 5], [6, 7]]),                       # a foreign table
           lambda: sk.pbs_many_batch(small, lut, 0),
           lambda: sk.pbs_many_batch(small, lut, t + 1),
           lambda: sk.make_many_lut([]),
           lambda: sk.make_many_lut(funcs(t, t + 1))]
    before = w.download()
    for q, call in enumerate(bad):
        with pytest.raises(helm_amd.HelmError):
            call()
        assert np.array_equal(w.download(), before), q
    # ... and the context works
    w.apply_many_luts([0, 1, 2, 3], lut, [[4, 5], [6, 7], [8, -1], [-1, 3]])
    dec = ck.decrypt_message_and_carry(w.download([4, 5, 6, 7, 8, 3]))
    fs = funcs(t, 2)
    assert [int(v) for v in dec] == [fs[0](0), fs[1](0), fs[0](1), fs[1](1), fs[0](2), fs[1](3)]
    assert np.array_equal(sk.make_many_lut(funcs(t, 1)), sk.make_lut(funcs(t, 1)[0]))
    sk.close()
    other.close()


def test_message_and_carry_of_a_full_size_block_from_one_rotation():
    """shortint_m2c2: a 2+2-bit block after an addition holds at most 6 < 8 = t / 2 - message v % 4 and carry v // 4 are two
    functions of one blind rotation.  Values 0..6 and 7."""
    ck = helm_amd.SiClientKey.generate("shortint_m2c2", seed=3)
    sk = helm_amd.SiServerKey(ck)
    k, N = ck.params.k, ck.params.N
    vals = np.arange(8, dtype=np.uint64)
    lut = sk.make_many_lut([lambda v: v % 4, lambda v: v // 4])
    w = sk.wires(24)
    w.upload(np.arange(8), ck.encrypt(vals))
    w.apply_many_luts(np.arange(8), lut, 8 + np.arange(16).reshape(8, 2))
    got = w.download(8 + np.arange(16)).reshape(8, 2, -1)
    dec = ck.decrypt_message_and_carry(got.reshape(16, -1)).reshape(8, 2)
    assert [[int(a), int(b)] for a, b in dec] == [[int(v) % 4, int(v) // 4] for v in vals]
    orc = oracle.Oracle64(ck.params.as_tuple(), ck.bsk, ck.ksk, use_ntt=True)
    out0 = orc.apply_luts(w.download(np.arange(8)), lut, np.zeros(8, dtype=np.int32))
    for g in range(8):
        assert np.array_equal(got[g, 0], out0[g]), g
        assert np.array_equal(got[g, 1, :k * N], ML.masks_from_output0(out0[g], k, N, N // 2)), g
    sk.close()


CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [%r, %r]
import helm_amd
import test_gpu_many_lut as T
ck = T._client_key("si_toy_2048")
sk = helm_amd.SiServerKey(ck)
sk.bound_violations(reset=True)
t = ck.t
res = {}
for n_out in (2, 3, t):
    per = t // T.ML.chunks(n_out)
    lut = sk.make_many_lut(T.funcs(t, n_out))
    w = sk.wires(per * (n_out + 1))
    w.upload(np.arange(per), ck.encrypt(np.arange(per, dtype=np.uint64)))
    out_idx = per + np.arange(per * n_out).reshape(per, n_out)
    w.apply_many_luts(np.arange(per), lut, out_idx)
    dec = ck.decrypt_message_and_carry(w.download(out_idx.reshape(-1))).reshape(per, n_out)
    res[str(n_out)] = {"ok": [[int(v) for v in row] for row in dec] == [[f(v) for f in T.funcs(t, n_out)] for v in range(per)]}
res["violations"] = sk.bound_violations()
sk.close()
print("RESULT " + json.dumps(res))
"""


def test_counting_build_counts_nothing_in_a_many_lut_launch():
    """One child process on libhelm_hip_check.so (the same epilogues under -DHELM_CHECK_BOUNDS): values right, every counter
    zero.  It is not retried."""
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    env = dict(os.environ, HELM_HIP_LIB=lib)
    p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["violations"] == [0] * 8, res
    assert all(res[str(n)]["ok"] for n in (2, 3, 16)), res
