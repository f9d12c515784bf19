"""Every blind-rotate kernel of both engines over all rotation amounts and on the rounding tie of the modulus switch.

Each bootstrap kernel has its own front (the modulus switch of the input row into MS[], in the boolean engine the gate's
linear combination before it) and its own rotated read of the accumulator; tests/rotation_edges.py builds the rows that drive
both through every amount 0 .. 2N - 1, in the three flavours "exact multiple", "largest word that rounds down" and "exactly
half way" (tests/test_rotation_edges.py pins the construction, the oracles and exact integers against each other on the CPU).
Every comparison here is word for word, no row is skipped or sampled, and each case first asserts the build that runs
(kernel_class(), field_bits(), the variant switch).

Families, per build:
  mask    one row per amount, ONE non-zero mask word (one active step)        against the oracle
  body    zero mask, the body walks the amounts                               against rotation_edges.zero_mask_reference
  step    the same with one fixed active step a = N + 1                       against the oracle
  const   every mask word alike, one row per edge, and a row walking the edges against the oracle
  wrap    (multi-bit) groups whose subset sums cancel or wrap past 2N         against the oracle
The oracle rows of a set are computed once per module and shared by all builds of the set.

Amount sets: every amount (ALL) for the mask and step sweeps up to N = 2048 and for the body sweep everywhere; R(N) (the edges,
the 63 / 64 / 65 seams and one amount per lane residue) at N >= 4096 and for multi-bit shapes other than k = 1, N <= 1024, whose
oracle rows cost 4 - 35 ms each.  Two departures from a plain "ALL everywhere", both for the oracle's cost:
  - a multi-bit group step runs whatever its exponents, so a zero-mask row has NO closed form there: the multi-bit body sweep
    goes against the oracle over R(N), and the "step" family (which exists so that a classical row reads every coefficient)
    is not run for multi-bit shapes - every group step already reads them all;
  - at N >= 4096 the "step" family runs over R(N).
The boolean builds and their fields come from test_gpu_saturation.CASES32, plus the one build that list lacks - variant 7 at
N = 1024, l = 2, the staggered k_pbs_duo<DuoCfg<F, 10, 1, 2, true>>, in FpI and under HELM_HIP_FIELD=51; the 64-bit ones from the
case lists of test_gpu_many_lut, test_gpu_saturation, test_gpu_multibit_saturation, test_gpu_si_kernel_forms and
test_gpu_large_multibit.  Variant 9 is not run on `toy`: there is no three-per-workgroup build at k = 1, N = 512
(launch_pbs_f falls through to the lockstep kernel, which variant 5 runs), so that context would repeat another.

What "asserts the build" can see: the engine reports kernel_class() and field_bits() (51 under variant 10, 98 on the two-prime
kernel) but has no query for the build HELM_HIP_PBS_VARIANT forced; the test checks that the variable holds the number while
the context is created (creation refuses a number the shape has no build for).  That variants 4 - 9 launch different kernels
rests on the engine's dispatch (launch_pbs_f, helm_hip_tu1_launch_wide), not on anything observed here.

Gate levels (order 0), one per boolean context above (every build, level count and field, not one per kernel kind): operand
rows solved so that the gate's own linear combination is a constant-amount row on an edge, in all flavours, both pre-images
of the XOR / XNOR doubling, with sums that wrap past 2^32, both MUX halves; every output wire against Python-integer
combination -> Oracle.bootstrap_noks -> Oracle.keyswitch and against Oracle.gate."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helm_amd
import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import many_lut as ML  # noqa: E402
import rotation_edges as RE  # noqa: E402
import saturation as S  # noqa: E402
import saturation_mb as M  # noqa: E402
import test_gpu_large_multibit as TLM  # noqa: E402
import test_gpu_many_lut as TML  # noqa: E402
import test_gpu_multibit_saturation as TMB  # noqa: E402
import test_gpu_saturation as TS  # noqa: E402
import test_gpu_si_kernel_forms as TSF  # noqa: E402
from test_gpu_generic_shapes import toy_params, n_cus  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_env = TS._env


def _describe(lwe, q, N, width):
    """The non-zero words of row q: (position, switched amount, word)."""
    row = lwe[q]
    at = np.flatnonzero(row)[:4]
    return "row %d: %s" % (q, [(int(i), S.modswitch(int(row[i]), N, width), hex(int(row[i]))) for i in at])


def _check(got, fam, name, label, N, width):
    if "bodies" in fam:                 # zero_mask_reference: every mask word 0, the body +-tv[bt mod N]
        bad = np.flatnonzero(got[:, :-1].any(axis=1) | (got[:, -1] != fam["bodies"]))
    else:
        bad = np.flatnonzero((got != fam["want"]).any(axis=1))
    assert len(bad) == 0, "%s, family %s: %d of %d rows differ; %s" % (
        label, name, len(bad), len(got), "; ".join(_describe(fam["lwe"], int(q), N, width) for q in bad[:6]))


def _zero_mask_bodies(lwe, tvs, idx, k, N, width):
    rows = RE.zero_mask_rows(lwe, tvs, idx, k, N, width)
    assert not rows[:, :-1].any()
    return rows[:, -1].copy()


# ------------------------------------------------------------------------------------------------------------------
# boolean engine
# ------------------------------------------------------------------------------------------------------------------
GENERIC_256 = next(tuple(s[1:]) for s in S.GENERIC32 if s.N == 256)
GENERIC_2048 = next(tuple(s[1:]) for s in S.GENERIC32 if s.N == 2048)
# (set or (k, N, l, logB), HELM_HIP_PBS_VARIANT, HELM_HIP_FIELD, crt, field_bits, kernel_class)
BOOL_CASES = (
    [(s, build, field, None, bits, cls) for s, build, field, _, bits, cls in TS.CASES32 if isinstance(s, str)] +
    # the staggered duo build at N = 1024, l = 2 (k_pbs_duo<DuoCfg<F, 10, 1, 2, true>>), which that list does not have
    [("toy_1024_l2", 7, None, None, 50, "tuned"), ("toy_1024_l2", 7, "51", None, 51, "tuned")] +
    [(GENERIC_256, None, None, None, 51, "generic"), (GENERIC_2048, None, None, None, 51, "generic"),
     ("toy_crt", None, None, "allow", 98, "crt"), ("toy", None, None, "force", 98, "tuned")])
assert len(set(BOOL_CASES)) == len(BOOL_CASES)
assert {(c[0], c[1], c[2]) for c in BOOL_CASES} >= (
    {(s, v, None) for s in ("toy_k2", "toy") for v in (4, 5, 6, 7)} | {("toy_k2", 9, None), ("toy_k2", 10, None)} |
    {(s, v, f) for s in ("toy_1024", "toy_1024_l2") for v in (4, 5, 6, 7, 8, 9) for f in (None, "51")})
assert ("toy_1024", None, "51", None, 51, "tuned") in BOOL_CASES


def _bool_id(c):
    name = c[0] if isinstance(c[0], str) else "k%d_N%d_l%d_B%d" % c[0]
    return "-".join([name] + ["%s%s" % kv for kv in (("build_", c[1]), ("field_", c[2]), ("crt_", c[3])) if kv[1] is not None])


_bool_keys, _bool_sets, _gate_sets = {}, {}, {}


def _bool_key(which):
    if which not in _bool_keys:
        _bool_keys[which] = (helm_amd.ClientKey.generate(which, seed=21) if isinstance(which, str) else
                             helm_amd.ClientKey(toy_params(*which), 1e-7, 1e-9, seed=7))
    return _bool_keys[which]


def _bool_set(which):
    """The rows of the four families of a set and their references: computed once, read by every build of the set."""
    if which not in _bool_sets:
        ck = _bool_key(which)
        p = ck.params
        shape, N, k = S.shape_of(p), p.N, p.k
        assert p.n <= 24 and p.pbs_order == 0
        rng = np.random.default_rng(N + 7 * k + p.pbs_l)
        tvs = rng.integers(0, 2**32, size=(2, N), dtype=np.uint32)
        orc = oracle.Oracle(p.as_tuple7(), ck.bsk, ck.ksk, use_ntt=True)
        fams = {}
        for name, lwe in (("mask", RE.mask_sweep(shape, RE.ALL(N), 32, rng)[0]),
                          ("body", RE.body_sweep(shape, RE.ALL(N), 32)[0]),
                          ("step", RE.body_sweep(shape, RE.ALL(N), 32, step=(0, N + 1))[0]),
                          ("const", RE.constant_rows(shape, 32, rng)[0])):
            idx = (np.arange(len(lwe)) % 2).astype(np.int32)
            fam = dict(lwe=lwe, idx=idx)
            if name == "body":
                fam["bodies"] = _zero_mask_bodies(lwe, tvs, idx, k, N, 32)
            else:
                fam["want"] = np.stack([orc.bootstrap_noks(lwe[q], tvs[idx[q]]) for q in range(len(lwe))])
            fams[name] = fam
        _bool_sets[which] = dict(ck=ck, tvs=tvs, fams=fams, N=N)
    return _bool_sets[which]


def _bool_context(case):
    which, build, field, crt, bits, cls = case
    with _env(HELM_HIP_PBS_VARIANT=build, HELM_HIP_FIELD=field, HELM_HIP_DUO=None, HELM_HIP_DUO1024=None, HELM_HIP_TRIO=None):
        assert os.environ.get("HELM_HIP_PBS_VARIANT") == (None if build is None else str(build))
        sk = helm_amd.ServerKey(_bool_key(which), crt=crt)     # (a build the shape does not have is refused here)
    assert sk.kernel_class() == cls and sk.field_bits() == bits, (sk.kernel_class(), sk.field_bits())
    return sk


def run_bool(case, families=("mask", "body", "step", "const"), check_build=False):
    st = _bool_set(case[0])
    sk = _bool_context(case)
    try:
        if check_build:
            sk.bound_violations(reset=True)
        for name in families:
            fam = st["fams"][name]
            assert len(fam["lwe"]) <= 2 * st["N"] + 1
            _check(sk.pbs_batch(fam["lwe"], st["tvs"], fam["idx"]), fam, name, _bool_id(case), st["N"], 32)
        assert sk.field_bits() == case[4]
        return sk.bound_violations() if check_build else None
    finally:
        sk.close()


@pytest.mark.parametrize("case", BOOL_CASES, ids=[_bool_id(c) for c in BOOL_CASES])
def test_boolean_builds_over_every_amount(case):
    run_bool(case)


@pytest.mark.parametrize("name", ["toy_k2", "toy_1024"])
def test_default_dispatch_across_the_build_seam(name):
    """2N + 1 rows in ONE launch under the size dispatch: full lockstep rounds and a remainder on another build."""
    st = _bool_set(name)
    N, fams = st["N"], st["fams"]
    lwe = np.concatenate([fams["mask"]["lwe"], fams["const"]["lwe"][1:2]])
    idx = np.concatenate([fams["mask"]["idx"], fams["const"]["idx"][1:2]])
    want = np.concatenate([fams["mask"]["want"], fams["const"]["want"][1:2]])
    assert len(lwe) == 2 * N + 1 and len(lwe) % (4 * n_cus()) != 0
    case = next(c for c in BOOL_CASES if c[0] == name and c[1] is None and c[2] is None)
    sk = _bool_context(case)
    try:
        _check(sk.pbs_batch(lwe, st["tvs"], idx), dict(lwe=lwe, want=want), "mask + 1", name + ", default dispatch", N, 32)
    finally:
        sk.close()


# gate levels: one per context of BOOL_CASES - every build, level count and field the sweeps above run (lockstep, wide, duo in
# step / staggered, trio / tri10 with three and two per workgroup, generic forced and by shape, two-prime by shape and forced)
GATE_CASES = BOOL_CASES


def _gate_set(which):
    if which not in _gate_sets:
        ck = _bool_key(which)
        p = ck.params
        n, N, kN = p.n, p.N, p.k * p.N
        G = RE.gate_rows(n, N, RE.E(N), np.random.default_rng(n + N))
        count = len(G["op"])
        orc = oracle.Oracle(p.as_tuple7(), ck.bsk, ck.ksk, use_ntt=True)
        tv = np.full(N, RE.PT_TRUE, dtype=np.uint32)
        want = np.zeros((count, n + 1), dtype=np.uint32)
        for q in range(count):
            op, l, r, c = int(G["op"][q]), G["l"][q], G["r"][q], G["c"][q]
            lin = np.array(RE.lincomb(op, 0, l, r, c, n), dtype=np.uint32)
            big = orc.bootstrap_noks(lin, tv)
            if op == RE.MUX:            # the two halves plus 1/8 before the keyswitch
                lin1 = np.array(RE.lincomb(op, 1, l, r, c, n), dtype=np.uint32)
                assert np.array_equal(lin if G["which"][q] == 0 else lin1, G["want"][q])
                big = big + orc.bootstrap_noks(lin1, tv)
                big[kN:] += np.uint32(RE.PT_TRUE)
            else:
                assert np.array_equal(lin, G["want"][q])
            want[q] = orc.keyswitch(big)
        # Oracle.gate on the same operands (one parallel level): a disagreement says which side moved
        wires = np.zeros((4 * count, n + 1), dtype=np.uint32)
        wires[:count], wires[count:2 * count], wires[2 * count:3 * count] = G["l"], G["r"], G["c"]
        ar = np.arange(count, dtype=np.int32)
        i2 = np.where(G["op"] == RE.MUX, 2 * count + ar, -1).astype(np.int32)
        ref = wires.copy()
        orc.eval_level(ref, G["op"], ar, count + ar, i2, 3 * count + ar)
        assert np.array_equal(ref[3 * count:], want), "Oracle.gate and the Python-integer combination disagree"
        _gate_sets[which] = dict(G=G, wires=wires, want=want, i2=i2, count=count)
    return _gate_sets[which]


@pytest.mark.parametrize("case", GATE_CASES, ids=[_bool_id(c) for c in GATE_CASES])
def test_gate_levels_on_crafted_operands(case):
    which = case[0]
    st = _gate_set(which)
    G, count = st["G"], st["count"]
    sk = _bool_context(case)
    try:
        assert sk.wire_words() == _bool_key(which).params.n + 1
        w = sk.wires(4 * count)
        w.upload(np.arange(3 * count), st["wires"][:3 * count])
        ar = np.arange(count, dtype=np.int32)
        w.eval_gate_level(G["op"], ar, count + ar, st["i2"], 3 * count + ar)
        got = w.download(3 * count + ar)
        bad = np.flatnonzero((got != st["want"]).any(axis=1))
        assert len(bad) == 0, "%d of %d gates differ; first (op, half, target, flavour, pre-image): %s" % (
            len(bad), count, [(int(G["op"][q]), int(G["which"][q]), G["target"][q], G["flavour"][q], G["preimage"][q])
                              for q in bad[:8]])
        assert np.array_equal(w.download(np.arange(3 * count)), st["wires"][:3 * count])     # the operands are untouched
    finally:
        sk.close()


# ------------------------------------------------------------------------------------------------------------------
# 64-bit engine
# ------------------------------------------------------------------------------------------------------------------
def _si_cases():
    """(id, key, generic mode, environment at creation, kernel class, field bits).  key: a named set, a saturation.Shape
    (a generated key of that shape), ("mb", MbShape) (n = 3 g, uniform key words below 2^61) or ("large", N, g)."""
    out = []
    # the tuned classical builds: k_pbs64 (si_toy_512, and the split sets under HELM_SI_SPLIT=0), k_pbs64s, k_pbs64k in both
    # pairs, the k = 2 sets - test_gpu_many_lut's list
    follows_key = {"si_toy_512_k3": 46, "si_toy_512_k2": 49}
    for cid, key, mode, env, cls, bits in TML.CASES:
        if isinstance(key, str) and "_mb" not in key and mode is None:
            out.append((cid, key, None, dict(env), cls, bits if bits is not None else follows_key[key]))
    # the generic kernel, one case per LOGN 8 .. 11: forced onto the named sets, and the smallest untuned N = 256 shape
    generic = [c for c in TS.CASES64 if c[5] == "generic"]
    for N in (256, 512, 1024, 2048):
        at = [c for c in generic if (S.NAMED64[c[0]] if isinstance(c[0], str) else c[0]).N == N]
        s, mode = min(at, key=lambda c: (S.NAMED64[c[0]] if isinstance(c[0], str) else c[0]).k)[:2]
        out.append(("generic-%s-%s" % (mode, s if isinstance(s, str) else "k%d_N%d_l%d_B%d" % s[1:]), s, mode, {}, "generic", 49))
    # the multi-bit forms: four tuned instantiations of k_pbs64s<., true>, eight of k_pbs64_generic<LOGN, g>
    for s, mode, cls, _ in TMB.TUNED_CASES + TMB.GENERIC_CASES:
        out.append(("%s-%s" % (M.shape_id(s), cls), ("mb", s), mode, {}, cls, 49))
    # k_pbs64_large<12, 1 | 2 | 3>, k_pbs64_n8192<1 | 2 | 3>
    for name, mode, cls, bits in TSF.FORMS:
        if cls in ("large", "n8192") and "_mb" not in name:
            out.append((name, name, mode, {}, cls, bits))
    for N in sorted(TLM.MODE):
        for g in (2, 3):
            out.append(("si_toy_%d_mb%d" % (N, g), ("large", N, g), TLM.MODE[N], {}, TLM.CLASS[N], 50))
    return out


SI_CASES = _si_cases()
assert len([c for c in SI_CASES if c[1][0] == "mb"]) == 12 and len([c for c in SI_CASES if c[4] in ("large", "n8192")]) == 6
assert [c[0] for c in SI_CASES if c[4] == "generic" and c[1][0] != "mb"] == [
    "generic-allow-k1_N256_l6_B5", "generic-force-si_toy_512", "generic-force-si_toy_1024", "generic-force-si_toy_2048"]

_si_sets = {}


def _si_material(key):
    """-> (params, bsk, ksk, client key or None)"""
    if isinstance(key, tuple) and key[0] == "mb":
        s = key[1]
        p = TMB._params(s)
        words = (p.n // s.g << s.g) * s.l * (s.k + 1) ** 2 * s.N
        bsk = np.random.default_rng(s.N + s.k + s.g).integers(-(1 << 61), 1 << 61, size=words, dtype=np.int64).view(np.uint64)
        assert not M.over_threshold(M.loader_bound(bsk, s))
        return p, bsk, TMB._ksk(s), None
    ck = TLM.toy_key(key[1], key[2]) if isinstance(key, tuple) and key[0] == "large" else TS._client_key(key, 64)
    return ck.params, ck.bsk, ck.ksk, ck


def _si_set(key):
    if key in _si_sets:
        return _si_sets[key]
    p, bsk, ksk, ck = _si_material(key)
    shape, N, k, g = S.shape_of(p), p.N, p.k, max(1, p.grouping_factor)
    assert p.n <= 12 and p.n % g == 0
    rng = np.random.default_rng(N + 7 * k + g)
    tvs = rng.integers(0, 2**64, size=(2, N), dtype=np.uint64)
    orc = oracle.Oracle64(p.as_tuple(), bsk, ksk, use_ntt=True)
    small = RE.ALL(N) if (N <= 2048 if g == 1 else (k == 1 and N <= 1024)) else RE.R(N)
    lists = [("mask", RE.mask_sweep(shape, small, 64, rng, g=g)[0])]
    if g == 1:
        lists += [("body", RE.body_sweep(shape, RE.ALL(N), 64)[0]),
                  ("step", RE.body_sweep(shape, RE.ALL(N) if N <= 2048 else RE.R(N), 64, step=(0, N + 1))[0])]
    else:
        lists += [("body", RE.body_sweep(shape, RE.R(N), 64)[0]), ("wrap", RE.wrap_groups(shape, g, 64, rng)[0])]
    lists.append(("const", RE.constant_rows(shape, 64, rng)[0]))
    fams = {}
    for name, lwe in lists:
        idx = (np.arange(len(lwe)) % 2).astype(np.int32)
        fam = dict(lwe=lwe, idx=idx)
        if name == "body" and g == 1:
            fam["bodies"] = _zero_mask_bodies(lwe, tvs, idx, k, N, 64)
        else:
            fam["want"] = np.stack([orc.bootstrap(lwe[q], tvs[idx[q]]) for q in range(len(lwe))])
        fams[name] = fam
    _si_sets[key] = dict(params=p, bsk=bsk, ksk=ksk, ck=ck, tvs=tvs, fams=fams, N=N, k=k, g=g)
    return _si_sets[key]


def _si_context(case):
    cid, key, mode, env, cls, bits = case
    st = _si_set(key)
    with _env(**dict({"HELM_SI_FIELD": None, "HELM_SI_SPLIT": None}, **env)):
        sk = helm_amd.SiServerKey(params=st["params"], bsk=st["bsk"], ksk=st["ksk"], generic=mode)
    assert sk.kernel_class() == cls and sk.field_bits() == bits, (sk.kernel_class(), sk.field_bits())
    return sk


def _si_launches(ctx, st, name):
    """One family through ctx.pbs_batch, at most 2N + 1 rows per launch (at N >= 4096: 2,048, so that the rows of a launch
    stay below 150 MB; such a launch goes out in rounds of round_capacity())."""
    fam = st["fams"][name]
    step = min(2 * st["N"] + 1, 2048 if st["N"] >= 4096 else 1 << 30)
    for lo in range(0, len(fam["lwe"]), step):
        part = {key: v[lo:lo + step] for key, v in fam.items()}
        yield part, ctx.pbs_batch(part["lwe"], st["tvs"], part["idx"])


def run_si(case, families=None, check_build=False, lane=False):
    st = _si_set(case[1])
    sk = _si_context(case)
    try:
        ctx = sk
        if lane:
            ctx = sk.fork()
            assert ctx.kernel_class() == case[4] and ctx.field_bits() == case[5]
        if check_build:
            sk.bound_violations(reset=True)
        for name in (families or list(st["fams"])):
            for part, got in _si_launches(ctx, st, name):
                _check(got, part, name, case[0], st["N"], 64)
        return sk.bound_violations() if check_build else None
    finally:
        sk.close()


@pytest.mark.parametrize("case", SI_CASES, ids=[c[0] for c in SI_CASES])
def test_shortint_builds_over_every_amount(case):
    run_si(case)


def test_a_lane_over_every_amount():
    run_si(next(c for c in SI_CASES if c[0] == "si_toy_1024"), families=("mask", "body"), lane=True)


MANY_LUT_CASES = ["si_toy_512", "si_toy_1024", "si_toy_512_k3", "generic-force-si_toy_512", "si_toy_4096", "si_toy_8192"]


@pytest.mark.parametrize("cid", MANY_LUT_CASES)
def test_many_lut_bodies_at_the_seams(cid):
    """pbs_many_batch with n_out = 2 on the body sweep over E(N), one build per kernel class: both extracts of every row
    against the accumulator X^(-bt) tv (many_lut.zero_mask_acc) - test_gpu_many_lut.py's five body values, at the seams."""
    case = next(c for c in SI_CASES if c[0] == cid)
    st = _si_set(case[1])
    N, k, n_out = st["N"], st["k"], 2
    shape = S.shape_of(st["params"])
    lwe, _ = RE.body_sweep(shape, RE.E(N), 64)
    tv = st["tvs"][1]
    sk = _si_context(case)
    try:
        got = sk.pbs_many_batch(lwe, tv, n_out)
        assert got.shape == (len(lwe), n_out, k * N + 1)
        for q, bt in enumerate(RE.E(N)):
            acc = ML.zero_mask_acc(tv, bt, k)
            for x in range(n_out):
                assert np.array_equal(got[q, x], ML.extract_at(acc, ML.output_coefficient(x, n_out, N))), (bt, x)
    finally:
        sk.close()


# ------------------------------------------------------------------------------------------------------------------
# the bound-counting build
# ------------------------------------------------------------------------------------------------------------------
CHECK_BOOL = ("toy_k2", None, None, None, 49, "tuned")
CHECK_SI = "si_toy_1024"


def child_main():
    """Runs in the child process of test_counting_build_counts_nothing_over_the_sweeps."""
    res = {"bool": run_bool(CHECK_BOOL, families=("mask", "body", "const"), check_build=True),
           "si": run_si(next(c for c in SI_CASES if c[0] == CHECK_SI), families=("mask", "body", "const"), check_build=True)}
    print("RESULT " + json.dumps(res))


def test_counting_build_counts_nothing_over_the_sweeps():
    """The check build (libhelm_hip_check.so) on one tuned set of each engine: word for word, every counter zero.  (The
    generic 64-bit contexts it refuses stay refused: tests/test_gpu_si_generic_shapes.py keeps that test.)  One child process."""
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    assert CHECK_BOOL in BOOL_CASES
    env = dict(os.environ, HELM_HIP_LIB=lib)
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_rotation_edges as T; T.child_main()" % (
        ROOT, os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res == {"bool": [0] * 8, "si": [0] * 8}, res
