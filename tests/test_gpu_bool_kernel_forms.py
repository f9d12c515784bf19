"""Every kernel form of the boolean engine through the same body (helm_amd/csrc/helm_hip.hip: the kernel-form record of a
context - the tuned class in its three fields, the generic and the CRT class, each also forced onto a tuned shape): what the
context reports, nine bootstraps word for word against oracle.Oracle(..., use_ntt=True), another key of the same set loaded
into the same context and the first one loaded back.  Then the remainder builds of the size dispatch: the costs
helm_hip_launch_costs prices them with under every switch, and one launch per remainder bucket against the lockstep build
and the oracle.  Public Python layer only; every set is toy-sized."""
import numpy as np
import pytest

import helm_amd
import oracle
from test_gpu_generic_shapes import toy_params, n_cus

pytestmark = pytest.mark.gpu

SWITCHES = ("HELM_HIP_PBS_VARIANT", "HELM_HIP_FIELD", "HELM_HIP_DUO", "HELM_HIP_DUO1024", "HELM_HIP_TRIO")

#        set                        environment                     crt      kernel class  field  what runs the launches
FORMS = [("toy",                    {},                             None,    "tuned",      51,    "tuned"),    # bound 2^49: above FpG's half
         ((1, 512, 2, 7),           {},                             None,    "tuned",      49,    "tuned"),    # toy's shape at 2^48
         ("toy_k2",                 {},                             None,    "tuned",      49,    "tuned"),
         ((1, 512, 3, 6),           {},                             None,    "tuned",      49,    "tuned"),    # bound 2^47.6 < FpG's half
         ("toy_k2",                 {"HELM_HIP_FIELD": "51"},       None,    "tuned",      51,    "tuned"),
         ("toy_1024",               {},                             None,    "tuned",      50,    "tuned"),
         ("toy_1024_l2",            {},                             None,    "tuned",      50,    "tuned"),
         ("toy_1024",               {"HELM_HIP_FIELD": "51"},       None,    "tuned",      51,    "tuned"),
         ((2, 512, 2, 7),           {},                             None,    "generic",    51,    "generic"),
         ("toy_k2",                 {"HELM_HIP_PBS_VARIANT": "10"}, None,    "tuned",      51,    "generic"),
         ("toy_crt",                {},                             "allow", "crt",        98,    "crt"),
         ("toy",                    {},                             "force", "tuned",      98,    "crt")]


def _id(f):
    name = f[0] if isinstance(f[0], str) else "shape_%d_%d_%d_%d" % f[0]
    return "-".join([name] + [f"{k[9:]}={v}" for k, v in f[1].items()] + ([f"crt={f[2]}"] if f[2] else []))


def client_key(which, seed):
    if isinstance(which, str):
        return helm_amd.ClientKey.generate(which, seed=seed)
    return helm_amd.ClientKey(toy_params(*which), 1e-7, 1e-9, seed=seed)


def set_switches(monkeypatch, env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def tuned_costs(N, k, field, duo=None, duo1024=None, trio=None):
    """The literal table of helm_hip_launch_costs for a tuned launch: duo / duo1024 / trio as HELM_HIP_DUO, HELM_HIP_DUO1024,
    HELM_HIP_TRIO give them (None: unset)."""
    trio = True if trio is None else trio != 0
    if N == 512:
        duo = 2 if duo is None else duo
        return [0.42, 0.66 if duo else 1.0, 0.86 if k == 2 and trio else 0.89, 1.0]
    duo1024 = 3 if duo1024 is None else duo1024
    lazy = field == 50
    two = 0.57 if duo1024 == 3 else (0.66 if lazy else 0.64) if duo1024 else 1.0
    three = (0.80 if lazy else 0.78) if trio else (0.97 if lazy else 0.93)
    return [0.44 if lazy else 0.45, two, three, 1.0]


def occupancy_costs(W):
    """... and its model for the generic / two-prime kernel at W resident workgroups per CU."""
    full = max(1.0, W / 2.0)
    return [max(1.0, ((q * W + 3) // 4) / 2.0) / full for q in (1, 2, 3, 4)]


def nine_rows(ck, seed):
    """The inputs of test_gpu_parity._nine_bootstraps_bit_exact: an encryption of True, a zero mask, random rows."""
    p = ck.params
    rng = np.random.default_rng(seed)
    lwe = rng.integers(0, 2**32, size=(9, p.n + 1), dtype=np.uint32)
    lwe[0] = ck.encrypt(True)
    lwe[3, :] = 0
    tvs = rng.integers(0, 2**32, size=(2, p.N), dtype=np.uint32)
    idx = rng.integers(0, 2, size=9).astype(np.int32)
    return lwe, tvs, idx


def oracle_rows(ck, lwe, tvs, idx, rows=None):
    # (the Goldilocks route is exact while an external product's column sums stay below 2^63, tests/crt_shapes.py: every set
    # here but toy_crt is below that by its capacity bound, 2^64.6 there - reached by crafted keys only; the (k+1) l N = 3072
    # terms of a generated key and these rows have a standard deviation of 2^57.2, so 2^63 is 55 of them away)
    orc = oracle.Oracle(ck.params.as_tuple7(), ck.bsk, ck.ksk, use_ntt=True)
    return {g: orc.bootstrap_noks(lwe[g], tvs[idx[g]]) for g in (range(len(lwe)) if rows is None else rows)}


def load_keys(sk, ck):
    """Both keys of ck into the context sk, as test_n1024_field_follows_the_loaded_key loads them."""
    from helm_amd._native import hip, hip_check, as_u32p
    bsk = np.ascontiguousarray(ck.bsk, dtype=np.uint32).reshape(-1)
    ksk = np.ascontiguousarray(ck.ksk, dtype=np.uint32).reshape(-1)
    hip_check(hip.helm_hip_load_bootstrap_key(sk._h, as_u32p(bsk), bsk.size))
    hip_check(hip.helm_hip_load_keyswitch_key(sk._h, as_u32p(ksk), ksk.size))


@pytest.mark.parametrize("which,env,crt,cls,bits,runs", FORMS, ids=[_id(f) for f in FORMS])
def test_form_reports_bootstraps_and_follows_reloaded_keys(which, env, crt, cls, bits, runs, monkeypatch):
    set_switches(monkeypatch, env)   # (HELM_HIP_FIELD is read again at every key load: the switches stay for the whole test)
    ck_a, ck_b = client_key(which, 3), client_key(which, 4)   # the same set, two keys
    p = ck_a.params
    assert p.n <= 24 and not np.array_equal(np.asarray(ck_a.bsk), np.asarray(ck_b.bsk))
    sk = helm_amd.ServerKey(ck_a, crt=crt)
    # 1. what the context says of itself
    cus = n_cus()
    assert sk.kernel_class() == cls and sk.field_bits() == bits
    quantum, batch = sk.launch_quantum(), sk.digit_batch()
    if runs == "tuned":
        assert quantum == 4 * cus and batch == 0 and sk.short_root_stages() == 2
        assert sk.launch_costs() == tuned_costs(p.N, p.k, bits)
    else:
        assert quantum > 0 and quantum % cus == 0 and batch > 0 and sk.short_root_stages() == 0
        assert sk.launch_costs() == occupancy_costs(quantum // cus)
    # 2. nine bootstraps word for word
    lwe, tvs, idx = nine_rows(ck_a, 2024)
    want_a, want_b = oracle_rows(ck_a, lwe, tvs, idx), oracle_rows(ck_b, lwe, tvs, idx)
    got_a = sk.pbs_batch(lwe, tvs, idx)
    for g in range(9):
        assert np.array_equal(got_a[g], want_a[g]), g
    # 3. key B into the same context
    load_keys(sk, ck_b)
    got_b = sk.pbs_batch(lwe, tvs, idx)
    for g in range(9):
        assert np.array_equal(got_b[g], want_b[g]), g
    assert not np.array_equal(got_a, got_b)
    # 4. key A again: the rows of step 2 come back, and the context says what it said
    load_keys(sk, ck_a)
    assert np.array_equal(sk.pbs_batch(lwe, tvs, idx), got_a)
    assert (sk.field_bits(), sk.launch_quantum(), sk.digit_batch()) == (bits, quantum, batch)
    sk.close()


@pytest.mark.parametrize("name", ["toy_k2", "toy_1024"])
def test_launch_costs_follow_the_remainder_switches(name, monkeypatch):
    """helm_hip_launch_costs prices the builds the size dispatch gives a remainder of <= 1, <= 2, <= 3 bootstraps per CU:
    under every setting of the switches that choose them, the literal of the build chosen."""
    ck = client_key(name, 3)
    p = ck.params
    for duo in (None, 0, 1):
        for trio in (None, 0):
            for duo1024 in ((None, 0, 1, 2) if p.N == 1024 else (None,)):
                env = {"HELM_HIP_DUO": duo, "HELM_HIP_TRIO": trio, "HELM_HIP_DUO1024": duo1024}
                set_switches(monkeypatch, {k: str(v) for k, v in env.items() if v is not None})
                sk = helm_amd.ServerKey(ck)
                bits = sk.field_bits()
                assert bits == (50 if p.N == 1024 else 49)
                assert sk.launch_costs() == tuned_costs(p.N, p.k, bits, duo, duo1024, trio), env
                sk.close()


_LOCKSTEP = {}


def lockstep_rows(name, monkeypatch):
    """6 CUs + 1 rows of the set, their bootstraps by a context created under HELM_HIP_PBS_VARIANT=5 (one launch of the
    lockstep build) and a cache of oracle rows: computed once per set, read by every case."""
    if name not in _LOCKSTEP:
        ck = client_key(name, 12)
        p = ck.params
        rng = np.random.default_rng(5)
        count = 6 * n_cus() + 1
        lwe = rng.integers(0, 2**32, size=(count, p.n + 1), dtype=np.uint32)
        lwe[0] = ck.encrypt(True)
        tvs = rng.integers(0, 2**32, size=(3, p.N), dtype=np.uint32)
        idx = rng.integers(0, 3, size=count).astype(np.int32)
        set_switches(monkeypatch, {"HELM_HIP_PBS_VARIANT": "5"})
        sk5 = helm_amd.ServerKey(ck)
        want = sk5.pbs_batch(lwe, tvs, idx)
        want.setflags(write=False)
        sk5.close()
        _LOCKSTEP[name] = (ck, lwe, tvs, idx, want, {})
    return _LOCKSTEP[name]


@pytest.mark.parametrize("name,env", [("toy_k2", {}), ("toy_k2", {"HELM_HIP_DUO": "0"}), ("toy_k2", {"HELM_HIP_TRIO": "0"}),
                                      ("toy_1024", {}), ("toy_1024", {"HELM_HIP_DUO1024": "1"})],
                         ids=["toy_k2", "toy_k2-DUO=0", "toy_k2-TRIO=0", "toy_1024", "toy_1024-DUO1024=1"])
def test_default_dispatch_at_every_remainder_bucket(name, env, monkeypatch):
    """One launch per remainder bucket of the size dispatch (none, <= 1, <= 2, <= 3 per CU, more; with and without full
    rounds before it): row for row what the lockstep build alone gives, and the oracle's rows at the seams."""
    ck, lwe, tvs, idx, want, exact = lockstep_rows(name, monkeypatch)
    cus = n_cus()
    set_switches(monkeypatch, env)
    sk = helm_amd.ServerKey(ck)
    for count in (cus, cus + 1, 2 * cus + 1, 3 * cus + 1, 4 * cus + 1, 4 * cus + 2 * cus + 1):
        got = sk.pbs_batch(lwe[:count], tvs, idx[:count])
        bad = np.nonzero((got != want[:count]).any(axis=1))[0]
        assert len(bad) == 0, f"{count} bootstraps: {len(bad)} rows differ from the lockstep build, first {bad[:8]}"
        full = count // (4 * cus) * (4 * cus)
        rows = {0, 1, count - 1} | ({full - 1, full} if full else set())
        exact.update(oracle_rows(ck, lwe, tvs, idx, rows - set(exact)))
        for g in sorted(rows):
            assert np.array_equal(got[g], exact[g]), (count, g)
    sk.close()
