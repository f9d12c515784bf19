"""Every kernel form of the 64-bit engine through the same body (helm_amd/csrc/helm_shortint.hip: the kernel-form record of a
context - class 0 in its four tuned forms, classes 1 to 3): what the context reports, bootstraps word for word against
oracle.Oracle64(..., use_ntt=True), and - the part only the k form met so far - another key of the same set loaded into the
same primary and the first one loaded back.  A reload runs the allocate-once, probe-once and pair-follows-key logic of the key
loader for the form at hand, on the primary and, through the shared key state, on a lane forked before it."""
import numpy as np
import pytest

import helm_amd
import oracle

pytestmark = pytest.mark.gpu

#        set                mode               kernel class  field bits   form
FORMS = [("si_toy_512",      None,              "tuned",      49),       # wide            k_pbs64
         ("si_toy_1024",     None,              "tuned",      49),       # split           k_pbs64s<., false>
         ("si_toy_1024_mb2", None,              "tuned",      49),       # split multi-bit k_pbs64s<., true>
         ("si_toy_512_k3",   None,              "tuned",      46),       # k               k_pbs64k (a generated key: 46 bits)
         ("si_toy_512",      "force",           "generic",    49),       #                 k_pbs64_generic
         ("si_toy_4096",     "large",           "large",      50),       #                 k_pbs64_large
         ("si_toy_8192",     "n8192",           "n8192",      50),       #                 k_pbs64_n8192
         ("si_toy_1024_mb2", "force+multibit",  "generic",    49),       # the multi-bit forms of the generic ...
         ("si_toy_4096_mb2", "large+multibit",  "large",      50)]       # ... and the large-N kernel


def load_keys(sk, ck):
    """Both keys of ck into the primary sk, as test_lane_follows_keys_reloaded_into_its_primary loads them."""
    from helm_amd._native import hip, hip_check, as_u64p
    bsk = np.ascontiguousarray(ck.bsk, dtype=np.uint64).reshape(-1)
    ksk = np.ascontiguousarray(ck.ksk, dtype=np.uint64).reshape(-1)
    hip_check(hip.helm_si_load_bootstrap_key(sk._h, as_u64p(bsk), bsk.size))
    hip_check(hip.helm_si_load_keyswitch_key(sk._h, as_u64p(ksk), ksk.size))


@pytest.mark.parametrize("name,mode,cls,bits", FORMS, ids=[f"{f[0]}-{f[1] or 'default'}" for f in FORMS])
def test_form_bootstraps_and_follows_reloaded_keys(name, mode, cls, bits):
    ck_a = helm_amd.SiClientKey.generate(name, seed=3)
    ck_b = helm_amd.SiClientKey.generate(name, seed=4)   # the same set, another key
    p, t = ck_a.params, ck_a.t
    assert not np.array_equal(np.asarray(ck_a.bsk), np.asarray(ck_b.bsk))
    # 1. what the context says of itself, and of a lane forked now
    sk = helm_amd.SiServerKey(ck_a, generic=mode)
    assert sk.kernel_class() == cls and sk.field_bits() == bits
    lane = sk.fork()
    assert lane.kernel_class() == cls and lane.field_bits() == bits
    cap = sk.round_capacity()
    assert cap > 0 and lane.round_capacity() == cap
    # 2. four rows word for word: an honest keyswitched ciphertext, a zero mask (no step is active), two random rows
    orc_a = oracle.Oracle64(p.as_tuple(), ck_a.bsk, ck_a.ksk, use_ntt=True)
    orc_b = oracle.Oracle64(p.as_tuple(), ck_b.bsk, ck_b.ksk, use_ntt=True)
    rng = np.random.default_rng(2024)
    small = rng.integers(0, 2**64, size=(4, p.n + 1), dtype=np.uint64)
    ct_a = ck_a.encrypt([3 % t])
    small[0] = sk.keyswitch_batch(ct_a)[0]
    assert np.array_equal(small[0], orc_a.keyswitch(ct_a[0]))
    small[1, :p.n] = 0
    luts = np.stack([orc_a.make_lut(lambda x: (3 * x + 1) % t), orc_a.make_lut(lambda x: x * x % t)])
    idx = np.array([0, 1, 0, 1], dtype=np.int32)
    want_a = np.stack([orc_a.bootstrap(small[g], luts[idx[g]]) for g in range(4)])
    want_b = np.stack([orc_b.bootstrap(small[g], luts[idx[g]]) for g in range(4)])
    assert not np.array_equal(want_a, want_b)
    got_a = sk.pbs_batch(small, luts, idx)
    assert np.array_equal(got_a, want_a)
    assert int(ck_a.decrypt_message_and_carry(got_a[:1])[0]) == (3 * 3 + 1) % t
    # 3. key B into the same primary: primary and lane bootstrap and keyswitch under B
    load_keys(sk, ck_b)
    assert sk.field_bits() == bits and lane.field_bits() == bits
    for ctx in (sk, lane):
        assert np.array_equal(ctx.pbs_batch(small, luts, idx), want_b)
    ct_b = ck_b.encrypt([5 % t])
    assert np.array_equal(lane.keyswitch_batch(ct_b)[0], orc_b.keyswitch(ct_b[0]))
    assert sk.round_capacity() == cap and lane.round_capacity() == cap
    # 4. key A again: the rows of step 2 come back
    load_keys(sk, ck_a)
    assert sk.field_bits() == bits and lane.field_bits() == bits
    for ctx in (sk, lane):
        assert np.array_equal(ctx.pbs_batch(small, luts, idx), got_a)
    sk.close()
