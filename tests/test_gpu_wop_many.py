"""helm_wop_eval_many_luts on the GPU: several wide-LUT tables on one input tuple share cleaning, bit extraction and circuit
bootstrap.  Every stage is deterministic, so the call must leave the wire table word for word as n_out separate
helm_wop_eval_luts calls on the same inputs, and its stage primitive the rows of single-table vertical packings on the same
GGSWs; end to end every output decrypts to its table's entry.  Every output of a group has its own table, so a swapped output
or key index shows."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import helm_amd
from helm_amd import _native as nv
from helm_amd import wopbs
from helm_amd.shortint import si_named_params

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:overflow encountered")]
U64 = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_keys(pbs_name, wop_name, seed, moduli=None, cbs=None):
    sp, a, b = si_named_params(pbs_name)
    wp, c, d = wopbs.wop_named_params(wop_name)
    if moduli is not None:
        sp.message_modulus, sp.carry_modulus = moduli
        wp.message_modulus, wp.carry_modulus = moduli
    if cbs is not None:
        wp.cbs_l, wp.cbs_logB = cbs
    ck = helm_amd.SiClientKey(sp, a, b, seed=seed)
    wk = wopbs.WopClientKey(ck, wp, c, d, seed=seed + 1)
    sk = helm_amd.SiServerKey(ck)
    wsk = wopbs.WopServerKey(sk, wk)
    return ck, wk, sk, wsk


def close(keys):
    keys[3].close()
    keys[2].close()


@pytest.fixture(scope="module")
def toy512():
    keys = make_keys("si_toy_512", "wop_toy_512", seed=11)
    yield keys
    close(keys)


@pytest.fixture(scope="module")
def toy1024():
    keys = make_keys("si_toy_1024", "wop_toy_1024", seed=12)
    yield keys
    close(keys)


@pytest.fixture(scope="module")
def toy2048():
    """wop_toy_2048 (message = carry = 2) beside a small PBS side of the same moduli"""
    keys = make_keys("si_toy_512", "wop_toy_2048", seed=13, moduli=(2, 2))
    yield keys
    close(keys)


def groups_case(ck, n_inputs, bpb, n_out, count, seed, truth_len=4096):
    """count groups on distinct input tuples, a distinct random truth table per output"""
    rng = np.random.default_rng(seed)
    vals = rng.integers(0, 1 << bpb, size=(count, n_inputs)).astype(U64)
    truth = rng.integers(0, 2, size=(count, n_out, truth_len), dtype=U64)
    assert len({t.tobytes() for t in truth.reshape(count * n_out, -1)}) == count * n_out
    cts = ck.encrypt(vals.reshape(-1))
    in_idx = np.arange(count * n_inputs, dtype=np.int32).reshape(count, n_inputs)
    out_idx = np.arange(count * n_inputs, count * (n_inputs + n_out), dtype=np.int32).reshape(count, n_out)
    return vals, truth, cts, in_idx, out_idx


def fresh(sk, cts, rows):
    w = sk.wires(rows)
    w.upload(np.arange(len(cts)), cts)
    return w


def expected(ck, vals, truth, bpb):
    """the table rule of helm_wop_make_table: x = sum block_j basis^j, block j = input n - 1 - j"""
    basis = int(ck.params.message_modulus)
    n = vals.shape[1]
    out = []
    for g in range(vals.shape[0]):
        x = sum(int(v) * basis ** j for j, v in enumerate(vals[g][::-1])) % basis ** n
        out.append([int(t[x]) & 1 if x < len(t) else 0 for t in truth[g]])
    return out


# ---- 1: shared form == separate calls ---------------------------------------------------------------------------
@pytest.mark.parametrize("which,n_inputs,bpb,n_out,count", [("toy512", 3, 4, 3, 5), ("toy512", 2, 4, 3, 2), ("toy1024", 11, 1, 2, 2)])
def test_shared_form_equals_separate_calls(request, which, n_inputs, bpb, n_out, count):
    ck, wk, sk, wsk = request.getfixturevalue(which)
    bits = n_inputs * bpb
    assert wsk.many_form(bits, n_out) == 1
    vals, truth, cts, in_idx, out_idx = groups_case(ck, n_inputs, bpb, n_out, count, seed=bits)
    rows = count * (n_inputs + n_out)
    w = fresh(sk, cts, rows)
    wsk.timing(reset=True)
    wsk.eval_many_luts(w, in_idx, truth, out_idx, bits_per_block=bpb)
    t_many = wsk.timing(reset=True)
    got = w.download()
    w.free()
    w = fresh(sk, cts, rows)
    for o in range(n_out):
        wsk.eval_luts(w, in_idx, truth[:, o], out_idx[:, o], bits_per_block=bpb)
        if o == 0:
            t_one = wsk.timing(reset=True)
    want = w.download()
    w.free()
    assert np.array_equal(got, want), "rows %s differ" % sorted({int(r) for r in np.argwhere(got != want)[:, 0]})[:8]
    dec = ck.decrypt_message_and_carry(got[out_idx.reshape(-1)]).reshape(count, n_out)
    assert [[int(v) for v in r] for r in dec] == expected(ck, vals, truth, bpb)
    assert t_many["gates"] == count * n_out and t_one["gates"] == count
    assert t_many["bootstraps"] == t_one["bootstraps"] + (n_out - 1) * count


# ---- 2: n_out = 1 -------------------------------------------------------------------------------------------------
def test_one_output_is_eval_luts(toy512):
    ck, wk, sk, wsk = toy512
    assert wsk.many_form(6, 1) == 0 and wsk.many_form(15, 1) == 0
    vals, truth, cts, in_idx, out_idx = groups_case(ck, 3, 2, 1, 4, seed=2)
    w = fresh(sk, cts, 16)
    wsk.eval_many_luts(w, in_idx, truth, out_idx, bits_per_block=2)
    got = w.download()
    w.free()
    w = fresh(sk, cts, 16)
    wsk.eval_luts(w, in_idx, truth[:, 0], out_idx[:, 0], bits_per_block=2)
    assert np.array_equal(got, w.download())
    w.free()


# ---- 3: stage level ------------------------------------------------------------------------------------------------
def encrypt_bits_small(wk, bits, rng):
    s = wk.lwe_secret.astype(bool)
    cts = rng.integers(0, 1 << 64, size=(len(bits), wk.params.n + 1), dtype=U64)
    cts[:, -1] = (cts[:, :-1] * s).sum(axis=1, dtype=U64) + (np.array(bits, dtype=U64) << U64(63)) + U64(999)
    return cts


def shared_stage(keys, cases, seed):
    """each (bits, n_out, value): one group whose GGSWs are circuit-bootstrap outputs of the value's bits and one control group
    of uniform words; every output equals the single-table vertical packing of its table on the same GGSWs word for word, and
    the bootstrapped group decrypts to the tables' entries"""
    ck, wk, sk, wsk = keys
    P = wk.params
    rng = np.random.default_rng(seed)
    for bits, n_out, value in cases:
        assert wsk.many_form(bits, n_out) == 1
        flat = [(value >> i) & 1 for i in range(bits)]
        boot = wsk.circuit_bootstrap(encrypt_bits_small(wk, flat, rng))
        ggsw = np.stack([boot, rng.integers(0, 1 << 64, size=boot.shape, dtype=U64)])
        words = max(1 << bits, P.N)
        tables = rng.integers(0, wk.t, size=(2, n_out, words), dtype=U64) * U64(wk.delta)
        tables[1] = rng.integers(0, 1 << 64, size=(n_out, words), dtype=U64)
        got = wsk.vertical_packing_many(ggsw, tables, n_out)
        assert got.shape == (2, n_out, P.N + 1)
        for o in range(n_out):
            assert np.array_equal(got[:, o], wsk.vertical_packing(ggsw, tables[:, o])), (P.N, bits, n_out, o)
        assert len({r.tobytes() for r in got[0]}) == n_out
        err = (wk.phase(got[0]) - tables[0, :, value]).astype(np.int64)
        assert int(np.abs(err).max()) < 1 << 56, (bits, n_out)


def test_stage_level_n512(toy512):
    """without a tree (6, 8 and 1 bits) and with one (11 bits: two levels), two to eight tables"""
    shared_stage(toy512, [(6, 2, 37), (6, 8, 63), (8, 2, 255), (1, 2, 1), (11, 3, 1500)], seed=30)


def test_stage_level_n1024_and_n2048(toy1024, toy2048):
    shared_stage(toy1024, [(5, 32, 31), (11, 2, 2047)], seed=31)
    shared_stage(toy2048, [(8, 8, 201)], seed=32)      # the S-box shape


def test_three_tables_of_eight_bits_take_the_shared_route_at_stage_level(toy512):
    """(8, 3) at N = 512: 3 x 256 > N - the shared form, which equals three single vertical packings on the same GGSWs"""
    ck, wk, sk, wsk = toy512
    P = wk.params
    assert wsk.many_form(8, 3) == 1
    rng = np.random.default_rng(33)
    ggsw = wsk.circuit_bootstrap(encrypt_bits_small(wk, [1, 0, 1, 1, 0, 0, 1, 0] * 2, rng)).reshape(2, 8, P.cbs_l, 2, 2 * P.N)
    tables = rng.integers(0, wk.t, size=(2, 3, P.N), dtype=U64) * U64(wk.delta)
    tables[:, :, 256:] = 0
    got = wsk.vertical_packing_many(ggsw, tables, 3)
    for o in range(3):
        assert np.array_equal(got[:, o], wsk.vertical_packing(ggsw, tables[:, o])), o


# ---- 4: end to end --------------------------------------------------------------------------------------------------
def test_end_to_end_every_input_n512(toy512):
    ck, wk, sk, wsk = toy512
    n_inputs, bpb, n_out, count = 3, 2, 8, 64
    assert wsk.many_form(6, 8) == 1
    rng = np.random.default_rng(50)
    truth = rng.integers(0, 2, size=(n_out, 4 ** n_inputs), dtype=U64)
    vals = np.array([[(x >> (2 * (n_inputs - 1 - q))) & 3 for q in range(n_inputs)] for x in range(count)], dtype=U64)
    cts = ck.encrypt(vals.reshape(-1))
    in_idx = np.arange(count * n_inputs, dtype=np.int32).reshape(count, n_inputs)
    out_idx = np.arange(count * n_inputs, count * (n_inputs + n_out), dtype=np.int32).reshape(count, n_out)
    w = fresh(sk, cts, count * (n_inputs + n_out))
    wsk.eval_many_luts(w, in_idx, truth, out_idx, bits_per_block=bpb)
    dec = ck.decrypt_message_and_carry(w.download(out_idx.reshape(-1))).reshape(count, n_out)
    w.free()
    assert [[int(v) for v in r] for r in dec] == expected(ck, vals, np.broadcast_to(truth, (count, n_out, truth.shape[1])), bpb)


def sbox_truth(seed):
    """the eight output bits of an 8-bit permutation: truth[o][x] under basis 2 (x = the input byte)"""
    perm = np.random.default_rng(seed).permutation(256)
    return perm, np.array([[(int(perm[x]) >> o) & 1 for x in range(256)] for o in range(8)], dtype=U64)


def test_end_to_end_sbox_n2048(toy2048):
    ck, wk, sk, wsk = toy2048
    assert wk.params.N == 2048 and wsk.many_form(8, 8) == 1
    perm, truth = sbox_truth(51)
    xs = [0, 255, 0x53, 0xA7, 1, 128]
    vals = np.array([[(x >> (7 - q)) & 1 for q in range(8)] for x in xs], dtype=U64)
    cts = ck.encrypt(vals.reshape(-1))
    count = len(xs)
    in_idx = np.arange(count * 8, dtype=np.int32).reshape(count, 8)
    out_idx = np.arange(count * 8, count * 16, dtype=np.int32).reshape(count, 8)
    w = fresh(sk, cts, count * 16)
    wsk.eval_many_luts(w, in_idx, truth, out_idx, bits_per_block=1)
    dec = ck.decrypt_message_and_carry(w.download(out_idx.reshape(-1))).reshape(count, 8)
    w.free()
    assert [sum(int(b) << o for o, b in enumerate(r)) for r in dec] == [int(perm[x]) for x in xs]


# ---- 5: edges of a call ---------------------------------------------------------------------------------------------
def test_overwriting_own_inputs_and_both_ends_of_a_batch(toy512):
    ck, wk, sk, wsk = toy512
    for n_out, bpb in ((2, 2), (3, 4)):            # 6 bits x 2 tables (no tree), 12 bits x 3 (three tree levels)
        vals, truth, cts, in_idx, out_idx = groups_case(ck, 3, bpb, n_out, 4, seed=60 + n_out)
        rows = 4 * (3 + n_out)
        w = fresh(sk, cts, rows)
        wsk.eval_many_luts(w, in_idx, truth, out_idx, bits_per_block=bpb)
        want = w.download(out_idx.reshape(-1))
        w.free()
        own = out_idx.copy()
        own[0, :n_out] = in_idx[0, :n_out]          # the first and the last group write over their own inputs
        own[3, :n_out] = in_idx[3, :n_out][::-1]
        w = fresh(sk, cts, rows)
        wsk.eval_many_luts(w, in_idx, truth, own, bits_per_block=bpb)
        assert np.array_equal(w.download(own.reshape(-1)), want), n_out
        w.free()
        dec = ck.decrypt_message_and_carry(want).reshape(4, n_out)
        assert [[int(v) for v in r] for r in dec] == expected(ck, vals, truth, bpb)


def test_refusals(toy512):
    ck, wk, sk, wsk = toy512
    w = sk.wires(12)
    w.upload(np.arange(4), ck.encrypt(np.array([1, 0, 1, 1], dtype=U64)))
    t2 = np.zeros((2, 2, 16), U64)
    with pytest.raises(nv.HelmError, match="input row of another"):
        wsk.eval_many_luts(w, [[0, 1], [2, 6]], t2, [[6, 7], [8, 9]], bits_per_block=1)
    with pytest.raises(nv.HelmError, match="two outputs of the call name row 7"):
        wsk.eval_many_luts(w, [[0, 1], [2, 3]], t2, [[6, 7], [7, 9]], bits_per_block=1)
    with pytest.raises(nv.HelmError, match="out of range"):
        wsk.eval_many_luts(w, [[0, 1]], t2[:1], [[6, 12]], bits_per_block=1)
    too_many = wsk.logN + 7
    tab = np.zeros(2 << too_many, U64)
    with pytest.raises(nv.HelmError, match="index bits"):
        nv.hip_check(nv.hip.helm_wop_eval_many_luts(wsk._h, w._h, nv.as_i32p(np.zeros(too_many, np.int32)), too_many, 1,
                                                    nv.as_u64p(tab), nv.as_i32p(np.array([6, 7], np.int32)), 2, 1))
    with pytest.raises(nv.HelmError, match="n_out must be at least 1"):
        nv.hip_check(nv.hip.helm_wop_eval_many_luts(wsk._h, w._h, nv.as_i32p(np.zeros(2, np.int32)), 2, 1, nv.as_u64p(tab),
                                                    nv.as_i32p(np.array([6], np.int32)), 0, 1))
    with pytest.raises(nv.HelmError, match="many_form"):
        wsk.many_form(wsk.logN + 7, 2)
    wsk.eval_many_luts(w, np.zeros((0, 2), np.int32), np.zeros((0, 2, 16), U64), np.zeros((0, 2), np.int32), bits_per_block=1)
    w.free()


def test_groups_across_the_chunk_edge():
    """12 index bits: a chunk is 1365 groups, and with n_out = 2 its 2730 tables leave in passes of 1365.  1367 groups in one
    call against the same groups in two calls that stay inside a chunk, word for word (the single-output model:
    tests/test_gpu_wopbs.py::test_a_batch_across_the_gate_chunk_edge)."""
    keys = make_keys("si_toy_512", "wop_toy_512", seed=61)
    ck, wk, sk, wsk = keys
    try:
        n_inputs, bpb, n_out, count = 3, 4, 2, 1367
        assert max(1, 16384 // 12) == 1365 and wsk.many_form(12, 2) == 1
        rng = np.random.default_rng(61)
        truth = rng.integers(0, 2, size=(count, n_out, 64), dtype=U64)
        tuples = rng.permutation(16 ** n_inputs)[:count]
        vals = np.array([[(int(x) >> (4 * (n_inputs - 1 - q))) & 15 for q in range(n_inputs)] for x in tuples], dtype=U64)
        cts = ck.encrypt(vals.reshape(-1))
        in_idx = np.arange(count * n_inputs, dtype=np.int32).reshape(count, n_inputs)
        out_idx = np.arange(count * n_inputs, count * (n_inputs + n_out), dtype=np.int32).reshape(count, n_out)

        def run(lo, hi):
            w = fresh(sk, cts, count * (n_inputs + n_out))
            wsk.eval_many_luts(w, in_idx[lo:hi], truth[lo:hi], out_idx[lo:hi], bits_per_block=bpb)
            rows = w.download(out_idx[lo:hi].reshape(-1))
            w.free()
            return rows

        whole = run(0, count)
        parts = np.concatenate([run(0, 700), run(700, count)])
        assert np.array_equal(whole, parts), "rows %s differ" % sorted({int(g) for g in np.argwhere(whole != parts)[:, 0]})[:8]
        dec = ck.decrypt_message_and_carry(whole).reshape(count, n_out)
        assert [[int(v) for v in r] for r in dec] == expected(ck, vals, truth, bpb)
    finally:
        close(keys)


# ---- 6: sharded -----------------------------------------------------------------------------------------------------
def _world1_exchange(sk, capacity_rows):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    sk.set_stream(torch.cuda.current_stream().cuda_stream)
    stage = torch.zeros((capacity_rows, sk.dim + 1), dtype=torch.int64, device=dev)
    gather = torch.zeros((capacity_rows, sk.dim + 1), dtype=torch.int64, device=dev)

    def exchange(_user, rows):
        gather[:rows].copy_(stage[:rows])
        return 0

    fn = nv.SI_EXCHANGE_FN(exchange)
    nv.hip_check(nv.hip.helm_si_set_exchange(sk._h, 0, 1, 1, nv.vp(stage.data_ptr()), nv.vp(gather.data_ptr()), capacity_rows, fn,
                                             None))
    return fn, stage, gather


@pytest.mark.parametrize("bpb,n_out", [(2, 4), (4, 3)])     # 6 bits (no tree), 12 bits (a tree)
def test_sharded_world_one_with_a_callback(bpb, n_out):
    keys = make_keys("si_toy_512", "wop_toy_512", seed=70)
    ck, wk, sk, wsk = keys
    try:
        count = 5
        assert wsk.many_form(3 * bpb, n_out) == 1
        vals, truth, cts, in_idx, out_idx = groups_case(ck, 3, bpb, n_out, count, seed=70 + bpb)
        rows = count * (3 + n_out)
        w = fresh(sk, cts, rows)
        wsk.eval_many_luts(w, in_idx, truth, out_idx, bits_per_block=bpb)
        want = w.download()
        w.free()
        keep = _world1_exchange(sk, 2 * n_out + 1)          # two groups per round: three rounds
        w = fresh(sk, cts, rows)
        wsk.eval_many_luts(w, in_idx, truth, out_idx, bits_per_block=bpb)
        sk.sync()
        assert np.array_equal(w.download(), want)
        assert sk.exchange_stats()[0] == 3
        nv.hip_check(nv.hip.helm_si_set_exchange(sk._h, 0, 1, 1, None, None, 1, nv.SI_EXCHANGE_FN(0), None))
        keep2 = _world1_exchange(sk, n_out - 1)
        with pytest.raises(nv.HelmError, match="exceeds the exchange's capacity_rows"):
            wsk.eval_many_luts(w, in_idx, truth, out_idx, bits_per_block=bpb)
        nv.hip_check(nv.hip.helm_si_set_exchange(sk._h, 0, 1, 1, None, None, 1, nv.SI_EXCHANGE_FN(0), None))
        del keep, keep2
        w.free()
    finally:
        close(keys)


@pytest.mark.parametrize("bpb,n_out", [(2, 4), (4, 3)])
def test_sharded_two_rank_threads(bpb, n_out):
    from helm_amd.comm import Comm
    sp, a, b = si_named_params("si_toy_512")
    wp, c, d = wopbs.wop_named_params("wop_toy_512")
    ck = helm_amd.SiClientKey(sp, a, b, seed=80)
    wk = wopbs.WopClientKey(ck, wp, c, d, seed=81)
    count, world = 5, 2
    vals, truth, cts, in_idx, out_idx = groups_case(ck, 3, bpb, n_out, count, seed=80 + bpb)
    rows = count * (3 + n_out)
    sk0 = helm_amd.SiServerKey(ck)
    wsk0 = wopbs.WopServerKey(sk0, wk)
    w0 = fresh(sk0, cts, rows)
    wsk0.eval_many_luts(w0, in_idx, truth, out_idx, bits_per_block=bpb)
    want = w0.download()
    wsk0.close()
    sk0.close()
    comms = Comm.in_process_group([0] * world)
    ranks, errors = [], []
    for r in range(world):
        sk = helm_amd.SiServerKey(ck)
        wsk = wopbs.WopServerKey(sk, wk)
        w = fresh(sk, cts, rows)
        sk.set_exchange_comm(comms[r], min_batch=1, capacity_rows=2 * n_out)
        sk.sync()
        ranks.append((sk, wsk, w))

    def rank_main(r):
        try:
            sk, wsk, w = ranks[r]
            wsk.eval_many_luts(w, in_idx, truth, out_idx, bits_per_block=bpb)
            sk.sync()
        except BaseException as e:  # noqa: BLE001
            errors.append((r, repr(e)))
            comms[r].abort_group()
    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
        assert not t.is_alive(), "a rank thread is stuck"
    assert not errors, errors
    for r, (sk, wsk, w) in enumerate(ranks):
        assert np.array_equal(w.download(), want), f"rank {r}'s table differs from the unsharded call"
        sk.set_exchange_comm(None)
        wsk.close()
        sk.close()
    for cm in comms:
        cm.destroy()


# ---- 7: LutCircuit --------------------------------------------------------------------------------------------------
def test_lut_circuit_shares_the_front_stages_of_an_sbox(toy2048):
    from helm_amd import Circuit, LutCircuit, PtxtType, verilog_parser
    ck, wk, sk, wsk = toy2048
    # the netlist format holds a 64-bit table constant (entries 0..63; the rest of an 8-input table reads 0)
    consts = [int(v) for v in np.random.default_rng(90).integers(1, 1 << 63, size=8)]
    assert len(set(consts)) == 8
    names = "abcdefgh"
    lines = ["input a, b, c, d, e, f, g, h;", "output " + ", ".join(f"y{o}" for o in range(8)) + ", z;"]
    for o in range(8):
        lines.append(f"lut s{o}(0x{consts[o]:016X}, a, b, c, d, e, f, g, h, y{o});")
    lines.append(f"lut sp(0x{consts[3]:016X}, b, a, c, d, e, f, g, h, z);")        # the same wires in another order
    gates_set, wire_set, input_wires, output_wires, dffs, _, _ = verilog_parser.read_verilog_text("\n".join(lines) + "\n", False)
    circuit = Circuit(gates_set, input_wires, output_wires, dffs)
    circuit.sort_circuit()
    circuit.compute_levels()
    lc = LutCircuit(ck, sk, circuit)
    L = wk.params.cbs_l
    front = 8 + 8 * L
    results = {}
    for share in (False, True):
        lc.set_wide_lut_key(wsk, bits_per_block=1, share=share)
        for x in (0x00, 0x3F, 0x2A, 0xC3):
            inputs = {n: PtxtType.Bool((x >> (7 - i)) & 1) for i, n in enumerate(names)}
            ptxt = circuit.evaluate(circuit.initialize_wire_map(wire_set, inputs, "bool"))
            wsk.timing(reset=True)
            enc = lc.evaluate_encrypted(lc.encrypt_inputs(wire_set, inputs), 1, "bool")
            t = wsk.timing(reset=True)
            dec = {wire: ck.decrypt(enc[wire]) for wire in ptxt}
            assert dec == {wire: int(bool(v)) for wire, v in ptxt.items()}, (share, x)
            results[(share, x)] = dec
            # the timing record counts what ran: 9 outputs; front stages per gate (off) or per group (on: the eight + the one)
            assert t["gates"] == 9
            assert t["bootstraps"] == (2 if share else 9) * front + 9, (share, t)
        assert lc.pbs_per_cycle() == (2 if share else 9) * front + 9
    assert all(results[(True, x)] == results[(False, x)] for x in (0x00, 0x3F, 0x2A, 0xC3))


# ---- 8: the bound-counting build --------------------------------------------------------------------------------------
CHILD = r"""
import json, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import helm_amd
import test_gpu_wop_many as T
keys = T.make_keys("si_toy_512", "wop_toy_512", seed=5)
ck, wk, sk, wsk = keys
sk.bound_violations(reset=True)
res = {}
for name, bpb, n_out in (("no_tree", 2, 4), ("tree", 4, 3)):
    vals, truth, cts, in_idx, out_idx = T.groups_case(ck, 3, bpb, n_out, 3, seed=9)
    w = T.fresh(sk, cts, 3 * (3 + n_out))
    wsk.eval_many_luts(w, in_idx, truth, out_idx, bits_per_block=bpb)
    dec = ck.decrypt_message_and_carry(w.download(out_idx.reshape(-1))).reshape(3, n_out)
    res[name] = {"form": wsk.many_form(3 * bpb, n_out), "decrypt_ok": [[int(v) for v in r] for r in dec] == T.expected(ck, vals, truth, bpb),
                 "violations": sk.bound_violations(reset=True)}
T.close(keys)
print("RESULT " + json.dumps(res))
"""


def test_both_forms_under_the_bound_counting_build():
    lib = os.path.join(ROOT, "helm_amd", "csrc", "libhelm_hip_check.so")
    assert os.path.exists(lib), "make -C helm_amd/csrc libhelm_hip_check.so"
    env = dict(os.environ, HELM_HIP_LIB=lib)
    p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["no_tree"]["form"] == 1 and res["tree"]["form"] == 1
    for name, r in res.items():
        assert r["decrypt_ok"], name
        assert r["violations"] == [0] * 8, (name, r["violations"])
