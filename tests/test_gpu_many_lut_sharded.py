"""helm_si_apply_many_luts under an exchange (helm_si_set_exchange): the batch is cut into `world` contiguous chunks of
ciphertexts, a rank rotates its chunk only, its chunk * n_out extracted rows travel through its exchange slot, and the table
ends word for word as the unsharded call leaves it.  World 1 with a callback (the single-GPU form of the path), then two ranks
on one GPU as tests/test_gpu_two_ranks_si.py rehearses them.  Every case is compared row for row with the unsharded call on a
fresh copy of the same table."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
SET = "si_toy_512"


def _cases(sk, t):
    """name -> (in_idx, out_idx [count, n_out], lut_idx, luts, capacity_rows per world size, exchange rounds per world size)"""
    f2 = [lambda v: (3 * v + 1) % t, lambda v: (5 * v + 2) % t]
    g2 = [lambda v: (v * v) % t, lambda v: (t - 1 - v) % t]
    f3 = [lambda v: (v + 1) % t, lambda v: (2 * v + 3) % t, lambda v: (7 * v) % t]
    luts2 = np.stack([sk.make_many_lut(f2), sk.make_many_lut(g2)])
    luts3 = np.stack([sk.make_many_lut(f3)])
    five = np.arange(5, dtype=np.int32)
    out5 = (8 + np.arange(10, dtype=np.int32)).reshape(5, 2)
    out3 = (8 + np.arange(12, dtype=np.int32)).reshape(4, 3)
    out3[1, 1] = -1                       # skipped outputs
    out3[3, 0] = -1
    out3[2, 2] = 2                        # ... and one over its own input row
    hazard = out5.copy()
    hazard[0, 1] = 4                      # row 4: an output of ciphertext 0 and the input of the last ciphertext
    hazard[1, 0] = 1                      # in place
    return {
        "count 5, n_out 2": (five, out5, five % 2, luts2, {1: 16, 2: 16}, {1: 1, 2: 1}),
        "n_out 3 (M = 4), skipped outputs": (five[:4], out3, np.zeros(4, dtype=np.int32), luts3, {1: 16, 2: 16}, {1: 1, 2: 1}),
        "three exchange rounds": (five, out5, five % 2, luts2, {1: 4, 2: 2}, {1: 3, 2: 3}),
        "an early output is a later input, several rounds": (five, hazard, five % 2, luts2, {1: 4, 2: 2}, {1: 3, 2: 3}),
    }


def _install(sk, rank, world, capacity_rows, dist_mod=None):
    """helm_si_set_exchange with torch buffers.  world 1: the callback copies the stage rows into the gather buffer on the
    engine's stream; otherwise SiServerKey.set_exchange (torch.distributed carries the all-gather)."""
    if world > 1:
        sk.set_exchange(dist_mod, rank, world, min_batch=2, capacity_rows=capacity_rows)
        return
    from helm_amd import _native as nv
    dev = torch.device("cuda", torch.cuda.current_device())
    sk.set_stream(torch.cuda.current_stream().cuda_stream)
    stage = torch.zeros((capacity_rows, sk.dim + 1), dtype=torch.int64, device=dev)
    gather = torch.zeros((capacity_rows, sk.dim + 1), dtype=torch.int64, device=dev)

    def exchange(_user, rows):
        gather[:rows].copy_(stage[:rows])
        return 0

    fn = nv.SI_EXCHANGE_FN(exchange)
    nv.hip_check(nv.hip.helm_si_set_exchange(sk._h, 0, 1, 2, nv.vp(stage.data_ptr()), nv.vp(gather.data_ptr()), capacity_rows, fn,
                                             None))
    sk._exchange = (fn, stage, gather)


def _remove(sk, rank, dist_mod=None):
    from helm_amd import _native as nv
    nv.hip_check(nv.hip.helm_si_set_exchange(sk._h, 0, 1, 1, None, None, 1, nv.SI_EXCHANGE_FN(0), None))
    sk._exchange = None


def _run(rank, world, dist_mod=None):
    """-> list of (case, problem) - empty when everything holds."""
    import helm_amd
    ck = helm_amd.SiClientKey.generate(SET, seed=3)      # the same keys and encryptions on every rank
    sk = helm_amd.SiServerKey(ck)
    t, dim, rows = ck.t, ck.dim, 20
    rng = np.random.default_rng(5)
    sentinel = rng.integers(0, 2**64, size=(rows, dim + 1), dtype=np.uint64)
    cts = ck.encrypt((np.arange(5) % (t // 4)).astype(np.uint64))   # inside the input bound of M = 4 too
    problems = []

    def table():
        w = sk.wires(rows)
        w.upload(np.arange(rows), sentinel)
        w.upload(np.arange(5), cts)
        return w

    sk.timing_enable(True)
    for name, (in_idx, out_idx, lut_idx, luts, cap, rounds) in _cases(sk, t).items():
        ref = table()
        ref.apply_many_luts(in_idx, luts, out_idx, lut_idx)
        want = ref.download()
        _install(sk, rank, world, cap[world], dist_mod)
        w = table()
        b0, r0 = sk.exchange_stats()
        sk.timing(reset=True)
        w.apply_many_luts(in_idx, luts, out_idx, lut_idx)
        sk.sync()
        got = w.download()
        b1, r1 = sk.exchange_stats()
        rotations = int(sk.timing().pbs_count)
        _remove(sk, rank, dist_mod)
        if not np.array_equal(got, want):
            problems.append((name, "rows differ from the unsharded call: %s" % np.nonzero((got != want).any(axis=1))[0].tolist()))
        if b1 - b0 != rounds[world]:
            problems.append((name, "exchange rounds %d, expected %d" % (b1 - b0, rounds[world])))
        if r1 - r0 < len(in_idx) * out_idx.shape[1]:
            problems.append((name, "rows through the gather buffer %d" % (r1 - r0)))
        # this rank's share: per round, chunk `rank` of ceil(per / world) ciphertexts
        n_out, count = out_idx.shape[1], len(in_idx)
        share, base, per_round = 0, 0, (cap[world] // n_out) * world
        while base < count:
            per = min(count - base, per_round)
            chunk = -(-per // world)
            share += max(0, min(per, (rank + 1) * chunk) - min(per, rank * chunk))
            base += per
        if rotations != share:
            problems.append((name, "pbs_count rose by %d, this rank's share is %d" % (rotations, share)))
        # the decrypted values, once
        if name == "count 5, n_out 2":
            dec = ck.decrypt_message_and_carry(got[out_idx.reshape(-1)]).reshape(5, 2)
            fs = [[lambda v: (3 * v + 1) % t, lambda v: (5 * v + 2) % t], [lambda v: (v * v) % t, lambda v: (t - 1 - v) % t]]
            if [[int(x) for x in row] for row in dec] != [[f(g % (t // 4)) for f in fs[g % 2]] for g in range(5)]:
                problems.append((name, "decrypted values"))
    # n_out beyond the slot: refused, nothing written, the context stays usable
    _install(sk, rank, world, 2, dist_mod)
    w = table()
    luts3 = np.stack([sk.make_many_lut([lambda v: v % t, lambda v: (v + 1) % t, lambda v: (v + 2) % t])])
    try:
        w.apply_many_luts([0, 1], luts3, [[8, 9, 10], [11, 12, 13]])
        problems.append(("n_out > capacity_rows", "accepted"))
    except helm_amd.HelmError as e:
        if "capacity_rows" not in str(e) or "error -1:" not in str(e):   # HELM_ERR_INVALID, and it says why
            problems.append(("n_out > capacity_rows", "message: %s" % e))
    before = w.download()
    expect = sentinel.copy()
    expect[:5] = cts
    if not np.array_equal(before, expect):
        problems.append(("n_out > capacity_rows", "the refused call wrote rows"))
    _remove(sk, rank, dist_mod)
    sk.close()
    return problems


def test_world_one_with_a_callback():
    torch.cuda.set_device(0)
    assert _run(0, 1) == []


def _worker(rank, world, port, result_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    problems = _run(rank, world, dist)
    with open(os.path.join(result_dir, f"rank{rank}.txt"), "w") as f:
        f.write(repr(problems))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        assert (tmp_path / f"rank{r}.txt").read_text() == "[]", f"rank {r}"
