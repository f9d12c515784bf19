#!/usr/bin/env python3
"""What the bootstrap-first order of the 64-bit engine (HELM_SI_CREATE_PBS_KS, SiServerKey(order="pbs_ks")) costs beside
the keyswitch-first one, on shortint_m2c2's shape with ONE key (the keys are the same in both orders): one process, the
orders alternated inside every repeat, 7 repeats, median [min - max] of the wall time of one call (stream synchronised), one
JSON line per (case, order) appended to profiles/r20/bench_pbs_first.jsonl.
  (a) one round of 256 helm_si_apply_luts            the same kernels and the same counts in both orders
  (c) helm_si_lincomb of 4,096 rows x 3 terms        row widths 2,049 and 743 words
  (d) chi-squared u32 through ArithCircuit           checked after decryption
  (e) bytes handed to the exchange per look-up       a world-1 exchange through the library's communicator: exchange_stats
                                                     rows x the row width, and the communicator's own byte count
(b), order 1 against the parent commit's library, is case (a) run from a checkout of the parent:
    bench_pbs_first.py --root PARENT_CHECKOUT --orders 1 --cases a --tag parent
(a build that knows nothing of order 0), alternated with `--orders 1 --cases a --tag branch` runs of this tree.
The key is generated with the set's shape and a lowered LWE noise (1e-9): at n = 742 the set's own noise is chosen for order 1
(helm_client64.cpp, shortint_m2c2_pbs_ks), and no timing depends on the noise.
usage: bench_pbs_first.py [--cases a,c,d,e] [--orders 1,0] [--repeats 7] [--out profiles/r20/bench_pbs_first.jsonl] [--tag T]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER_NAME = {1: "ks_pbs", 0: "pbs_ks"}


def stats(ts):
    return {"min_ms": round(min(ts), 4), "median_ms": round(statistics.median(ts), 4), "max_ms": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,c,d,e")
    ap.add_argument("--orders", default="1,0")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "bench_pbs_first.jsonl"))
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import numpy as np
    import helm_amd
    from helm_amd import ArithCircuit, Circuit, verilog_parser

    cases, orders = a.cases.split(","), [int(o) for o in a.orders.split(",")]
    p, _, glwe_std = helm_amd.si_named_params("shortint_m2c2")
    ck = helm_amd.SiClientKey(p, 1e-9, glwe_std, seed=2)
    t = ck.t
    side = {}
    for order in orders:
        # (a checkout that knows nothing of the order takes no such argument)
        sk = helm_amd.SiServerKey(ck, order=ORDER_NAME[order]) if order == 0 else helm_amd.SiServerKey(ck)
        words = sk.wire_words() if hasattr(sk, "wire_words") else ck.dim + 1
        side[order] = (sk, words)
    enc = lambda order, v: ck.encrypt(v, small=True) if order == 0 else ck.encrypt(v)                      # noqa: E731
    dec = lambda order, c: ck.decrypt_message_and_carry(c, small=True) if order == 0 else ck.decrypt_message_and_carry(c)  # noqa: E731
    lines = []

    def record(case, order, what, extra):
        sk, words = side[order]
        rec = {"tool": "bench_pbs_first", "tag": a.tag, "case": case, "what": what, "pbs_order": order, "repeats": a.repeats,
               "params": list(ck.params.as_tuple()), "wire_words": int(words), "kernel_class": sk.kernel_class()}
        rec.update(extra)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def timed(fn, sync):
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e3

    def alternate(run):
        for order in orders:
            run(order)          # warm-up of every shape the timed window uses
        ts = {o: [] for o in orders}
        for _ in range(a.repeats):
            for order in orders:
                ts[order].append(run(order))
        return ts

    f = lambda v: (5 * v + 3) % t   # noqa: E731
    if "a" in cases or "e" in cases:
        B = 256
        vals = (np.arange(B) % t).astype(np.uint64)
        tabs = {}
        for order in orders:
            sk, _ = side[order]
            w = sk.wires(2 * B)
            w.upload(np.arange(B), enc(order, vals))
            tabs[order] = (w, sk.make_lut(f))
        idx_in, idx_out = np.arange(B, dtype=np.int32), np.arange(B, 2 * B, dtype=np.int32)

        def run_a(order):
            sk, _ = side[order]
            w, lut = tabs[order]
            return timed(lambda: w.apply_luts(idx_in, lut, idx_out), sk.sync)

    if "a" in cases:
        ts = alternate(run_a)
        for order in orders:
            w, _ = tabs[order]
            assert [int(v) for v in dec(order, w.download(idx_out))] == [f(int(v)) for v in vals], order
            record("a", order, "one round of 256 apply_luts", dict(stats(ts[order]), look_ups=B))
        split = {o: [] for o in orders}
        for order in orders:
            side[order][0].timing_enable(True)
            side[order][0].timing(reset=True)
        for _ in range(a.repeats):
            for order in orders:
                run_a(order)
                tm = side[order][0].timing(reset=True)
                split[order].append((tm.pbs_ms, tm.ks_ms, tm.pbs_count, tm.ks_count))
        for order in orders:
            side[order][0].timing_enable(False)
            s = split[order]
            record("a", order, "helm_si_timing split of one round", {"pbs_ms": stats([x[0] for x in s]), "ks_ms": stats([x[1] for x in s]),
                                                                     "pbs_count": int(s[0][2]), "ks_count": int(s[0][3])})

    if "c" in cases:
        R = 4096
        lin = {}
        for order in orders:
            sk, words = side[order]
            w = sk.wires(4 * R)
            rows = np.random.default_rng(3).integers(0, 2**64, size=(3 * R, words), dtype=np.uint64)
            w.upload(np.arange(3 * R), rows)
            lin[order] = w
        in_idx = np.arange(3 * R, dtype=np.int32).reshape(3, R).T.copy()
        coef = np.tile(np.array([4, 2, 1], dtype=np.int64), (R, 1))
        out_idx = np.arange(3 * R, 4 * R, dtype=np.int32)
        ts = alternate(lambda order: timed(lambda: lin[order].lincomb(in_idx, coef, out_idx), side[order][0].sync))
        for order in orders:
            record("c", order, "lincomb of 4096 rows x 3 terms", dict(stats(ts[order]), rows=R, terms=3))
            lin[order].free()

    if "d" in cases:
        net = os.path.join(ROOT, "tests", "netlists", "chi_squared_arith.v")
        gs, ws, ins, outs, dffs, _, _ = verilog_parser.read_verilog_file(net, True)
        inputs = verilog_parser.read_input_wires(os.path.join(ROOT, "tests", "golden", "chi_squared_arith_1.inputs.csv"), "u32")
        acs = {}
        for order in orders:
            c = Circuit(gs, ins, outs, dffs)
            c.sort_circuit()
            c.compute_levels()
            ac = ArithCircuit(ck, side[order][0], c)
            acs[order] = (ac, ac.encrypt_inputs(ws, inputs), c)
        cycle = [0]
        last = {}

        def run_d(order):
            ac, enc_in, _ = acs[order]
            cycle[0] += 1       # a new cycle number defeats the same-cycle memo
            t0 = time.perf_counter()
            last[order] = ac.evaluate_encrypted(enc_in, cycle[0], "u32")
            side[order][0].sync()
            return (time.perf_counter() - t0) * 1e3

        ts = alternate(run_d)
        for order in orders:
            out = {k: v.value for k, v in acs[order][0].decrypt_outputs(last[order], False).items()}
            assert out == {"alpha": 529, "beta1": 242, "beta2": 275, "beta3": 1250}, (order, out)
            record("d", order, "chi-squared u32 through ArithCircuit",
                   dict(stats(ts[order]), bootstraps=int(acs[order][0].pbs_per_cycle()), rounds=int(acs[order][0].pbs_rounds_per_cycle())))

    if "e" in cases:
        from helm_amd.comm import Comm
        for order in orders:
            sk, words = side[order]
            comm = Comm.in_process_group([0])[0]
            sk.set_exchange_comm(comm, min_batch=1, capacity_rows=256)
            b0, r0 = sk.exchange_stats()
            s0 = comm.stats()["bytes_sent"]
            run_a(order)
            b1, r1 = sk.exchange_stats()
            sent = comm.stats()["bytes_sent"] - s0
            sk.set_exchange_comm(None)
            comm.destroy()
            assert sent == (r1 - r0) * words * 8, (order, sent, r1 - r0, words)
            record("e", order, "bytes handed to the exchange per look-up (world 1, 256 look-ups)",
                   {"exchange_rounds": b1 - b0, "exchange_rows": r1 - r0, "bytes_sent": int(sent), "bytes_per_look_up": sent / B})

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")
    for order in orders:
        side[order][0].close()


if __name__ == "__main__":
    main()
