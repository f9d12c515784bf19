#!/usr/bin/env python3
"""What the keyswitch-first order (pbs_order = 1) costs beside the bootstrap-first one, on boolean_default's shape with the
SAME key material (same seed; only pbs_order differs): one process, the orders alternated inside every repeat, 7 repeats,
median [min - max] of the wall time of one call (stream synchronised), one JSON line per (case, order) appended to
profiles/r19/bench_ks_first.jsonl.
  (a) one launch of 4,096 AND gates                 + the helm_hip_timing split (pbs / keyswitch / linear), from a second
                                                      set of repeats with the event timing on
  (b) one launch of 4,096 gates, a quarter MUX      5,120 bootstraps
  (c) one AES-128 evaluation through GateCircuit    the FIPS-197 vector, checked after decryption
In order 1 the keyswitch scope holds the gate keyswitch (k_ks_gate_digits + k_ks_mfma) and k_big_out; the bootstrap kernel
and its count are the same in both orders.  For the kernels by name run the same command under
`rocprofv3 --kernel-trace --stats` (a run of its own: tracing slows the host).

--root DIR imports helm_amd from another checkout of the project (an A/B of order 0 against an older build, which knows
nothing of order 1: --orders 0).
usage: bench_ks_first.py [--cases a,b,c] [--orders 0,1] [--repeats 7] [--out profiles/r19/bench_ks_first.jsonl] [--tag T]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AND, MUX = 0, 3


def stats(ts):
    return {"min_ms": round(min(ts), 4), "median_ms": round(statistics.median(ts), 4), "max_ms": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--orders", default="0,1")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "bench_ks_first.jsonl"))
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import numpy as np
    import helm_amd
    from helm_amd import Circuit, GateCircuit, PtxtType, verilog_parser

    cases, orders = a.cases.split(","), [int(o) for o in a.orders.split(",")]
    B = 4096
    side = {}
    for order in orders:
        p, lwe_std, glwe_std = helm_amd.named_params("boolean_default")
        p.pbs_order = order
        ck = helm_amd.ClientKey(p, lwe_std, glwe_std, seed=2)
        sk = helm_amd.ServerKey(ck, device=0)
        rng = np.random.default_rng(1)
        bits = rng.integers(0, 2, 3 * B).astype(bool)
        w = sk.wires(4 * B)
        w.upload(np.arange(3 * B), ck.encrypt(bits))
        side[order] = (ck, sk, w, bits)
    i0, i1 = np.arange(B, dtype=np.int32), np.arange(B, 2 * B, dtype=np.int32)
    out = np.arange(3 * B, 4 * B, dtype=np.int32)
    levels = {"a": (np.full(B, AND, np.int32), np.full(B, -1, np.int32))}
    ops_b = np.where(np.arange(B) % 4 == 0, MUX, AND).astype(np.int32)
    levels["b"] = (ops_b, np.where(ops_b == MUX, np.arange(2 * B, 3 * B), -1).astype(np.int32))
    lines = []

    def record(case, order, what, extra):
        ck, sk, _, _ = side[order]
        rec = {"tool": "bench_ks_first", "tag": a.tag, "case": case, "what": what, "pbs_order": order, "repeats": a.repeats,
               "params": list(ck.params.as_tuple7()), "kernel_class": sk.kernel_class(), "field_bits": sk.field_bits()}
        rec.update(extra)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for case in [c for c in cases if c in levels]:
        ops, i2 = levels[case]
        n_pbs = int(B + (ops == MUX).sum())

        def run(order):
            _, sk, w, _ = side[order]
            t0 = time.perf_counter()
            w.eval_gate_level(ops, i0, i1, i2, out)
            sk.sync()
            return (time.perf_counter() - t0) * 1e3

        for order in orders:  # warm-up of every shape the timed window uses, and the values
            run(order)
            ck, sk, w, bits = side[order]
            x, y, c = bits[:B], bits[B:2 * B], bits[2 * B:]
            want = np.where(ops == MUX, np.where(c, x, y), x & y)
            assert np.array_equal(ck.decrypt(w.download(out)), want), (case, order)
        ts = {o: [] for o in orders}
        for _ in range(a.repeats):
            for order in orders:  # alternated
                ts[order].append(run(order))
        for order in orders:
            record(case, order, f"one launch of {B} gates, {n_pbs} bootstraps", dict(stats(ts[order]), bootstraps=n_pbs))
        if case == "a":  # the engine's own split, event timing on: a second set of repeats
            split = {o: [] for o in orders}
            for order in orders:
                side[order][1].timing_enable(True)
                side[order][1].timing(reset=True)
            for _ in range(a.repeats):
                for order in orders:
                    run(order)
                    t = side[order][1].timing(reset=True)
                    split[order].append((t.pbs_ms, t.ks_ms, t.linear_ms, t.pbs_count, t.ks_count))
            for order in orders:
                side[order][1].timing_enable(False)
                s = split[order]
                record("a", order, "helm_hip_timing split of one launch",
                       {"pbs_ms": stats([x[0] for x in s]), "ks_ms": stats([x[1] for x in s]), "linear_ms": stats([x[2] for x in s]),
                        "pbs_count": int(s[0][3]), "ks_count": int(s[0][4])})

    if "c" in cases:
        from helm_amd.netlists import aes128, aes128_reference_encrypt
        gates_set, wire_set, input_wires, output_wires, dffs, _, _ = verilog_parser.read_verilog_text(aes128(), False)
        key, pt = bytes(range(16)), bytes.fromhex("00112233445566778899aabbccddeeff")
        kv, pv = int.from_bytes(key, "big"), int.from_bytes(pt, "big")
        inputs = {f"key[{i}]": PtxtType.Bool((kv >> i) & 1) for i in range(128)}
        inputs.update({f"pt[{i}]": PtxtType.Bool((pv >> i) & 1) for i in range(128)})
        gcs = {}
        for order in orders:
            ck, sk, _, _ = side[order]
            circuit = Circuit(gates_set, input_wires, output_wires, dffs)
            circuit.sort_circuit()
            circuit.compute_levels()
            gc = GateCircuit(ck, sk, circuit)
            gcs[order] = (gc, gc.encrypt_inputs(wire_set, inputs), circuit)

        cycle = [0]

        def run_aes(order):
            gc, enc_in, _ = gcs[order]
            cycle[0] += 1  # a new cycle number: GateCircuit returns its memo for a cycle it has evaluated on this map
            t0 = time.perf_counter()
            enc = gc.evaluate_encrypted(enc_in, cycle[0], "bool")  # ends in helm_hip_sync
            return (time.perf_counter() - t0) * 1e3, enc

        for order in orders:
            _, enc = run_aes(order)
            o = gcs[order][0].decrypt_outputs(enc, False)
            ct = sum(o[f"ct[{i}]"].value << i for i in range(128)).to_bytes(16, "big")
            assert ct == aes128_reference_encrypt(key, pt), order
        ts = {o: [] for o in orders}
        for _ in range(a.repeats):
            for order in orders:
                ts[order].append(run_aes(order)[0])
        for order in orders:
            record("c", order, "one AES-128 evaluation through GateCircuit",
                   dict(stats(ts[order]), bootstraps=int(gcs[order][0].pbs_per_cycle())))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    for order in orders:
        side[order][1].close()


if __name__ == "__main__":
    main()
