"""Effect of the three-input fusion pass (verilog_parser.fuse3) on whole netlists, measured:

    python tools/bench_fuse3.py [--set boolean_default] [--repeats 7] [--out profiles/rNN/bench_fuse3.jsonl]

Netlists: the 32-bit ripple adder, the c880-class ALU, ONE AES-128 evaluation, and AES-128 x 32 blocks.  Each runs unfused
and fused on the same context and key, as a program whose launches are packed the way GateCircuit packs them
(pack_levels with the engine's launch quantum and cost table), alternated, `--repeats` times each: wall time of one pass
(Program.run + sync) as median [min - max], bootstraps and launches per pass.  Every output wire of every block is
decrypted after the last pass and compared with the plaintext evaluator (AES: with the software AES).  One JSON object per
line; the comparison is fused against unfused."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import helm_amd  # noqa: E402
from helm_amd import Circuit, PtxtType, verilog_parser  # noqa: E402
from helm_amd.distributed import gate_pbs, level_arrays, pack_levels  # noqa: E402
from helm_amd.netlists import aes128, aes128_reference_encrypt, alu_c880_class, ripple_adder  # noqa: E402


class Netlist:
    def __init__(self, text):
        gates, self.wire_set, self.inputs, self.outputs, dffs, _, _ = verilog_parser.read_verilog_text(text, False)
        self.circuit = Circuit(gates, self.inputs, self.outputs, dffs)
        self.circuit.sort_circuit()
        self.circuit.compute_levels()
        self.names = list(self.inputs) + sorted(self.wire_set)
        self.index = {w: i for i, w in enumerate(self.names)}
        self.arrays = level_arrays(self.circuit, self.index)

    def plain_outputs(self, bits):
        m = {w: PtxtType.None_() for w in self.wire_set}
        m.update({w: PtxtType.Bool(bits[w]) for w in self.inputs})
        out = self.circuit.evaluate(m)
        return [bool(out[w].value) for w in self.outputs]


def tiled(nl, blocks):
    """`blocks` copies of the netlist side by side: block b lives in rows [b * n_wires, (b + 1) * n_wires)."""
    ops, i0, i1, i2, out, off = nl.arrays
    nw, nlv = len(nl.names), len(off) - 1
    shift = lambda a: np.concatenate([np.concatenate([np.where(a[off[l]:off[l + 1]] >= 0, a[off[l]:off[l + 1]] + b * nw, -1)  # noqa: E731
                                                      for b in range(blocks)]) for l in range(nlv)]).astype(np.int32)
    ops_t = np.concatenate([np.tile(ops[off[l]:off[l + 1]], blocks) for l in range(nlv)]).astype(np.int32)
    return ops_t, shift(i0), shift(i1), shift(i2), shift(out), (off * blocks).astype(np.int64)


class Variant:
    """One netlist text on the context: its packed program, wire table and expected outputs."""

    def __init__(self, sk, ck, text, blocks, inputs_per_block, expected):
        self.nl = nl = Netlist(text)
        arrays = tiled(nl, blocks)
        packed = pack_levels(*arrays, sk.launch_quantum(), quarter_cost=sk.launch_costs())
        self.arrays = packed[:6] if packed[6] else arrays
        self.levels = len(arrays[5]) - 1
        self.launches = len(self.arrays[5]) - 1
        self.bootstraps = int(gate_pbs(arrays[0]).sum())
        self.prog = helm_amd.Program(sk, *self.arrays)
        nw = len(nl.names)
        self.w = sk.wires(nw * blocks)
        rows = np.concatenate([b * nw + np.array([nl.index[x] for x in nl.inputs]) for b in range(blocks)])
        bits = np.concatenate([[inputs_per_block[b][x] for x in nl.inputs] for b in range(blocks)]).astype(bool)
        self.w.upload(rows, ck.encrypt(bits))
        self.out_rows = np.concatenate([b * nw + np.array([nl.index[x] for x in nl.outputs]) for b in range(blocks)])
        self.expected = np.concatenate([expected(nl, inputs_per_block[b]) for b in range(blocks)]).astype(bool)
        self.times = []

    def run(self, sk):
        t0 = time.perf_counter()
        self.prog.run(self.w)
        sk.sync()
        self.times.append(time.perf_counter() - t0)

    def outputs_ok(self, ck):
        return bool(np.array_equal(ck.decrypt(self.w.download(self.out_rows)), self.expected))


def aes_expected(nl, bits):
    key = sum(int(bits[f"key[{i}]"]) << i for i in range(128)).to_bytes(16, "big")
    pt = sum(int(bits[f"pt[{i}]"]) << i for i in range(128)).to_bytes(16, "big")
    ct = int.from_bytes(aes128_reference_encrypt(key, pt), "big")
    return [bool((ct >> int(w[3:-1])) & 1) for w in nl.outputs]


def plain_expected(nl, bits):
    return nl.plain_outputs(bits)


def measure(sk, ck, label, text, blocks, expected, repeats, rng):
    fused_text, stats = verilog_parser.fuse3(text)
    base = Netlist(text)
    inputs = [{w: bool(rng.integers(0, 2)) for w in base.inputs} for _ in range(blocks)]
    variants = {"unfused": Variant(sk, ck, text, blocks, inputs, expected),
                "fused": Variant(sk, ck, fused_text, blocks, inputs, expected)}
    for v in variants.values():      # warm-up: buffers, code objects
        v.run(sk)
        v.times.clear()
    for _ in range(repeats):         # alternated
        for v in variants.values():
            v.run(sk)
    rec = {"netlist": label, "blocks": blocks, "repeats": repeats, "fuse3_stats": list(stats)}
    for name, v in variants.items():
        ms = [t * 1e3 for t in v.times]
        rec[name] = {"bootstraps": v.bootstraps, "levels": v.levels, "launches": v.launches,
                     "wall_ms_median": round(statistics.median(ms), 3), "wall_ms_min": round(min(ms), 3),
                     "wall_ms_max": round(max(ms), 3), "outputs_ok": v.outputs_ok(ck)}
        v.prog.destroy()
        v.w.free()
    rec["speedup_median"] = round(rec["unfused"]["wall_ms_median"] / rec["fused"]["wall_ms_median"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--set", default="boolean_default")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated labels: adder32,c880,aes,aes_x32")
    a = ap.parse_args()
    ck = helm_amd.ClientKey.generate(a.set, seed=1)
    sk = helm_amd.ServerKey(ck)
    rng = np.random.default_rng(0)
    jobs = [("adder32", ripple_adder(32), 1, plain_expected), ("c880", alu_c880_class(), 1, plain_expected),
            ("aes", aes128(), 1, aes_expected), ("aes_x32", aes128(), 32, aes_expected)]
    out = open(a.out, "w") if a.out else None
    for label, text, blocks, expected in jobs:
        if a.only and label not in a.only.split(","):
            continue
        rec = measure(sk, ck, label, text, blocks, expected, a.repeats, rng)
        rec["set"] = a.set
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    sk.close()


if __name__ == "__main__":
    main()
