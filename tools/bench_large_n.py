#!/usr/bin/env python3
"""What the large-N kernel (k = 1, N = 4096: shortint_m2c3, 5 bits per block) costs beside the 4-bit set and the WoP route.
7 repeats each, median [min - max] of the wall time per call (stream synchronised):
  (a) one full round of apply_luts under shortint_m2c3           round_capacity() rows on k_pbs64_large
  (b) the same round under shortint_m2c2 on its tuned kernel
  (c) the same round under shortint_m2c2 with generic="force"    the existing kernel closest in kind
  (d) one LUT level of 256 five-input gates through LutCircuit under shortint_m2c3 (one bootstrap per gate)
  (e) the same 256 gates through the WoP route under shortint_m2c2 (wopbs_m1c1, two bits per block)
One JSON line per measurement, written to profiles/r17/bench_large_n.jsonl (a run replaces the file).  The measurements
run in ONE fresh child process under its own time limit.
usage: bench_large_n.py [--repeats 7] [--out profiles/r17/bench_large_n.jsonl] [--timeout 500]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, os, statistics, sys, tempfile, time
import numpy as np
sys.path.insert(0, %r)
import helm_amd
from helm_amd import Circuit, EvalCircuit, LutCircuit, PtxtType, verilog_parser, wopbs
from helm_amd.shortint import si_named_params
repeats = %d
GATES, ARITY = 256, 5


def timed(fn):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": round(min(ts), 3), "median_ms": round(statistics.median(ts), 3), "max_ms": round(max(ts), 3)}


def emit(rec):
    print("RESULT " + json.dumps(rec), flush=True)


def full_round(run, name, generic):
    ck = helm_amd.SiClientKey.generate(name, seed=1)
    sk = helm_amd.SiServerKey(ck, generic=generic)
    t, B = ck.t, sk.round_capacity()
    vals = (np.arange(B) %% t).astype(np.uint64)
    w = sk.wires(2 * B)
    w.upload(np.arange(B), ck.encrypt(vals))
    f = lambda v: (3 * v + 1) %% t
    lut = sk.make_lut(f)[None]
    inp, out = np.arange(B, dtype=np.int32), np.arange(B, 2 * B, dtype=np.int32)

    def one():
        w.apply_luts(inp, lut, out)
        sk.sync()
    rec = {"run": run, "set": name, "generic": generic, "kernel_class": sk.kernel_class(), "field_bits": sk.field_bits(),
           "rows": int(B), "repeats": repeats, **timed(one)}
    got = ck.decrypt_message_and_carry(w.download(out))
    rec["decrypt_ok"] = [int(v) for v in got] == [f(int(v)) for v in vals]
    rec["us_per_row"] = round(rec["median_ms"] * 1e3 / B, 2)
    emit(rec)
    return ck, sk


def lut_level(ck, sk):
    """256 five-input gates with random truth tables over 16 input bits, one level, through LutCircuit."""
    rng = np.random.default_rng(5)
    lines = ["module level5(x, y);", "  input [15:0] x;", "  output [%%d:0] y;" %% (GATES - 1)]
    for g in range(GATES):
        ins = rng.choice(16, size=ARITY, replace=False)
        lines.append("  lut g%%d(0x%%08X, %%s, y[%%d]);" %% (g, int(rng.integers(1, 2**32 - 1)), ", ".join("x[%%d]" %% i for i in ins), g))
    with tempfile.NamedTemporaryFile("w", suffix=".v", delete=False) as fh:
        fh.write("\n".join(lines + ["endmodule", ""]))
    try:
        gs, ws, ins, outs, d, _, _ = verilog_parser.read_verilog_file(fh.name, False)
    finally:
        os.unlink(fh.name)
    c = Circuit(gs, ins, outs, d)
    c.sort_circuit()
    c.compute_levels()
    inputs = {"x[%%d]" %% i: PtxtType.Bool(int(rng.integers(0, 2))) for i in range(16)}
    ptxt = c.evaluate(c.initialize_wire_map(ws, inputs, "bool"))
    lc = LutCircuit(ck, sk, c)
    lc.set_timing_lines(False)
    enc_in = EvalCircuit.encrypt_inputs(lc, ws, inputs)
    cycle = [0]

    def one():
        cycle[0] += 1
        one.out = EvalCircuit.evaluate_encrypted(lc, enc_in, cycle[0], "bool")
        sk.sync()
    rec = {"run": "d_lut_level_5_input_gates", "set": "shortint_m2c3", "route": "LutCircuit, one bootstrap per gate",
           "gates": GATES, "arity": ARITY, "repeats": repeats, **timed(one)}
    rec["rotations"] = lc.pbs_per_cycle()
    rec["decrypt_ok"] = all(ck.decrypt(one.out[wire]) == int(bool(want)) for wire, want in ptxt.items())
    rec["gates_per_s"] = round(GATES / (rec["median_ms"] * 1e-3), 1)
    emit(rec)


def wop_level():
    """The same number of five-input gates through the WoP route (tools/wop_bench.py's set-up)."""
    sp, sa, sb = si_named_params("shortint_m2c2")
    wp, wa, wb = wopbs.wop_named_params("wopbs_m1c1")
    sp.message_modulus, sp.carry_modulus = wp.message_modulus, wp.carry_modulus
    ck = helm_amd.SiClientKey(sp, sa, sb, seed=1)
    wk = wopbs.WopClientKey(ck, wp, wa, wb, seed=2)
    sk = helm_amd.SiServerKey(ck)
    wsk = wopbs.WopServerKey(sk, wk)
    rng = np.random.default_rng(0)
    basis, m = wp.message_modulus, ARITY
    truth = rng.integers(0, 2, size=basis ** m, dtype=np.uint64)
    xs = rng.integers(0, 1 << m, size=GATES)
    bits_in = np.array([[(x >> (m - 1 - q)) & 1 for q in range(m)] for x in xs], dtype=np.uint64)
    w = sk.wires(GATES * (m + 1))
    w.upload(np.arange(GATES * m), ck.encrypt(bits_in.reshape(-1)))
    in_idx = np.arange(GATES * m, dtype=np.int32).reshape(GATES, m)
    out_idx = np.arange(GATES * m, GATES * (m + 1), dtype=np.int32)

    def one():
        wsk.eval_luts(w, in_idx, truth, out_idx, bits_per_block=2)
        sk.sync()
    rec = {"run": "e_wop_5_input_gates", "set": "shortint_m2c2", "route": "WoP-PBS, wopbs_m1c1, two bits per block",
           "gates": GATES, "arity": ARITY, "repeats": repeats, **timed(one)}
    got = ck.decrypt_message_and_carry(w.download(out_idx))
    want = [int(truth[sum(int(v) * basis ** j for j, v in enumerate(r[::-1]))]) for r in bits_in]
    rec["decrypt_ok"] = [int(v) for v in got] == want
    rec["gates_per_s"] = round(GATES / (rec["median_ms"] * 1e-3), 1)
    emit(rec)
    wsk.close()
    sk.close()


ck3, sk3 = full_round("a_full_round_m2c3_large", "shortint_m2c3", "large")
lut_level(ck3, sk3)
sk3.close()
del ck3, sk3
for run, generic in (("b_full_round_m2c2_tuned", None), ("c_full_round_m2c2_forced_generic", "force")):
    _, sk = full_round(run, "shortint_m2c2", generic)
    sk.close()
wop_level()
'''


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "bench_large_n.jsonl"))
    ap.add_argument("--timeout", type=int, default=500)
    args = ap.parse_args()
    # one fresh process, under its own time limit (timeout -k: a hung GPU step is ended, nothing is started after it)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, "-c", CHILD % (ROOT, args.repeats)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    lines = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:  # (a run replaces the file: five records, one run)
        for ln in lines:
            fh.write(ln + "\n")
            print(ln)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        return p.returncode
    recs = {json.loads(ln)["run"]: json.loads(ln) for ln in lines}
    d, e = recs.get("d_lut_level_5_input_gates"), recs.get("e_wop_5_input_gates")
    if d and e:
        print("five-input gates per second: LutCircuit on shortint_m2c3 %.1f, WoP route on shortint_m2c2 %.1f (x %.2f)" %
              (d["gates_per_s"], e["gates_per_s"], d["gates_per_s"] / e["gates_per_s"]))
    return 0 if len(lines) == 5 and all(json.loads(ln)["decrypt_ok"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
