#!/usr/bin/env python3
"""What the N = 8192 kernel (k = 1, N = 8192: shortint_m3c3, 6 bits per block) costs beside the 5-bit set and the WoP route.
Four cases in ONE process, alternated (each repeat runs every case once), 7 repeats, median [min - max] of the wall time per
call (stream synchronised):
  (a) one round of 256 apply_luts under shortint_m3c3            k_pbs64_n8192
  (b) the same round under shortint_m2c3                         k_pbs64_large (class 2), for scale
  (c) one LUT level of 256 six-input gates through LutCircuit under shortint_m3c3 (one bootstrap per gate)
  (d) the same 256 gates through the WoP route under shortint_m2c2 (wopbs_m1c1, two bits per block): the route such a gate
      takes without the kernel; (d) / (c) is reported as measured
Every output of (a) and (c) is decrypted and compared - the full-size check of the kernel (shortint_m3c3's key generation
takes minutes on the CPU, so it is not a test of the suite) - and so are (b) and (d).  One JSON line per case, written to
profiles/r21/bench_n8192.jsonl (a run replaces the file).  The measurements run in one fresh child process under its own
time limit; a case whose output decrypts wrong makes the tool fail.
usage: bench_n8192.py [--repeats 7] [--out profiles/r21/bench_n8192.jsonl] [--timeout 1100]"""
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
ROWS, GATES, ARITY = 256, 256, 6


def note(msg):
    print("[bench_n8192] %%s (%%.0f s)" %% (msg, time.perf_counter() - T0), file=sys.stderr, flush=True)


def full_round(run, ck, sk):
    t = ck.t
    vals = (np.arange(ROWS) %% t).astype(np.uint64)
    w = sk.wires(2 * ROWS)
    w.upload(np.arange(ROWS), ck.encrypt(vals))
    f = lambda v: (3 * v + 1) %% t
    lut = sk.make_lut(f)[None]
    inp, out = np.arange(ROWS, dtype=np.int32), np.arange(ROWS, 2 * ROWS, dtype=np.int32)

    def one():
        w.apply_luts(inp, lut, out)
        sk.sync()

    def check():
        got = ck.decrypt_message_and_carry(w.download(out))
        return [int(v) for v in got] == [f(int(v)) for v in vals]
    rec = {"run": run, "kernel_class": sk.kernel_class(), "field_bits": sk.field_bits(), "rows": ROWS,
           "round_capacity": int(sk.round_capacity())}
    return one, check, rec


def lut_level(ck, sk):
    """256 six-input gates with random truth tables over 16 input bits, one level, through LutCircuit (no wide-LUT key)."""
    rng = np.random.default_rng(6)
    lines = ["module level6(x, y);", "  input [15:0] x;", "  output [%%d:0] y;" %% (GATES - 1)]
    for g in range(GATES):
        ins = rng.choice(16, size=ARITY, replace=False)
        lines.append("  lut g%%d(0x%%016X, %%s, y[%%d]);" %% (g, int(rng.integers(1, 2**63 - 1)), ", ".join("x[%%d]" %% i for i in ins), g))
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
    state = {"cycle": 0, "out": None}

    def one():
        state["cycle"] += 1
        state["out"] = EvalCircuit.evaluate_encrypted(lc, enc_in, state["cycle"], "bool")
        sk.sync()

    rec = {"run": "c_lut_level_6_input_gates_m3c3", "route": "LutCircuit, one bootstrap per gate", "gates": GATES,
           "arity": ARITY}

    def check():
        rec["rotations"] = lc.pbs_per_cycle()    # (counted by the evaluations above)
        return all(ck.decrypt(state["out"][wire]) == int(bool(want)) for wire, want in ptxt.items())
    return one, check, rec, lc


def wop_level():
    """The same number of six-input gates through the WoP route (tools/bench_large_n.py's set-up)."""
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

    def check():
        got = ck.decrypt_message_and_carry(w.download(out_idx))
        want = [int(truth[sum(int(v) * basis ** j for j, v in enumerate(r[::-1]))]) for r in bits_in]
        return [int(v) for v in got] == want
    rec = {"run": "d_wop_6_input_gates_m2c2", "route": "WoP-PBS, wopbs_m1c1, two bits per block", "gates": GATES, "arity": ARITY}
    return one, check, rec, (wsk, sk)


T0 = time.perf_counter()
ck6 = helm_amd.SiClientKey.generate("shortint_m3c3", seed=1)
note("shortint_m3c3 key generated")
sk6 = helm_amd.SiServerKey(ck6, generic="n8192")
ck5 = helm_amd.SiClientKey.generate("shortint_m2c3", seed=1)
sk5 = helm_amd.SiServerKey(ck5, generic="large")
note("server keys loaded")
cases = []
one, check, rec = full_round("a_round_256_m3c3_n8192", ck6, sk6); cases.append((one, check, rec))
one, check, rec = full_round("b_round_256_m2c3_large", ck5, sk5); cases.append((one, check, rec))
one, check, rec, keep_c = lut_level(ck6, sk6); cases.append((one, check, rec))
one, check, rec, keep_d = wop_level(); cases.append((one, check, rec))
note("cases set up")
for one, _, _ in cases:      # warm-up, every case once
    one()
times = [[] for _ in cases]
for _ in range(repeats):     # alternated: each repeat runs every case once
    for i, (one, _, _) in enumerate(cases):
        t0 = time.perf_counter(); one(); times[i].append((time.perf_counter() - t0) * 1e3)
for (one, check, rec), ts in zip(cases, times):
    rec.update({"repeats": repeats, "min_ms": round(min(ts), 3), "median_ms": round(statistics.median(ts), 3),
                "max_ms": round(max(ts), 3), "decrypt_ok": bool(check())})
    n = rec.get("gates", rec.get("rows"))
    rec["per_s"] = round(n / (rec["median_ms"] * 1e-3), 1)
    print("RESULT " + json.dumps(rec), flush=True)
'''


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "bench_n8192.jsonl"))
    ap.add_argument("--timeout", type=int, default=1100)
    args = ap.parse_args()
    # one fresh process, under its own time limit (timeout -k: a hung GPU step is ended, nothing is started after it)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, "-c", CHILD % (ROOT, args.repeats)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)  # (the child's progress notes go straight to stderr)
    lines = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:  # (a run replaces the file: four records, one run)
        for ln in lines:
            fh.write(ln + "\n")
            print(ln)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:])
        return p.returncode
    recs = {json.loads(ln)["run"]: json.loads(ln) for ln in lines}
    c, d = recs.get("c_lut_level_6_input_gates_m3c3"), recs.get("d_wop_6_input_gates_m2c2")
    if c and d:
        print("six-input gates per second: LutCircuit on shortint_m3c3 %.1f, WoP route on shortint_m2c2 %.1f (d / c = x %.2f)" %
              (c["per_s"], d["per_s"], d["median_ms"] / c["median_ms"]))
    return 0 if len(lines) == 4 and all(json.loads(ln)["decrypt_ok"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
