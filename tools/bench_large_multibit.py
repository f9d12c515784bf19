#!/usr/bin/env python3
"""What multi-bit blind rotation costs and saves on the two large-N kernels (k_pbs64_large<12, g>, k_pbs64_n8192<g>) beside
their classical form.  Seven cases in ONE process, alternated (each repeat runs every case once), 7 repeats, median
[min - max] of the wall time per call (stream synchronised):
  (a) one round of 256 apply_luts under shortint_m3c3                      k_pbs64_n8192<0>, 864 steps
  (b) the same under shortint_m3c3_multibit3                               k_pbs64_n8192<3>, 288 group steps
  (c) the same under shortint_m3c3's values with grouping_factor = 2       k_pbs64_n8192<2>, 432 group steps
  (d) the same under shortint_m2c3                                         k_pbs64_large<12, 0>, 1024 steps, PBS 22 x 1
  (e) the same under shortint_m2c3_multibit3                               k_pbs64_large<12, 3>, 341 group steps, PBS 15 x 2
  (f) one LUT level of 256 six-input gates through LutCircuit under shortint_m3c3
  (g) the same level under shortint_m3c3_multibit3
Every output is decrypted and compared; key generation is timed outside the measured region and reported per record.  Each
record carries the transforms and pointwise products of one step and per consumed mask word, so that the measured ratios
stand beside the operation counts.  One JSON line per case, written to profiles/r22/bench_large_multibit.jsonl (a run replaces
the file).  The measurements run in one fresh child process under its own time limit; a case whose output decrypts wrong
makes the tool fail.
usage: bench_large_multibit.py [--repeats 7] [--out profiles/r22/bench_large_multibit.jsonl] [--timeout 1100]
                               [--classical-only]   (cases a, d and f only: what a library without the multi-bit form runs,
                                                     HELM_HIP_LIB chooses the library)"""
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
from helm_amd import Circuit, EvalCircuit, LutCircuit, PtxtType, verilog_parser
from helm_amd.shortint import si_named_params
repeats, classical_only = %d, %d
ROWS, GATES, ARITY = 256, 256, 6


def note(msg):
    print("[bench_large_multibit] %%s (%%.0f s)" %% (msg, time.perf_counter() - T0), file=sys.stderr, flush=True)


def counts(p):
    """Per step of the kernel that runs p: transforms (forward + inverse) and pointwise modular products per coefficient
    and field - monomial products d^ M(e_S) and key products - and the same per consumed mask word."""
    g = max(1, p.grouping_factor)
    l, sub = p.pbs_l, 1 << g if g > 1 else 1
    if p.N == 8192:    # form (a): per column all 2 l digit polynomials go forward, one column sum comes back
        transforms, mono, keyp = 2 * (2 * l + 1), 2 * 2 * l * (sub - 1), 2 * 2 * l * sub
    else:              # both columns from one pass over the 2 l digit polynomials
        transforms, mono, keyp = 2 * l + 2, 2 * l * (sub - 1), 2 * 2 * l * sub
    return {"steps": p.n // g, "transforms_per_step": transforms, "monomial_products_per_step": mono,
            "key_products_per_step": keyp, "transforms_per_mask_word": round(transforms / g, 3),
            "products_per_mask_word": round((mono + keyp) / g, 3)}


def make(name, mode, group=None):
    t0 = time.perf_counter()
    if group is None:
        ck = helm_amd.SiClientKey.generate(name, seed=1)
    else:
        p, a, b = si_named_params(name)
        p.grouping_factor = group
        ck = helm_amd.SiClientKey(p, a, b, seed=1)
    keygen = time.perf_counter() - t0
    sk = helm_amd.SiServerKey(ck, generic=mode)
    note("%%s g=%%d: key generated in %%.1f s, loaded" %% (name, max(1, ck.params.grouping_factor), keygen))
    return ck, sk, round(keygen, 2)


def full_round(run, ck, sk, keygen):
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
    p = ck.params
    rec = {"run": run, "kernel_class": sk.kernel_class(), "field_bits": sk.field_bits(), "rows": ROWS,
           "n": p.n, "N": p.N, "pbs": [p.pbs_l, p.pbs_logB], "grouping_factor": max(1, p.grouping_factor),
           "keygen_s": keygen}
    rec.update(counts(p))
    return one, check, rec


def lut_level(run, ck, sk, keygen):
    """256 six-input gates with random truth tables over 16 input bits, one level, through LutCircuit."""
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

    rec = {"run": run, "route": "LutCircuit, one bootstrap per gate", "gates": GATES, "arity": ARITY,
           "grouping_factor": max(1, ck.params.grouping_factor), "keygen_s": keygen}

    def check():
        rec["rotations"] = lc.pbs_per_cycle()
        return all(ck.decrypt(state["out"][wire]) == int(bool(want)) for wire, want in ptxt.items())
    return one, check, rec, lc


T0 = time.perf_counter()
cases, keep = [], []
ck, sk, kg = make("shortint_m3c3", "n8192")
cases.append(full_round("a_round_256_m3c3", ck, sk, kg))
r = lut_level("f_lut_level_6_input_gates_m3c3", ck, sk, kg); cases.append(r[:3]); keep.append(r[3])
ck5, sk5, kg5 = make("shortint_m2c3", "large")
cases.append(full_round("d_round_256_m2c3", ck5, sk5, kg5))
if not classical_only:
    ckb, skb, kgb = make("shortint_m3c3_multibit3", "n8192+multibit")
    cases.append(full_round("b_round_256_m3c3_multibit3", ckb, skb, kgb))
    r = lut_level("g_lut_level_6_input_gates_m3c3_multibit3", ckb, skb, kgb); cases.append(r[:3]); keep.append(r[3])
    ckc, skc, kgc = make("shortint_m3c3", "n8192+multibit", group=2)
    cases.append(full_round("c_round_256_m3c3_group2", ckc, skc, kgc))
    cke, ske, kge = make("shortint_m2c3_multibit3", "large+multibit")
    cases.append(full_round("e_round_256_m2c3_multibit3", cke, ske, kge))
note("cases set up")
for one, _, _ in cases:      # warm-up, every case once
    one()
times = [[] for _ in cases]
for _ in range(repeats):     # alternated: each repeat runs every case once
    for i, (one, _, _) in enumerate(cases):
        t0 = time.perf_counter(); one(); times[i].append((time.perf_counter() - t0) * 1e3)
for (one, check, rec), ts in sorted(zip(cases, times), key=lambda x: x[0][2]["run"]):
    rec.update({"repeats": repeats, "min_ms": round(min(ts), 3), "median_ms": round(statistics.median(ts), 3),
                "max_ms": round(max(ts), 3), "decrypt_ok": bool(check())})
    n = rec.get("gates", rec.get("rows"))
    rec["per_s"] = round(n / (rec["median_ms"] * 1e-3), 1)
    print("RESULT " + json.dumps(rec), flush=True)
'''


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "bench_large_multibit.jsonl"))
    ap.add_argument("--timeout", type=int, default=1100)
    ap.add_argument("--classical-only", action="store_true")
    args = ap.parse_args()
    # one fresh process, under its own time limit (timeout -k: a hung GPU step is ended, nothing is started after it)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, "-c", CHILD % (ROOT, args.repeats, int(args.classical_only))]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)  # (the child's progress notes go straight to stderr)
    lines = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:  # (a run replaces the file)
        for ln in lines:
            fh.write(ln + "\n")
            print(ln)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:])
        return p.returncode
    recs = {json.loads(ln)["run"][0]: json.loads(ln) for ln in lines}
    for num, den, what in (("a", "b", "m3c3 round, classical / multibit3"), ("a", "c", "m3c3 round, classical / group 2"),
                           ("d", "e", "m2c3 round, classical 22 x 1 / multibit3 15 x 2"),
                           ("f", "g", "six-input LUT level, classical / multibit3")):
        if num in recs and den in recs:
            print("%s: %.1f ms / %.1f ms = x %.2f" % (what, recs[num]["median_ms"], recs[den]["median_ms"],
                                                      recs[num]["median_ms"] / recs[den]["median_ms"]))
    want = 3 if args.classical_only else 7
    return 0 if len(lines) == want and all(json.loads(ln)["decrypt_ok"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
