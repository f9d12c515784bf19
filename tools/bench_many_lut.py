#!/usr/bin/env python3
"""What a many-LUT bootstrap costs beside the plain one: shortint_m2c2, one round of round_capacity() ciphertexts (one
bootstrap per CU), 7 repeats each of
  (a) one apply_luts                              one function, one blind rotation
  (b) two apply_luts with two tables              two functions today: two blind rotations
  (c) one apply_many_luts, n_out = 2              two functions, one blind rotation
  (d) one apply_many_luts, n_out = 4              four functions, one blind rotation
  (s2), (s4) the row scatter of (c) and (d) alone (a row copy of count * n_out rows through the same kernel)
min / median / max of the wall time per call (stream synchronised), one JSON line per measurement, appended to
profiles/r14/bench_many_lut.jsonl.  The measurement runs in ONE fresh child process under its own time limit.
usage: bench_many_lut.py [--repeats 7] [--out profiles/r14/bench_many_lut.jsonl] [--timeout 300]

--operators: what the operators gain from it instead (set_many_lut off / on, shortint_m2c2, 7 repeats, median [min - max] of the
wall time of one evaluation, rotations per evaluation off / on), one JSON line per run appended to
profiles/r15/bench_many_lut_operators.jsonl:
  (a) chi-squared on u32, one evaluation                      the same rounds, fewer rotations in propagate()'s first round
  (b) --copies independent chi-squared circuits in one netlist  their chains' merged rounds exceed helm_si_round_capacity
  (c) one LUT level of 1,024 full-adder pairs                  2,048 gates, 1,024 rotations with the switch on"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, statistics, sys, time
import numpy as np
sys.path.insert(0, %r)
import helm_amd
repeats = %d
ck, sk = helm_amd.gen_keys_shortint("shortint_m2c2", seed=1)
t = ck.t
B = sk.round_capacity()
vals = (np.arange(B) %% 7).astype(np.uint64)            # a block after one addition: at most 6 < t / 2
w = sk.wires(6 * B)
w.upload(np.arange(B), ck.encrypt(vals))
inp = np.arange(B, dtype=np.int32)
msg, carry = sk.make_lut(lambda v: v %% 4), sk.make_lut(lambda v: v // 4)
two = np.stack([msg, carry])
many2 = sk.make_many_lut([lambda v: v %% 4, lambda v: v // 4])
many4 = sk.make_many_lut([lambda v: v %% 4, lambda v: v // 4, lambda v: (v + 1) %% 4, lambda v: int(v == 0)])
out1 = np.arange(B, 2 * B, dtype=np.int32)
out1b = np.arange(2 * B, 3 * B, dtype=np.int32)
out2 = np.arange(B, 3 * B, dtype=np.int32).reshape(B, 2)
out4 = np.arange(B, 5 * B, dtype=np.int32).reshape(B, 4)


def a():
    w.apply_luts(inp, msg, out1)


def b():
    w.apply_luts(inp, two, out1, np.zeros(B, dtype=np.int32))
    w.apply_luts(inp, two, out1b, np.ones(B, dtype=np.int32))


def c():
    w.apply_many_luts(inp, many2, out2)


def d():
    w.apply_many_luts(inp, many4, out4)


def scatter(n):   # the same kernel (a row gather / scatter), the same number of rows
    src = np.arange(B, B + n * B, dtype=np.int32)
    return lambda: w.lincomb(src.reshape(-1, 1), np.ones((n * B, 1), dtype=np.int64), src)


def timed(fn):
    fn(); sk.sync()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter(); fn(); sk.sync(); ts.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": round(min(ts), 4), "median_ms": round(statistics.median(ts), 4), "max_ms": round(max(ts), 4)}


res = {}
for name, fn in (("a_apply_luts", a), ("b_two_apply_luts", b), ("c_many_n_out_2", c), ("d_many_n_out_4", d),
                 ("s2_staged_row_copy_2B", scatter(2)), ("s4_staged_row_copy_4B", scatter(4))):
    res[name] = timed(fn)
c()
got = ck.decrypt_message_and_carry(w.download(out2.reshape(-1))).reshape(B, 2)
ok = bool(np.array_equal(got[:, 0], vals %% 4) and np.array_equal(got[:, 1], vals // 4))
print("RESULT " + json.dumps({"set": "shortint_m2c2", "count": int(B), "repeats": repeats, "decrypt_ok": ok, "timings": res}))
sk.close()
'''


OPERATORS_CHILD = r'''
import json, os, statistics, sys, tempfile, time
import numpy as np
sys.path.insert(0, %r)
import helm_amd
from helm_amd import ArithCircuit, Circuit, PtxtType, verilog_parser
repeats, copies = %d, %d
ck, sk = helm_amd.gen_keys_shortint("shortint_m2c2", seed=1)
cap = sk.round_capacity()
GATES = [("mult", "N0", "N2", "t0"), ("mult", "t0", "4", "t1"), ("mult", "N1", "N1", "t2"), ("sub", "t1", "t2", "t3"),
         ("mult", "t3", "t3", "alpha"), ("mult", "N0", "2", "t4"), ("add", "t4", "N1", "t5"), ("mult", "t5", "t5", "t6"),
         ("mult", "t6", "2", "beta1"), ("mult", "N2", "2", "t7"), ("add", "t7", "N1", "t8"), ("mult", "t5", "t8", "beta2"),
         ("mult", "t8", "t8", "t9"), ("mult", "t9", "2", "beta3")]


def chi_netlist(k):
    """k independent copies of tests/netlists/chi_squared_arith.v in one module (wire names suffixed _c)."""
    nm = lambda w, c: w if w.isdigit() else "%%s_%%d" %% (w, c)
    ins = ", ".join(nm(w, c) for c in range(k) for w in ("N0", "N1", "N2"))
    outs = ", ".join(nm(w, c) for c in range(k) for w in ("alpha", "beta1", "beta2", "beta3"))
    lines = ["module chi_squared(%%s, %%s);" %% (ins, outs), "  input [31:0] %%s;" %% ins, "  output [31:0] %%s;" %% outs]
    for c in range(k):
        for g, (op, a, b, o) in enumerate(GATES):
            lines.append("  %%s g%%d_%%d(%%s, %%s, %%s);" %% (op, g, c, nm(a, c), nm(b, c), nm(o, c)))
    return "\n".join(lines + ["endmodule", ""])


def timed(fn):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": round(min(ts), 3), "median_ms": round(statistics.median(ts), 3), "max_ms": round(max(ts), 3)}


def chi(k, name):
    with tempfile.NamedTemporaryFile("w", suffix=".v", delete=False) as f:
        f.write(chi_netlist(k))
    try:
        gs, ws, ins, outs, d, _, _ = verilog_parser.read_verilog_file(f.name, True)
    finally:
        os.unlink(f.name)
    c = Circuit(gs, ins, outs, d)
    c.sort_circuit()
    c.compute_levels()
    inputs = {}
    for q in range(k):
        inputs.update({"N0_%%d" %% q: PtxtType.U32(2), "N1_%%d" %% q: PtxtType.U32(7), "N2_%%d" %% q: PtxtType.U32(9)})
    rec = {"run": name, "set": "shortint_m2c2", "copies": k, "round_capacity": int(cap), "repeats": repeats}
    cycle = [0]
    for on in (False, True):
        ac = ArithCircuit(ck, sk, c, many_lut=on)
        enc = ac.encrypt_inputs(ws, inputs)

        def one():
            cycle[0] += 1
            one.out = ac.evaluate_encrypted(enc, cycle[0], "u32")   # returns after the final synchronisation
        key = "on" if on else "off"
        rec[key] = timed(one)
        rec[key]["rotations"] = ac.pbs_per_cycle()
        rec[key]["launches"] = ac.pbs_rounds_per_cycle()
        dec = {n: int(v.value) for n, v in ac.decrypt_outputs(one.out, True).items()}
        rec[key]["decrypt_ok"] = all(dec["%%s_%%d" %% (n, q)] == v for q in range(k)
                                     for n, v in (("alpha", 529), ("beta1", 242), ("beta2", 275), ("beta3", 1250)))
    rec["ratio_on_over_off"] = round(rec["on"]["median_ms"] / rec["off"]["median_ms"], 4)
    print("RESULT " + json.dumps(rec), flush=True)


def lut_level(pairs):
    rng = np.random.default_rng(1)
    bits = rng.integers(0, 2, size=3 * pairs).astype(np.uint64)
    w = sk.wires(5 * pairs)
    w.upload(np.arange(3 * pairs), ck.encrypt(bits))
    in_idx = np.repeat(np.arange(3 * pairs, dtype=np.int32).reshape(pairs, 3), 2, axis=0)
    arity = np.full(2 * pairs, 3, dtype=np.int32)
    table = np.tile(np.array([0x96, 0xE8], dtype=np.uint64), pairs)
    out = np.arange(3 * pairs, 5 * pairs, dtype=np.int32)
    rec = {"run": "c_lut_level_full_adder_pairs", "set": "shortint_m2c2", "pairs": pairs, "round_capacity": int(cap),
           "repeats": repeats}
    sk.timing_enable(True)
    for on in (False, True):
        sk.set_level_many_lut(on)

        def one():
            w.eval_lut_level(arity, in_idx, table, out)
            sk.sync()
        key = "on" if on else "off"
        rec[key] = timed(one)
        sk.timing(reset=True)
        one()
        rec[key]["rotations"] = int(sk.timing().pbs_count)
        got = ck.decrypt(w.download(out)).reshape(pairs, 2)
        b = bits.reshape(pairs, 3).astype(np.int64)
        rec[key]["decrypt_ok"] = bool(np.array_equal(got[:, 0], b.sum(axis=1) %% 2) and np.array_equal(got[:, 1], b.sum(axis=1) // 2))
    sk.set_level_many_lut(False)
    rec["ratio_on_over_off"] = round(rec["on"]["median_ms"] / rec["off"]["median_ms"], 4)
    print("RESULT " + json.dumps(rec), flush=True)


chi(1, "a_chi_squared_u32")
chi(copies, "b_chi_squared_u32_concurrent_copies")
lut_level(1024)
sk.close()
'''


def operators(args):
    out = args.out or os.path.join(ROOT, "profiles", "r15", "bench_many_lut_operators.jsonl")
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, "-c", OPERATORS_CHILD % (ROOT, args.repeats, args.copies)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    lines = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as fh:
        for ln in lines:
            fh.write(ln + "\n")
            print(ln)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        return p.returncode
    return 0 if all(json.loads(ln)[k]["decrypt_ok"] for ln in lines for k in ("off", "on")) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--operators", action="store_true", help="the operators with set_many_lut off / on (module docstring)")
    ap.add_argument("--copies", type=int, default=4, help="--operators, run (b): independent chi-squared circuits in one netlist")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=300)
    args = ap.parse_args()
    if args.operators:
        return operators(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "r14", "bench_many_lut.jsonl")
    # one fresh process, under its own time limit (timeout -k: a hung GPU step is ended, nothing is started after it)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, "-c", CHILD % (ROOT, args.repeats)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        return p.returncode
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]
    rec = json.loads(line)
    tm = rec["timings"]
    rec["ratio_c_over_a"] = round(tm["c_many_n_out_2"]["median_ms"] / tm["a_apply_luts"]["median_ms"], 4)
    rec["ratio_d_over_a"] = round(tm["d_many_n_out_4"]["median_ms"] / tm["a_apply_luts"]["median_ms"], 4)
    rec["ratio_c_over_b"] = round(tm["c_many_n_out_2"]["median_ms"] / tm["b_two_apply_luts"]["median_ms"], 4)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))
    return 0 if rec["decrypt_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
