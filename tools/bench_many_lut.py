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
usage: bench_many_lut.py [--repeats 7] [--out profiles/r14/bench_many_lut.jsonl] [--timeout 300]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "bench_many_lut.jsonl"))
    ap.add_argument("--timeout", type=int, default=300)
    args = ap.parse_args()
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
