#!/usr/bin/env python3
"""What the 64-bit engine's generic blind-rotate kernel (k_pbs64_generic) costs.  (1) Same box, same process, launches
alternating: one full round (round_capacity() bootstraps of the generic context) of shortint_m2c2, shortint_m1c1 and
shortint_m2c1 on their tuned kernels against the generic kernel forced onto the same key (SiServerKey(generic="force")),
with a digest of the rows of each.  (2) One full round of three full-size shapes no tuned build covers (n = 742, the noise of
shortint_m2c2).  (3) The multi-bit form: one full round of shortint_m2c2_multibit3 on the tuned multi-bit kernel against the
generic kernel forced onto the same key (generic="force+multibit"), and one full round of an untuned multi-bit shape at
n = 888 (k = 3, N = 512, g = 2, the noise of shortint_m2c2_multibit3).  Timed: the bootstrap launch alone (helm_si_timing
pbs_ms, HIP events), after one warm-up launch.
usage: bench_generic64.py [--repeats R] [--only classical|multibit]
   -> one JSON line per setting: min / median / max ms per round, bootstraps/s"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import helm_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--only", choices=("classical", "multibit"), default=None, help="(1) and (2), or (3) alone; default: all")
args = ap.parse_args()


def timed(sk, small, luts, idx):
    sk.timing(reset=True)
    out = sk.pbs_batch(small, luts, idx)
    return sk.timing(reset=True).pbs_ms, out


def run(label, ck, keys, rows):
    p = ck.params
    rng = np.random.default_rng(0)
    small = rng.integers(0, 2**64, size=(rows, p.n + 1), dtype=np.uint64)
    luts = np.stack([keys[0][1].make_lut(lambda x: (3 * x + 1) % ck.t), keys[0][1].make_lut(lambda x: x // 2)])
    idx = (np.arange(rows) % 2).astype(np.int32)
    times = {name: [] for name, _ in keys}
    digests = {}
    for _, sk in keys:
        sk.timing_enable(True)
        timed(sk, small, luts, idx)  # warm-up: module load, first touch of the key
    for _ in range(args.repeats):
        for name, sk in keys:  # alternating
            ms, out = timed(sk, small, luts, idx)
            times[name].append(ms)
            digests[name] = hashlib.sha256(out.tobytes()).hexdigest()[:16]
    lines = []
    for name, sk in keys:
        t = sorted(times[name])
        med = t[len(t) // 2]
        lines.append({"what": label, "setting": name, "shape": [p.n, p.k, p.N, p.pbs_l, p.pbs_logB], "rows": rows,
                      "grouping_factor": p.grouping_factor,
                      "kernel_class": sk.kernel_class(), "round_capacity": sk.round_capacity(), "field_bits": sk.field_bits(),
                      "min_ms": round(t[0], 3), "median_ms": round(med, 3), "max_ms": round(t[-1], 3),
                      "spread_pct": round(100 * (t[-1] - t[0]) / med, 1), "bootstraps_per_s": round(rows / (med * 1e-3)),
                      "digest": digests[name]})
    for line in lines:
        print(json.dumps(line), flush=True)
    return lines


SETS = [] if args.only == "multibit" else [("shortint_m2c2", "force"), ("shortint_m1c1", "force"), ("shortint_m2c1", "force")]
if args.only != "classical":
    SETS.append(("shortint_m2c2_multibit3", "force+multibit"))
for name, mode in SETS:
    ck = helm_amd.SiClientKey.generate(name, seed=1)
    tuned = helm_amd.SiServerKey(ck)
    forced = helm_amd.SiServerKey(ck, generic=mode)
    rows = forced.round_capacity()
    ab = run(f"{name}, one full round of the generic kernel: tuned vs forced generic", ck,
             [("tuned", tuned), ("forced generic", forced)], rows)
    print(json.dumps({"what": f"{name}: ratio generic / tuned (median)", "ratio": round(ab[1]["median_ms"] / ab[0]["median_ms"], 2),
                      "tuned_round_capacity": tuned.round_capacity(), "digests_equal": ab[0]["digest"] == ab[1]["digest"]}),
          flush=True)
    forced.close()
    tuned.close()

base, a, b = helm_amd.si_named_params("shortint_m2c2")
for k, N, l, logB in () if args.only == "multibit" else ((4, 512, 1, 22), (3, 1024, 1, 21), (1, 2048, 3, 8)):
    q = helm_amd.SiParams.from_buffer_copy(base)
    q.k, q.N, q.pbs_l, q.pbs_logB = k, N, l, logB
    ck = helm_amd.SiClientKey(q, a, b, seed=1)
    sk = helm_amd.SiServerKey(ck, generic="allow")
    run("untuned shape, n = 742, one full round", ck, [(f"k={k} N={N} l={l} logB={logB}", sk)], sk.round_capacity())
    sk.close()

if args.only != "classical":
    base, a, b = helm_amd.si_named_params("shortint_m2c2_multibit3")
    k, N, l, logB, g = 3, 512, 1, 18, 2
    q = helm_amd.SiParams.from_buffer_copy(base)
    q.k, q.N, q.pbs_l, q.pbs_logB, q.grouping_factor = k, N, l, logB, g
    ck = helm_amd.SiClientKey(q, a, b, seed=1)
    sk = helm_amd.SiServerKey(ck, generic="allow+multibit")
    run("untuned multi-bit shape, n = 888, one full round", ck, [(f"k={k} N={N} l={l} logB={logB} g={g}", sk)], sk.round_capacity())
    sk.close()
