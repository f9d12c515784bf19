#!/usr/bin/env python3
"""What the two-prime blind-rotate kernel (k_pbs_crt) costs.  Same box, same process, launches alternating.
(1) boolean_default's shape and helm_cuda's shape, each on (a) its tuned kernels (default dispatch), (b) the single-prime
generic kernel (HELM_HIP_PBS_VARIANT=10) and (c) k_pbs_crt (ServerKey(crt="force")), with a digest of the rows of each: one
launch of `count` bootstraps, count = the least common multiple of the three contexts' launch quanta (whole rounds on every
kernel).  (2) boolean_tfhe_lib at full size (n = 830, k = 2, N = 1024, one level of 23 bits: crt="allow", kernel class
"crt"), one full round: gate-bootstraps per second.  Before anything is timed, every context evaluates one level of the six
binary gates and two MUXes, and the level must decrypt to the truth table.  Timed: the blind-rotate launch alone
(helm_hip_timing pbs_ms, HIP events), after one warm-up launch.
usage: bench_crt.py [--repeats R]   -> one JSON line per setting: min / median / max ms per launch, bootstraps/s, digest"""
import argparse
import hashlib
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import helm_amd  # noqa: E402
import oracle  # noqa: E402  (opcodes only)

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()


def context(ck, variant=None, crt=None):
    if variant is not None:
        os.environ["HELM_HIP_PBS_VARIANT"] = str(variant)
    try:
        sk = helm_amd.ServerKey(ck, crt=crt)  # the variant is read when the context is created
    finally:
        os.environ.pop("HELM_HIP_PBS_VARIANT", None)
    sk.timing_enable(True)
    return sk


def check_truth_table(ck, sk, label):
    bits = np.array([0, 1, 0, 1, 0, 0, 1, 1, 1, 0], dtype=bool)
    ops = [oracle.AND, oracle.NAND, oracle.OR, oracle.NOR, oracle.XOR, oracle.XNOR, oracle.MUX, oracle.MUX]
    i0, i1, i2 = [0, 2, 4, 6, 0, 2, 4, 5], [1, 3, 5, 7, 3, 5, 6, 7], [-1] * 6 + [8, 9]
    w = sk.wires(18)
    w.upload(np.arange(10), ck.encrypt(bits))
    w.eval_gate_level(ops, i0, i1, i2, np.arange(10, 18, dtype=np.int32))
    got = [bool(x) for x in ck.decrypt(w.download(np.arange(10, 18)))]
    a, b = bits[i0], bits[i1]
    want = [a[0] & b[0], not (a[1] & b[1]), a[2] | b[2], not (a[3] | b[3]), a[4] ^ b[4], not (a[5] ^ b[5]),
            a[6] if bits[8] else b[6], a[7] if bits[9] else b[7]]
    if got != [bool(x) for x in want]:
        sys.exit(f"{label}: the gate level does not decrypt to the truth table: {got}")
    w.free()


def timed(sk, lwe, tv):
    sk.timing(reset=True)
    out = sk.pbs_batch(lwe, tv[None, :])
    return sk.timing(reset=True).pbs_ms, out


def run(label, ck, cases, count):
    p = ck.params
    rng = np.random.default_rng(0)
    lwe = ck.encrypt(rng.integers(0, 2, size=count).astype(bool))
    tv = np.full(p.N, 0x20000000, dtype=np.uint32)
    times = {name: [] for name, _ in cases}
    digests = {}
    for _, sk in cases:  # warm-up launch (module load, first touch of the key)
        timed(sk, lwe, tv)
    for _ in range(args.repeats):
        for name, sk in cases:  # alternating
            ms, out = timed(sk, lwe, tv)
            times[name].append(ms)
            digests[name] = hashlib.sha256(out.tobytes()).hexdigest()[:16]
    lines = []
    for name, sk in cases:
        t = sorted(times[name])
        med = t[len(t) // 2]
        lines.append({"what": label, "setting": name, "shape": [p.n, p.k, p.N, p.pbs_l, p.pbs_logB], "count": count,
                      "kernel_class": sk.kernel_class(), "launch_quantum": sk.launch_quantum(), "field_bits": sk.field_bits(),
                      "min_ms": round(t[0], 3), "median_ms": round(med, 3), "max_ms": round(t[-1], 3),
                      "spread_pct": round(100 * (t[-1] - t[0]) / med, 1), "bootstraps_per_s": round(count / (med * 1e-3)),
                      "digest": digests[name]})
    for line in lines:
        print(json.dumps(line), flush=True)
    return lines


for name in ("boolean_default", "helm_cuda"):
    ck = helm_amd.ClientKey.generate(name, seed=1)
    cases = [("(a) tuned (default dispatch)", context(ck)), ("(b) variant 10 (k_pbs_generic)", context(ck, variant=10)),
             ("(c) crt=force (k_pbs_crt)", context(ck, crt="force"))]
    for label, sk in cases:
        check_truth_table(ck, sk, f"{name} {label}")
    count = 1
    for _, sk in cases:
        count = math.lcm(count, sk.launch_quantum())
    if count > 8192:  # (quanta without a small common multiple: whole rounds of the two-prime kernel)
        count = 4 * cases[2][1].launch_quantum()
    ab = run(f"{name}: whole rounds on every kernel, same rows", ck, cases, count)
    print(json.dumps({"what": f"{name}: ratios of the medians", "crt_over_generic": round(ab[2]["median_ms"] / ab[1]["median_ms"], 2),
                      "crt_over_tuned": round(ab[2]["median_ms"] / ab[0]["median_ms"], 2),
                      "generic_over_tuned": round(ab[1]["median_ms"] / ab[0]["median_ms"], 2),
                      "digests_equal": len({x["digest"] for x in ab}) == 1}), flush=True)
    for _, sk in cases:
        sk.close()

ck = helm_amd.ClientKey.generate("boolean_tfhe_lib", seed=1)
sk = context(ck, crt="allow")
check_truth_table(ck, sk, "boolean_tfhe_lib")
run("boolean_tfhe_lib at full size (recalled parameter set), one full round: gate-bootstraps/s", ck, [("crt=allow (k_pbs_crt)", sk)],
    sk.launch_quantum())
sk.close()
