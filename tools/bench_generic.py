#!/usr/bin/env python3
"""What the generic blind-rotate kernel (k_pbs_generic) costs.  (1) Same box, same process, launches alternating: one full
round of boolean_default (1,024 bootstraps) under the default dispatch (the lockstep k_pbs) against HELM_HIP_PBS_VARIANT=10
(the generic kernel on the same shape), with a digest of the rows of each.  (2) Bootstraps per second of the generic kernel at
two full-size shapes no tuned build covers.  Timed: the blind-rotate launch alone (helm_hip_timing pbs_ms, HIP events).
usage: bench_generic.py [--rounds R]   -> one JSON line per setting: best and median ms per launch, bootstraps/s, digest"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import helm_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()


def context(params, lwe_std, glwe_std, variant=None):
    ck = helm_amd.ClientKey(params, lwe_std, glwe_std, seed=1)
    if variant is not None:
        os.environ["HELM_HIP_PBS_VARIANT"] = str(variant)
    try:
        sk = helm_amd.ServerKey(ck)  # the variant is read when the context is created
    finally:
        os.environ.pop("HELM_HIP_PBS_VARIANT", None)
    sk.timing_enable(True)
    return ck, sk


def timed(sk, lwe, tv):
    sk.timing(reset=True)
    out = sk.pbs_batch(lwe, tv[None, :])
    return sk.timing(reset=True).pbs_ms, out


def run(label, cases, count):
    lines = []
    rng = np.random.default_rng(0)
    prep = []
    for name, (ck, sk) in cases:
        lwe = ck.encrypt(rng.integers(0, 2, size=count).astype(bool)) if not prep else prep[0][2]
        prep.append((name, sk, lwe, ck))
    tv = np.full(prep[0][3].params.N, 0x20000000, dtype=np.uint32)
    times = {name: [] for name, *_ in prep}
    digests = {}
    for name, sk, lwe, _ in prep:  # warm-up launch (module load, first-touch of the key)
        timed(sk, lwe, tv)
    for _ in range(args.rounds):
        for name, sk, lwe, _ in prep:
            ms, out = timed(sk, lwe, tv)
            times[name].append(ms)
            digests[name] = hashlib.sha256(out.tobytes()).hexdigest()[:16]
    for name, sk, _, ck in prep:
        t = sorted(times[name])
        p = ck.params
        lines.append({"what": label, "setting": name, "shape": [p.n, p.k, p.N, p.pbs_l, p.pbs_logB], "count": count,
                      "kernel_class": sk.kernel_class(), "launch_quantum": sk.launch_quantum(),
                      "launch_costs": sk.launch_costs(), "field_bits": sk.field_bits(), "best_ms": round(t[0], 3),
                      "median_ms": round(t[len(t) // 2], 3), "bootstraps_per_s": round(count / (t[len(t) // 2] * 1e-3)),
                      "digest": digests[name]})
    for line in lines:
        print(json.dumps(line), flush=True)
    return lines


p, a, b = helm_amd.named_params("boolean_default")
ab = run("boolean_default, one full round: default dispatch vs the generic kernel",
         [("default", context(p, a, b)), ("variant 10 (k_pbs_generic)", context(p, a, b, 10))], 1024)
print(json.dumps({"what": "ratio generic / tuned (median)", "ratio": round(ab[1]["median_ms"] / ab[0]["median_ms"], 2),
                  "digests_equal": ab[0]["digest"] == ab[1]["digest"]}), flush=True)
for k, N, l, logB in ((2, 1024, 2, 6), (1, 2048, 3, 5)):
    q = helm_amd.named_params("boolean_default")[0]
    q.k, q.N, q.pbs_l, q.pbs_logB = k, N, l, logB
    ck, sk = context(q, a, b)
    run("generic shape, n = 722", [(f"k={k} N={N} l={l} logB={logB}", (ck, sk))], 1024)
    sk.close()
