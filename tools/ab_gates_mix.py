"""One side of a same-box A/B of the gate front ends: 4,096 AND gates plus a quarter as many MUX gates in one launch.

    HELM_HIP_LIB=<a build of libhelm_hip.so> python tools/ab_gates_mix.py --label parent|branch
        [--set boolean_default | boolean_default_ks_pbs] [--out profiles/rNN/ab_gates_mix.jsonl]

Run it from alternating fresh processes (one per side and repeat).  A keyswitch-first set (pbs_order = 1) with
HELM_HIP_KS_MFMA=0 in the environment takes the level through k_keyswitch_gate, the vector-ALU keyswitch that forms the
gates' linear combinations as it reads the wire rows; without it through k_ks_gate_digits.  Wall time of one launch (mean of
`--reps` back-to-back launches after a warm-up), the engine's own bootstrap and keyswitch times, a decrypt check.  The
record carries the label, never a path."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import helm_amd  # noqa: E402

AND, MUX = 0, 3


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--label", required=True)
    ap.add_argument("--set", default="boolean_default")
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, Q = a.B, a.B // 4
    ck = helm_amd.ClientKey.generate(a.set, seed=1)
    sk = helm_amd.ServerKey(ck)
    bits = np.random.default_rng(0).integers(0, 2, size=3 * B).astype(bool)
    w = sk.wires(4 * B + Q)
    w.upload(np.arange(3 * B), ck.encrypt(bits))
    ar = np.arange(B + Q, dtype=np.int32)
    ops = np.where(ar < B, AND, MUX).astype(np.int32)
    i0, i1 = ar % B, B + ar % B
    i2 = np.where(ar < B, -1, 2 * B + ar % B).astype(np.int32)
    out = (3 * B + ar).astype(np.int32)
    prog = helm_amd.Program(sk, ops, i0.astype(np.int32), i1.astype(np.int32), i2, out, [0, B + Q])
    sk.timing_enable(True)
    prog.run(w)
    sk.sync()
    sk.timing(reset=True)
    t0 = time.perf_counter()
    for _ in range(a.reps):
        prog.run(w)
    sk.sync()
    dt = (time.perf_counter() - t0) / a.reps
    t = sk.timing(reset=True)
    a_, b_, c_ = bits[:B], bits[B:2 * B], bits[2 * B:]
    want = np.concatenate([a_ & b_, np.where(c_[:Q], a_[:Q], b_[:Q])])
    rec = {"label": a.label, "set": a.set, "ks_mfma": os.environ.get("HELM_HIP_KS_MFMA"), "and_gates": B, "mux_gates": Q,
           "wall_ms": round(dt * 1e3, 4), "pbs_ms": round(t.pbs_ms / a.reps, 4), "ks_ms": round(t.ks_ms / a.reps, 4),
           "decrypt_ok": bool(np.array_equal(ck.decrypt(w.download(out)), want))}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    prog.destroy()
    sk.close()


if __name__ == "__main__":
    main()
