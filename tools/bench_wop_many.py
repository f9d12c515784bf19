"""Wide LUT gates on shared inputs: 256 outputs of 8 one-bit inputs under wopbs_m1c1, two ways, one process, the cases
alternated, both shapes warmed, REPEATS repeats, median [min - max] of the wall time of the C call (synchronised), the stage
breakdown of helm_wop_get_timing, every output decrypted and checked.

  a  256 single gates through helm_wop_eval_luts (32 input tuples, each read by 8 gates): the route without sharing
  b  32 groups x 8 through helm_wop_eval_many_luts: the front stages once per group

Usage: python tools/bench_wop_many.py [out.jsonl]
       python tools/bench_wop_many.py --ab PARENT_TREE [out.jsonl]   single gates, this tree against a built checkout of the
                                                                     parent commit, child processes alternated
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("HELM_BENCH_TREE", ROOT))     # --ab: the child imports the package of the tree it measures
REPEATS, GROUPS, M, N_OUT = 7, 32, 8, 8


def setup():
    import numpy as np
    import helm_amd
    from helm_amd import wopbs
    from helm_amd.shortint import si_named_params
    sp, sa, sb = si_named_params("shortint_m2c2")
    wp, wa, wb = wopbs.wop_named_params("wopbs_m1c1")
    sp.message_modulus, sp.carry_modulus = wp.message_modulus, wp.carry_modulus
    ck = helm_amd.SiClientKey(sp, sa, sb, seed=1)
    wk = wopbs.WopClientKey(ck, wp, wa, wb, seed=2)
    sk = helm_amd.SiServerKey(ck)
    wsk = wopbs.WopServerKey(sk, wk)
    rng = np.random.default_rng(0)
    xs = rng.permutation(256)[:GROUPS]
    bits_in = np.array([[(int(x) >> (M - 1 - q)) & 1 for q in range(M)] for x in xs], dtype=np.uint64)
    truth = rng.integers(0, 2, size=(N_OUT, 256), dtype=np.uint64)      # distinct tables; basis 2: index = the byte
    tables = np.stack([wopbs.make_table(wp, M, 1, t) for t in truth])   # [N_OUT][N]
    w = sk.wires(GROUPS * (M + N_OUT))
    w.upload(np.arange(GROUPS * M), ck.encrypt(bits_in.reshape(-1)))
    in_idx = np.arange(GROUPS * M, dtype=np.int32).reshape(GROUPS, M)
    out_idx = np.arange(GROUPS * M, GROUPS * (M + N_OUT), dtype=np.int32).reshape(GROUPS, N_OUT)
    return np, ck, sk, wsk, w, xs, truth, tables, in_idx, out_idx


def single_case(np, wsk, w, tables, in_idx, out_idx):
    from helm_amd import _native as nv
    ii = np.ascontiguousarray(np.repeat(in_idx, N_OUT, axis=0))
    tt = np.ascontiguousarray(np.tile(tables, (GROUPS, 1)))
    oo = np.ascontiguousarray(out_idx.reshape(-1))
    return lambda: nv.hip_check(nv.hip.helm_wop_eval_luts(wsk._h, w._h, nv.as_i32p(ii), M, 1, nv.as_u64p(tt), nv.as_i32p(oo),
                                                          GROUPS * N_OUT))


def groups_case(np, wsk, w, tables, in_idx, out_idx):
    from helm_amd import _native as nv
    tt = np.ascontiguousarray(np.broadcast_to(tables, (GROUPS,) + tables.shape))
    oo = np.ascontiguousarray(out_idx)
    return lambda: nv.hip_check(nv.hip.helm_wop_eval_many_luts(wsk._h, w._h, nv.as_i32p(in_idx), M, 1, nv.as_u64p(tt),
                                                               nv.as_i32p(oo), N_OUT, GROUPS))


def timed(ck, sk, wsk, w, xs, truth, out_idx, run):
    wsk.timing(reset=True)
    t0 = time.perf_counter()
    run()
    sk.sync()
    dt = (time.perf_counter() - t0) * 1e3
    t = wsk.timing(reset=True)
    got = ck.decrypt_message_and_carry(w.download(out_idx.reshape(-1))).reshape(GROUPS, N_OUT)
    ok = all(int(got[g, o]) == int(truth[o, xs[g]]) for g in range(GROUPS) for o in range(N_OUT))
    return dt, t, ok


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def run_child(flag, env):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), flag], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])


def main(out_path):
    np, ck, sk, wsk, w, xs, truth, tables, in_idx, out_idx = setup()
    cases = {"a_single_256": single_case(np, wsk, w, tables, in_idx, out_idx),
             "b_groups_32x8": groups_case(np, wsk, w, tables, in_idx, out_idx)}
    forms = {"a_single_256": 0, "b_groups_32x8": wsk.many_form(M, N_OUT)}
    for name, run in cases.items():                 # warm both shapes
        assert timed(ck, sk, wsk, w, xs, truth, out_idx, run)[2], name
    wall = {k: [] for k in cases}
    stages = {k: [] for k in cases}
    for _ in range(REPEATS):
        for name, run in cases.items():             # alternated
            dt, t, ok = timed(ck, sk, wsk, w, xs, truth, out_idx, run)
            assert ok, name
            wall[name].append(dt)
            stages[name].append(t)
    recs = []
    for name in cases:
        med = {f: round(statistics.median(s[f] for s in stages[name]), 3) for f in stages[name][0]}
        recs.append({"case": name, "set": "wopbs_m1c1 beside shortint_m2c2 (moduli 2 x 2)", "inputs": M, "bits_per_block": 1,
                     "outputs": GROUPS * N_OUT, "form": forms[name], "repeats": REPEATS, "wall_ms": spread(wall[name]),
                     "stages_median": med, "decrypt_ok": True})
    recs.append({"ratios": {"b_over_a": round(statistics.median(wall["b_groups_32x8"]) / statistics.median(wall["a_single_256"]), 4)}})
    with open(out_path, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))
    wsk.close()
    sk.close()


def child_single():
    np, ck, sk, wsk, w, xs, truth, tables, in_idx, out_idx = setup()
    run = single_case(np, wsk, w, tables, in_idx, out_idx)
    v = []
    for rep in range(4):
        dt, t, ok = timed(ck, sk, wsk, w, xs, truth, out_idx, run)
        assert ok
        if rep:
            v.append(dt)
    print("CHILD " + json.dumps(v))


def ab(parent_tree, out_path):
    """the same 256 single gates under this tree and under a built checkout of the parent commit, child processes alternated"""
    wall = {"this": [], "parent": []}
    for _ in range(3):
        for name, tree in (("this", ROOT), ("parent", os.path.abspath(parent_tree))):
            wall[name] += run_child("--child-single", {"HELM_BENCH_TREE": tree})
    rec = {"case": "a_single_256 through helm_wop_eval_luts", "this_build_ms": spread(wall["this"]), "parent_build_ms": spread(wall["parent"]),
           "runs_each": len(wall["this"]), "ratio_of_medians": round(statistics.median(wall["this"]) / statistics.median(wall["parent"]), 4)}
    with open(out_path, "w") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child-single":
        child_single()
    elif len(sys.argv) > 2 and sys.argv[1] == "--ab":
        ab(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else "ab_wop_single_vs_parent.jsonl")
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else "bench_wop_many.jsonl")
