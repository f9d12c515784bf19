"""Audit of whole evaluations that use the many-LUT bootstrap: tests/test_gpu_audit.py's Auditor (kinds 0 and 1: look-up batches
and linear steps against the CPU oracle) plus kind 2 records (helm_si_apply_many_luts) against tests/many_lut.py:

  mask words  of every written output of a checked row: many_lut.masks_from_output0 of the oracle's bootstrap of the same row
  bodies      output 0: the oracle's own; output x > 0: B[h] of the exact accumulator (many_lut.accumulator_exact) when
              `exact`, else the phase of the written row lies within delta / 2 of the table's value for the decrypted input
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import many_lut as ML  # noqa: E402
import saturation as S  # noqa: E402
from test_gpu_audit import Auditor  # noqa: E402


class ManyLutAuditor(Auditor):
    def __init__(self, ck, orc, every=1, batch_every=1, exact=True):
        super().__init__(ck, orc, every, batch_every)
        self.exact = exact
        self.many_batches = self.many_rows = self.many_outputs = 0
        self.kinds = set()

    def __call__(self, rec):
        self.kinds.add(rec["kind"])
        if rec["kind"] != "many_luts":
            return super().__call__(rec)
        with self.lock:
            self.batches += 1
            self.lut_batches += 1
            self.many_batches += 1
            n, nb = self.batches, self.lut_batches
            cnt = len(rec["lut_idx"])
            self.luts_seen += cnt
        if self.batch_every > 1 and nb > 3 and nb % self.batch_every:
            return True
        p = self.ck.params
        k, N, t = p.k, p.N, self.ck.t
        n_out, box, delta = rec["n_out"], N // t, self.ck.delta
        rows = np.arange(cnt) if self.every == 1 else np.unique(np.concatenate([[0, cnt - 1], np.arange(n % self.every, cnt, self.every)]))
        out0 = self.orc.apply_luts(rec["in_rows"][rows], rec["luts"], rec["lut_idx"][rows])
        vals = self.ck.decrypt_message_and_carry(rec["in_rows"][rows])
        bad, outputs = [], 0
        for q, g in enumerate(rows):
            tv = rec["luts"][rec["lut_idx"][g]]
            acc = None
            for x in range(n_out):
                got = rec["out_rows"][g, x]
                if not got.any():          # a skipped output
                    continue
                outputs += 1
                h = ML.output_coefficient(x, n_out, N)
                ok = np.array_equal(got[:k * N], ML.masks_from_output0(out0[q], k, N, h))
                if x == 0:
                    ok = ok and got[k * N] == out0[q][k * N]
                elif self.exact:
                    if acc is None:
                        acc = ML.accumulator_exact(self.orc.keyswitch(rec["in_rows"][g]), tv, self.ck.bsk, S.shape_of(p),
                                                   max(1, p.grouping_factor))
                    ok = ok and int(got[k * N]) == acc[k][h]
                else:
                    j = h + int(vals[q]) * box   # the centre of the input's box, h coefficients on (j < N: the bound holds)
                    err = (int(self.ck.phase(got[None, :])[0]) - int(tv[j])) % ML.MOD
                    ok = ok and j < N and min(err, ML.MOD - err) < delta // 2
                if not ok:
                    bad.append(("many_luts", n, int(g), x))
        with self.lock:
            self.luts_checked += len(rows)
            self.many_rows += len(rows)
            self.many_outputs += outputs
            self.bad += bad
        return True
