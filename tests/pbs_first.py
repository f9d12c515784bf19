"""Reference of the bootstrap-first order of the 64-bit engine (HELM_SI_CREATE_PBS_KS, helm_si_pbs_order = 0), composed of
what oracle.Oracle64 already exposes - no new oracle code.

Wires are small LWE rows of n + 1 words under the LWE key.  A look-up is
    big   = Oracle64.bootstrap(row, lut)          the sample extract at coefficient 0, k N + 1 words
    small = Oracle64.keyswitch(big)               the wire row
a LUT level is the packing linear combination on n + 1-word rows in Python integers mod 2^64, followed by that, and the
outputs of a many-LUT look-up are the keyswitch of each extract of tests/many_lut.py (as it stands).  Every call reads all
of its inputs before it writes any output, as the engine does.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import many_lut as ML  # noqa: E402
import saturation as S  # noqa: E402

MOD = 1 << 64


class PbsFirst:
    """orc: an oracle.Oracle64 over the key's (bsk, ksk)."""

    def __init__(self, orc):
        self.orc = orc
        self.p = orc.p
        self.n, self.k, self.N, self.t = orc.p.n, orc.p.k, orc.p.N, orc.t
        self.delta = orc.delta

    # ---- one look-up ------------------------------------------------------------------------------------------------
    def apply_lut_small(self, row, lut):
        return self.orc.keyswitch(self.orc.bootstrap(np.ascontiguousarray(row, dtype=np.uint64), lut))

    def apply_luts(self, wires, in_idx, luts, out_idx, lut_idx=None):
        """In place on `wires` ([rows, n + 1] uint64), as SiWires.apply_luts: every input is read first."""
        assert wires.dtype == np.uint64 and wires.shape[1] == self.n + 1
        luts = np.atleast_2d(luts)
        lut_idx = np.zeros(len(in_idx), dtype=np.int32) if lut_idx is None else lut_idx
        outs = [self.apply_lut_small(wires[int(in_idx[g])], luts[int(lut_idx[g])]) for g in range(len(in_idx))]
        for g, o in enumerate(outs):
            wires[int(out_idx[g])] = o

    # ---- linear steps -----------------------------------------------------------------------------------------------
    def lincomb_row(self, wires, in_idx, coef, const_add=0):
        acc = [0] * (self.n + 1)
        for r, c in zip(in_idx, coef):
            if int(r) < 0:
                continue
            row = wires[int(r)]
            for i in range(self.n + 1):
                acc[i] = (acc[i] + int(c) * int(row[i])) % MOD
        acc[self.n] = (acc[self.n] + int(const_add) * self.delta) % MOD
        return np.array(acc, dtype=np.uint64)

    def lincomb(self, wires, in_idx, coef, out_idx, const_add=None):
        outs = [self.lincomb_row(wires, in_idx[g], coef[g], 0 if const_add is None else const_add[g])
                for g in range(len(out_idx))]
        for g, o in enumerate(outs):
            wires[int(out_idx[g])] = o

    # ---- a LUT level (helm_si_eval_lut_level) ---------------------------------------------------------------------
    def level_lut(self, arity, table):
        t = self.t
        if arity == 2:
            f = [(int(table) >> (((v >> 1) & 1) * 2 + (v & 1))) & 1 for v in range(t)]
        else:
            f = [(int(table) >> (v & ((1 << arity) - 1))) & 1 for v in range(t)]
        return self.orc.make_lut(f)

    def eval_lut_level(self, wires, arity, in_idx, table, out_idx):
        """In place on `wires`: bootstrapped gates first (pack, then the look-up on the packed row), copies and negations
        after them - the engine's order, which matters for a flip-flop that latches a wire of its own level."""
        in_idx = np.atleast_2d(np.asarray(in_idx))
        boot = [g for g in range(len(arity)) if arity[g] >= 2]
        rest = [g for g in range(len(arity)) if arity[g] < 2]
        packed = [self.lincomb_row(wires, in_idx[g][:arity[g]], [1 << (arity[g] - 1 - q) for q in range(arity[g])])
                  for g in boot]
        outs = [self.apply_lut_small(packed[i], self.level_lut(arity[g], table[g])) for i, g in enumerate(boot)]
        for i, g in enumerate(boot):
            wires[int(out_idx[g])] = outs[i]
        lin = [self.lincomb_row(wires, in_idx[g][:1], [1 if (arity[g] == 0 or int(table[g]) == 0) else -1]) for g in rest]
        for i, g in enumerate(rest):
            wires[int(out_idx[g])] = lin[i]

    # ---- many-LUT ---------------------------------------------------------------------------------------------------
    def many_lut_outputs(self, row, tv, n_out, bsk, group=1):
        """The n_out wire rows of ONE blind rotation of `row` with the many-LUT polynomial tv: the keyswitch of the extract at
        x N / M of the exact accumulator (many_lut.accumulator_exact: up to a second per row)."""
        acc = ML.accumulator_exact(row, tv, bsk, S.shape_of(self.p), group)
        return [self.orc.keyswitch(ML.extract_at(acc, ML.output_coefficient(x, n_out, self.N))) for x in range(n_out)]

    # ---- client side -------------------------------------------------------------------------------------------------
    def phase(self, lwe_sk_bits, row):
        v = int(row[self.n])
        for i in range(self.n):
            if int(lwe_sk_bits[i]):
                v -= int(row[i])
        return v % MOD

    def decrypt(self, lwe_sk_bits, row):
        """message and carry"""
        return ((self.phase(lwe_sk_bits, row) + self.delta // 2) // self.delta) % self.t
