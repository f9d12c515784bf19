"""Reference of a keyswitch-first level (pbs_order = 1), composed of the oracle's existing parts - no new oracle code.

Wires are big LWE rows of k N + 1 words under the GLWE key.  A bootstrapped gate is
    lin   = oracle.lincomb(k N, op, which, in0, in1, in2)      the gate formulas of order 0 over k N + 1 words, +-1/8 on the body
    small = Oracle.keyswitch(lin)
    big   = Oracle.bootstrap_noks(small, tv = all +1/8)        the sample extract is the gate's row
and a MUX is big(which = 0) + big(which = 1) with PT_TRUE added to the body (what tfhe's boolean engine does under the big
encryption key, as recalled - DESIGN.md 4.3).  NOT, BUF, DFF and the constants are orc_gate_linear_only at dimension k N.
"""
import ctypes as C

import numpy as np

import oracle

PT_TRUE, PT_FALSE = 0x20000000, 0xE0000000
BOOTSTRAPPED = (oracle.AND, oracle.NAND, oracle.OR, oracle.NOR, oracle.XOR, oracle.XNOR, oracle.MUX)
LINEAR = (oracle.NOT, oracle.BUF, oracle.DFF, oracle.CONST_ONE, oracle.CONST_ZERO)
KS_PBS = 16  # HELM_HIP_CREATE_KS_PBS


def linear_only(dim, op, in0):
    L = oracle.lib()
    u32p = C.POINTER(C.c_uint32)
    L.orc_gate_linear_only.argtypes = [C.c_int, C.c_int, u32p, u32p]
    out = np.zeros(dim + 1, dtype=np.uint32)
    L.orc_gate_linear_only(int(dim), int(op), oracle._u32(in0), oracle._u32(out))
    return out


class KsFirst:
    """orc: an oracle.Oracle over the key's (bsk, ksk) - any of its routes.  fp=True takes the bootstraps through the
    oracle's fp64 route (full-size sets)."""

    def __init__(self, orc, fp=False):
        self.orc, self.fp = orc, fp
        self.p = orc.p
        self.kN = orc.p.k * orc.p.N
        self.tv = np.full(orc.p.N, PT_TRUE, dtype=np.uint32)

    def lin(self, op, which, in0, in1, in2=None):
        return oracle.lincomb(self.kN, op, which, in0, in1, in2)

    def small(self, op, which, in0, in1, in2=None):
        """The keyswitch stage of one bootstrap: n + 1 words."""
        return self.orc.keyswitch(self.lin(op, which, in0, in1, in2))

    def half(self, op, which, in0, in1, in2=None):
        s = self.small(op, which, in0, in1, in2)
        if self.fp:
            return self.orc.bootstrap_noks_fp(s[None, :], self.tv)[0]
        return self.orc.bootstrap_noks(s, self.tv)

    def gate(self, op, in0=None, in1=None, in2=None):
        if op in LINEAR:
            return linear_only(self.kN, op, in0)
        assert op in BOOTSTRAPPED
        if op != oracle.MUX:
            return self.half(op, 0, in0, in1)
        out = self.half(op, 0, in0, in1, in2) + self.half(op, 1, in0, in1, in2)
        out[self.kN] = np.uint32((int(out[self.kN]) + PT_TRUE) & 0xFFFFFFFF)
        return out

    def eval_level(self, wires, opcode, in0, in1, in2, outw):
        """In place on `wires` ([n_wires, k N + 1] uint32): every gate reads the table as it was before the level."""
        assert wires.dtype == np.uint32 and wires.shape[1] == self.kN + 1
        src = wires.copy()
        row = lambda i: np.ascontiguousarray(src[i]) if i >= 0 else None  # noqa: E731
        for g in range(len(opcode)):
            wires[outw[g]] = self.gate(int(opcode[g]), row(int(in0[g])), row(int(in1[g])), row(int(in2[g])))

    def run_program(self, wires, opcode, in0, in1, in2, outw, level_offsets):
        for l in range(len(level_offsets) - 1):
            a, b = int(level_offsets[l]), int(level_offsets[l + 1])
            self.eval_level(wires, opcode[a:b], in0[a:b], in1[a:b], in2[a:b], outw[a:b])


def plain_gate(op, a=False, b=False, c=False):
    """The plaintext truth of a gate; MUX is sel = in2 ? in0 : in1."""
    return {oracle.AND: a and b, oracle.NAND: not (a and b), oracle.OR: a or b, oracle.NOR: not (a or b),
            oracle.XOR: a != b, oracle.XNOR: a == b, oracle.MUX: a if c else b, oracle.NOT: not a, oracle.BUF: a,
            oracle.DFF: a, oracle.CONST_ONE: True, oracle.CONST_ZERO: False}[op]
