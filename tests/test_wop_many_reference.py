"""CPU side of helm_wop_eval_many_luts (several wide-LUT tables on one input tuple): the host's grouping rule, the new symbols
in the libraries and headers, and argument validation that needs no device.  The look-up itself has one form (one vertical
packing per table on the group's GGSWs) whose reference is helm_wop_eval_luts: tests/test_gpu_wop_many.py compares them word
for word on the GPU."""
import ctypes as C
import os
import re

import numpy as np

from helm_amd import _host as H
from helm_amd import _native as nv
from helm_amd import wopbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _groups(in_idx, cap):
    in_idx = np.ascontiguousarray(in_idx, dtype=np.int32)
    out = np.zeros(len(in_idx), dtype=np.int64)
    n = H.host.helm_host_wide_lut_groups(in_idx.ctypes.data_as(C.POINTER(C.c_int32)), len(in_idx), in_idx.shape[1], cap,
                                         out.ctypes.data_as(C.POINTER(C.c_int64)))
    return n, list(out)


def test_grouping_rule():
    a, b, perm = [3, 1, 2], [4, 5, 6], [1, 3, 2]
    n, g = _groups([a, b, a, perm, a, b], 16)
    assert (n, g) == (3, [0, 1, 0, 2, 0, 1])           # equal tuples group, a permutation does not, the order is kept
    n, g = _groups([a] * 5, 2)
    assert (n, g) == (3, [0, 0, 1, 1, 2])              # a full group is closed, the next gate opens another
    n, g = _groups([a, b, a, b, a], 2)
    assert (n, g) == (3, [0, 1, 0, 1, 2])
    n, g = _groups([a, b, perm], 1)
    assert (n, g) == (3, [0, 1, 2])                    # cap 1: no sharing
    assert _groups(np.zeros((0, 3), np.int32), 4)[0] == 0
    assert H.host.helm_host_wide_lut_groups(None, 3, 3, 4, None) == -1
    one = np.zeros(3, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    out = np.zeros(1, np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    assert H.host.helm_host_wide_lut_groups(one, 1, 3, 0, out) == -1 and H.host.helm_host_wide_lut_groups(one, 1, 0, 4, out) == -1
    # the cap a LutCircuit uses: the tables of one pass of the engine's chunk, max(1, 16384 / bits)
    assert [H.host.helm_host_wide_lut_group_cap(b) for b in (0, 1, 8, 12, 17, 16385)] == [0, 16384, 2048, 1365, 963, 1]
    assert all(H.host.helm_host_wide_lut_group_cap(b) == max(1, 16384 // b) for b in range(1, 18))


def test_a_random_level_groups_exactly_the_equal_tuples():
    """against a plain dictionary: with a cap nothing reaches, two gates share a group iff their tuples are equal in order"""
    rng = np.random.default_rng(3)
    pool = rng.integers(0, 6, size=(7, 4)).astype(np.int32)
    in_idx = pool[rng.integers(0, 7, size=60)]
    n, g = _groups(in_idx, 1000)
    first = {}
    want = [first.setdefault(tuple(int(v) for v in row), len(first)) for row in in_idx]
    assert g == want and n == len(first)


def test_new_symbols_are_exported_and_declared():
    for name in ("helm_wop_eval_many_luts", "helm_wop_many_form", "helm_wop_vertical_packing_many_batch"):
        assert hasattr(nv.hip, name) and name in nv.WOP_API, name
    for name in ("helm_host_wide_lut_groups", "helm_host_wide_lut_group_cap", "helm_host_si_circuit_set_wopbs_share"):
        assert hasattr(H.host, name) and name in H.HOST_API, name
    wop_h = open(os.path.join(ROOT, "include", "helm_wopbs.h")).read()
    host_h = open(os.path.join(ROOT, "include", "helm_host.h")).read()
    assert re.search(r"int helm_wop_eval_many_luts\(helm_wop_ctx \*ctx, helm_si_wires \*w, const int32_t \*in_idx", wop_h)
    assert "int helm_wop_many_form(const helm_wop_ctx *ctx, int32_t bits, int32_t n_out);" in wop_h
    assert "int helm_wop_vertical_packing_many_batch(" in wop_h
    assert "int helm_host_si_circuit_set_wopbs_share(helm_si_circuit *c, int on);" in host_h
    assert "helm_host_wide_lut_groups(" in host_h
    for attr in ("eval_many_luts", "vertical_packing_many", "many_form"):
        assert hasattr(wopbs.WopServerKey, attr)
    # argument validation needs no device
    assert nv.hip.helm_wop_many_form(None, 8, 8) == -1
    assert nv.hip.helm_wop_eval_many_luts(None, None, None, 1, 1, None, None, 2, 1) == -1
    assert nv.hip.helm_wop_vertical_packing_many_batch(None, None, 1, None, 2, None, 1) == -1
