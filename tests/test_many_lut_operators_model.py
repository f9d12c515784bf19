"""Where the operators use the many-LUT bootstrap, as plain integers (no GPU, no project code beyond tests/many_lut.py):

  carry propagation, round 1   a block sum is 0..7 < 8 = t / 2 at 2+2 bits, so its message and its weighted carry state are the
                               two functions of one two-function table (RadixEngine::set_many_lut builds one per weight)
  LUT levels                   gates of one arity on one input tuple pack the same index < 2^arity; up to M of them share a
                               rotation, M the largest power of two with 2^arity <= t / M (helm_si_set_level_many_lut)
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import many_lut as ML  # noqa: E402

T, N = 16, 512          # 2+2-bit blocks; the polynomial size only has to hold whole boxes


def lut_msg(v):
    return v & 3


def lut_t(w, v):
    """The weighted carry state of a block sum: 0 absorbs, 1 propagates (sum == 3), 2 generates (sum >= 4), times 2^w."""
    return (2 if v >= 4 else 1 if v == 3 else 0) << w


def read_poly(tv, t, h, v):
    """What a bootstrap with test polynomial tv answers for input v at extract coefficient h: undo the half-box rotation and
    read coefficient h + v * box + box / 2 (the centre of v's box), negacyclically."""
    n = len(tv)
    box = n // t
    j = (h + v * box) % (2 * n)           # tv is acc rotated left by box / 2: its coefficient v * box is acc's box centre
    val = int(tv[j % n])
    return val if j < n else -val % ML.MOD


@pytest.mark.parametrize("w", range(4))
def test_pair_table_is_the_message_and_the_weighted_state(w):
    per = T // 2
    tv = ML.many_lut_poly([[lut_msg(v) for v in range(per)], [lut_t(w, v) for v in range(per)]], T, N)
    delta = (1 << 63) // T
    for v in range(8):                    # every block sum of round 1 (<= 6, <= 7 for block 0)
        assert read_poly(tv, T, ML.output_coefficient(0, 2, N), v) == lut_msg(v) * delta % ML.MOD, (w, v)
        assert read_poly(tv, T, ML.output_coefficient(1, 2, N), v) == lut_t(w, v) * delta % ML.MOD, (w, v)
    # ... and the two one-function tables the pair replaces say the same
    one_msg = ML.many_lut_poly([[lut_msg(v) for v in range(T)]], T, N)
    one_t = ML.many_lut_poly([[lut_t(w, v) % 32 for v in range(T)]], T, N)
    for v in range(8):
        assert read_poly(one_msg, T, 0, v) == read_poly(tv, T, 0, v)
        assert read_poly(one_t, T, 0, v) == read_poly(tv, T, N // 2, v)


def group_max(arity, t):
    """The grouping rule of helm_si_set_level_many_lut: the largest M with 2^arity <= t / M; 1 = no sharing."""
    return t >> arity if arity >= 2 and (1 << arity) <= t else 1


def groups_of(n_gates, arity, t):
    """Rotations of n_gates gates on one input tuple."""
    gm = group_max(arity, t)
    return -(-n_gates // gm)


def test_grouping_rule():
    assert group_max(3, 16) == 2
    assert group_max(2, 16) == 4
    assert group_max(2, 8) == 2
    assert group_max(2, 4) == 1 and group_max(3, 8) == 1 and group_max(4, 16) == 1   # the index needs the whole space
    assert group_max(0, 16) == group_max(1, 16) == 1                                   # no bootstrap to share
    assert group_max(5, 16) == 1                                                       # (refused by the level itself)
    for t in (4, 8, 16, 32):
        for arity in range(2, 6):
            M = group_max(arity, t)
            assert M & (M - 1) == 0
            assert M == 1 or (1 << arity) <= t // M                # a group's index is below its table's input bound
            assert (1 << arity) > t // (2 * M) or (1 << arity) > t  # and M is the largest such
    # a full adder (0x96 and 0xE8 on the same three inputs) at t = 16: one rotation; the 8-bit adder: 8 instead of 16
    assert groups_of(2, 3, 16) == 1 and 8 * groups_of(2, 3, 16) == 8
    assert groups_of(3, 3, 16) == 2 and groups_of(5, 2, 16) == 2 and groups_of(2, 2, 4) == 2


def test_grouped_gates_read_their_own_function():
    """A pair of arity-3 gates in a dispatch of n_out = 4 (a level that also holds four arity-2 gates on one tuple): the pair's
    table has M = 2 chunks, so its gates are outputs 0 and 2 of the four - coefficients 0 and N / 2."""
    tables = [0x96, 0xE8]
    per = T // 2
    tv = ML.many_lut_poly([[(tb >> (v & 7)) & 1 for v in range(per)] for tb in tables], T, N)
    delta = (1 << 63) // T
    Md, Mg = 4, 2
    for i, tb in enumerate(tables):
        h = ML.output_coefficient(i * (Md // Mg), Md, N)
        assert h == i * N // 2
        for v in range(8):
            assert read_poly(tv, T, h, v) == ((tb >> v) & 1) * delta, (i, v)
