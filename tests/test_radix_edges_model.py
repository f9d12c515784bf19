"""tests/radix_edges.py checked on the CPU: the operand catalogue against arithmetic done another way (digit by digit, bit by
bit), the table families against their decoder, and the restated scratch walk of RadixEngine (helm_amd/csrc/host/
shortint_circuit.cpp) against the source's text and against what the level declares.

The finding this file pins: scratch_rows() used to be a closed form, (4 nb + 4) vectors of nb rows for a multiplication.  The
term reduction groups terms while the sum of their bounds stays <= 15; a scalar digit 3 gives a term bounded by 9, which is
reduced ALONE into two vectors.  For a scalar whose digits are all 3 the walk takes

    nb          4    8    16    32    64
    vectors    16   33    69   137   276          (digit terms + every reduction round's message / carry vectors)
    closed form 20  36    68   132   260

so the closed form fell short in vectors from 16 blocks on.  In rows the level wrote past its declared scratch from 32 blocks
on (nb x the difference, less what propagate leaves unused of its 5 W + 16 rows: 55 of 176 at nb = 32, 91 of 336 at nb = 64,
and at nb = 16 the 42 unused rows still covered the one vector of 16): 105 rows at nb = 32, 933 at nb = 64.  scratch_rows() is now
the walk itself run dry, and take() panics past the region's end.

With the budget being the walk, `used <= declared` below is a statement about the restatement alone (prop_rows bounds what
propagate takes); the C++ is tied to it by the text tripwire here and, on the device, by tests/test_gpu_radix_edges.py, which
asserts helm_host_radix_scratch_rows() == level_take() for every level it runs."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radix_edges as E  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 16, 17, 32, 64)


# ---- the catalogue -----------------------------------------------------------------------------------------------------
def _add_digits(da, db, carry):
    out = []
    for x, y in zip(da, db):
        s = x + y + carry
        out.append(s & 3)
        carry = s >> 2
    return out


def _by_hand(kind, nb, a, b):
    """The operator on digit and bit lists: no big-integer +, -, *, //, <<, >> on the operands themselves."""
    M = 4 ** nb
    b %= M if kind not in (E.SHL, E.SHR, E.SHL_SCALAR, E.SHR_SCALAR) else 2 * nb
    da, db = E.digits(a, nb), E.digits(b, nb)
    if kind in (E.ADD, E.ADD_SCALAR):
        return E.from_digits(_add_digits(da, db, 0))
    if kind in (E.SUB, E.SUB_SCALAR):
        return E.from_digits(_add_digits(da, [3 - y for y in db], 1))
    if kind in (E.MUL, E.MUL_SCALAR):
        acc = [0] * nb
        for j, y in enumerate(db):
            carry = 0
            for k in range(j, nb):
                s = acc[k] + da[k - j] * y + carry
                acc[k], carry = s & 3, s >> 2
        return E.from_digits(acc)
    bits = [(a >> i) & 1 for i in range(2 * nb)]
    if kind in (E.SHL, E.SHL_SCALAR):
        return sum(v << i for i, v in enumerate(([0] * b + bits)[:2 * nb]))
    if kind in (E.SHR, E.SHR_SCALAR):
        return sum(v << i for i, v in enumerate(bits[b:]))
    if kind in (E.DIV, E.DIV_SCALAR):   # restoring, most significant bit first; a zero divisor accepts every subtraction
        r = q = 0
        for t in range(2 * nb - 1, -1, -1):
            r = 2 * r + bits[t]
            if r >= b:
                r -= b
                q |= 1 << t
        return q
    return a


@pytest.mark.parametrize("nb", WIDTHS)
def test_the_catalogue_against_arithmetic_by_hand(nb):
    M = 4 ** nb
    for kind in range(13):
        cases = E.catalogue(kind, nb)
        assert cases and len({(a, b) for a, b, _ in cases}) == len(cases)
        for a, b, want in cases:
            assert 0 <= a < M and 0 <= want < M and (kind in E.SCALAR_KINDS or 0 <= b < M), (E.KIND_NAMES[kind], nb, a, b)
            assert want == _by_hand(kind, nb, a, b), (E.KIND_NAMES[kind], nb, hex(a), hex(b), hex(want))


@pytest.mark.parametrize("nb", (4, 5, 16, 17, 64))
def test_the_chains_are_what_they_say(nb):
    """generate at s, propagate up to e - 1, absorb at e; block sums reach 6 and 7 in the subtraction of (M - 1, 0)."""
    M = 4 ** nb
    for kind, chain in ((E.ADD, E.add_chain), (E.SUB, E.sub_chain)):
        for s, e in E.seam_pairs(nb):
            a, b = chain(nb, s, e)
            sums = E.block_sums(kind, nb, a, b)
            assert sums[s] >= 4 and all(v == 3 for v in sums[s + 1:min(e, nb)]), (nb, s, e, sums)
            assert e >= nb or sums[e] <= 2
            carried = [i for i in range(nb) if s < i <= e]      # exactly these blocks receive a carry
            want = E.digits(E.answer(kind, nb, a, b), nb)
            for i in range(nb):
                assert want[i] == (sums[i] + (1 if i in carried else 0)) & 3, (nb, s, e, i)
    seams = {(s, e) for s, e in E.seam_pairs(nb)}
    for p in (3, 4, 5, 15, 16, 17, 63, 64):
        if p <= nb:
            assert any(e == p for _, e in seams) and (p >= nb or any(s == p for s, _ in seams))
    sums = E.block_sums(E.SUB, nb, M - 1, 0)
    assert sums[0] == 7 and set(sums[1:]) <= {6}
    assert set(E.block_sums(E.ADD, nb, M - 1, M - 1)) == {6}
    assert set(E.block_sums(E.ADD, nb, E.rep([1], nb), E.rep([2], nb))) == {3}


def test_the_catalogue_holds_the_named_ends():
    for nb in (4, 8, 16):
        M, top = 4 ** nb, 1 << (2 * nb - 1)
        div = {(a, b) for a, b, _ in E.catalogue(E.DIV, nb)}
        assert {(M - 1, 1), (M - 1, 2), (M - 1, 3), (M - 1, M - 1), (M - 1, top), (M - 1, top + 1)} <= div
        assert any(b == 0 for _, b in div) and any(a == 0 for a, _ in div) and any(a == b for a, b in div) and any(a < b for a, b in div)
        assert all(w == M - 1 for _, b, w in E.catalogue(E.DIV_SCALAR, nb) if b == 0)
        sc = [s for _, s, _ in E.catalogue(E.MUL_SCALAR, nb)]
        assert {M - 1, E.rep([2], nb), E.rep([1], nb), E.rep([3, 0], nb), 0, 1, 2, top, 2 * top, 4 * top} <= set(sc) and max(sc) > M
        amounts = {s for _, s, _ in E.catalogue(E.SHL, nb)}
        assert {0, 1, 2, 3, 2 * nb - 1, 2 * nb, 2 * nb + 1, M - 1} <= amounts
        assert {0, 1, 2, 3, 2 * nb - 1, 2 * nb, 2 * nb + 1} <= {s for _, s, _ in E.catalogue(E.SHR_SCALAR, nb)}
        assert {a for a, _, _ in E.catalogue(E.SHR, nb)} == {M - 1, 1, top}
        mul = {(a, b) for a, b, _ in E.catalogue(E.MUL, nb)}
        assert {(M - 1, M - 1), (M - 1, 1), (E.rep([3, 0], nb), E.rep([3, 0], nb)), (3 * 4 ** (nb - 1), 3)} <= mul
        for kind in (E.ADD_SCALAR, E.SUB_SCALAR):
            sc = {s for _, s, _ in E.catalogue(kind, nb)}
            assert 0 in sc and M - 1 in sc and max(sc) >= M


# ---- the decoder -------------------------------------------------------------------------------------------------------
def _make_lut(vals, t, N):
    """helm_si_make_lut restated (helm_amd/csrc/helm_shortint.hip)."""
    delta, box = (1 << 63) // t, N // t
    acc = [0] * N
    for v in range(t):
        for j in range(box):
            acc[v * box + j] = (vals[v] * delta) % 2 ** 64
    for j in range(box // 2):
        acc[j] = (-acc[j]) % 2 ** 64
    return [acc[(j + box // 2) % N] for j in range(N)]


@pytest.mark.parametrize("t,N", [(16, 512), (32, 4096), (16, 2048)])
def test_every_family_decodes_to_itself(t, N):
    delta = (1 << 63) // t
    seen = {}
    for name in E.FAMILIES:
        ent = E.family_entries(name, t)
        got = E.decode_table(_make_lut(ent[:t], t, N), t, delta)
        assert got == ent and E.family_of(got, t) == name, name
        assert E.has_negative_entry(got, t) == (name in E.V3_FAMILIES), name
        seen[tuple(ent)] = name
    assert len(seen) == len(E.FAMILIES) == 27 and len(E._RAW) == 30   # the constructor's 30 tables, three pairs alike
    assert {n for n in E.FAMILIES if '/' in n} == {'resolve/gc2', 'q3/s2', 't2/q1'}
    # the padding-bit rule: a V_3 table read at v in [16, 30] answers minus its entry at v - 16, under both encodings
    for name in E.V3_FAMILIES:
        ent = E.family_entries(name, t)
        for v in range(16, 31):
            assert ent[v] == (-ent[v - 16]) % (2 * t), (name, t, v)
    src = re.sub(r"\s+", "", open(os.path.join(ROOT, "helm_amd", "csrc", "helm_shortint.hip")).read())
    assert "for(intj=0;j<N;j++)tv[j]=acc[(size_t)((j+half)%N)];" in src
    # a pair table of many-LUT carry propagation: message and weighted state over t / 2 inputs each
    per = t // 2
    vals = [v & 3 for v in range(per)] + [E.FAMILIES["t3"](v) for v in range(per)]
    assert E.decode_many_table(_make_lut(vals, t, N), t, delta, 2) == [vals[:per], vals[per:]]


def test_the_weighted_state_sixteen_is_positive_under_both_encodings():
    """Found by this file: add_lut read every entry >= 16 as entry - 32, so lut_t_[3]'s 16 (2 << 3) became - 16.  At t = 16 that
    is the same residue; at t = 32 it is 48, and V_3 = t_0 + 2 t_1 + 4 t_2 + 8 t_3 of four generating blocks came out as
    2 + 4 + 8 + 48 = 62 = - 2 instead of 30: past the padding bit, so the look-up answered with the wrong sign."""
    for t in (16, 32):
        ent = E.family_entries("t3", t)
        assert ent[:8] == [0, 0, 0, 8, 16, 16, 16, 16], (t, ent[:8])
        v3 = sum(E.family_entries(n, t)[6] for n in ("t0", "t1", "t2/q1", "t3")) % (2 * t)
        assert v3 == 30


def test_the_families_are_the_constructors():
    src = re.sub(r"\s+", "", open(os.path.join(ROOT, "helm_amd", "csrc", "host", "shortint_circuit.cpp")).read())
    for line in ("lut_t_[p]=add_lut([p](intv){return(v>=4?2:v==3?1:0)<<p;});",
                 "lut_s_[p]=add_lut([p](intv){returnv==15?0:32-(1<<p);});",
                 "lut_q_[i]=add_lut([i](intv){returnv>=(2<<i)?8:v==(2<<i)-1?4:0;});",
                 "lut_gc_[i]=add_lut([i](intv){returnv>=(2<<i)?4:0;});",
                 "lut_q3_=add_lut([](intv){returnv==15?0:32-4;});", "lut_gc3_=add_lut([](int){return32-2;});",
                 "lut_resolve_=add_lut([](intv){returnv>=8?4:0;});",
                 "lut_final_=add_lut([](intv){return((v&3)+((v>>2)>=2?1:0))&3;});",
                 "lut_cout_=add_lut([](intv){returnv>=8?1:0;});",
                 "lut_sel_=add_lut([](intv){return(v>>2)?(v&3):0;});",
                 "if(t==32)vals[(size_t)v+16]=(uint64_t)((2*t-sv)%(2*t));",
                 # 16 is + 16 (the state "generates" of a group's fourth block, weighted 8), never - 16: see the t = 32 case below
                 "constinte=(int)f(v),sv=e>16?e-32:e;"):
        assert line in src, line


# ---- the scratch walk --------------------------------------------------------------------------------------------------
def test_the_restated_walk_is_the_source():
    """A tripwire on the deciding lines, whitespace-stripped: whoever edits them is asked to edit radix_edges.py too."""
    src = re.sub(r"\s+", "", open(os.path.join(ROOT, "helm_amd", "csrc", "host", "shortint_circuit.cpp")).read())
    for line in (
            "intRadixEngine::prop_rows(intW){return5*W+16;}",
            # the budget is the walk, dry; a real level is bounded by it
            "returnwalk(nullptr,ops,0);",
            "if(rows<0)rows=scratch_rows(ops_in);", "WalkModemode(dry_,scratch_end_,false,(int64_t)scratch+rows);",
            "if(rows<0||(scratch_end_>=0&&(int64_t)sp+rows>scratch_end_))throwPanic(",
            "return(int64_t)sp-scratch;",
            # digit terms of a scalar product, terms of a product and of a square
            "constintbase=take(nb_);", "ms.terms.push_back(Term{base,j,3*digit});",
            "constintLb=take(nb_),Hb=j+1<nb_?take(nb_):-1;", "constintLb=take(nb_),Hb=2*j+1<nb_?take(nb_):-1;",
            "if(Hb>=0)ms.terms.push_back(Term{Hb,2*j+1,4});",
            "ms.terms.push_back(Term{base,0,t==0?3+nc:3});",
            # the reduction
            "constintT=5;", "if(ms.terms.size()>2)returntrue;", "returns>6;",
            "while(e<ms.terms.size()&&e-q<(size_t)T&&s+ms.terms[e].maxv<=15)s+=ms.terms[e++].maxv;",
            "if(e-q==1&&s<=3){", "constintMb=take(nb_),Cb=low+1<nb_?take(nb_):-1;",
            "if(s>3)prop_bases.push_back(ms.out);",
            "propagate(w,prop_bases,take(prop_rows(nb_)*(int)prop_bases.size()),nb_,nullptr);",
            # propagate and carries
            "constintneed=flags?W:W-1;", "constinttbase=take(G*W);", "constintbase=take(G*need);",
            "constintvbase=take(G*n),sbase=take(G*ng);",
            "constintgneed=(need==n&&n%4==0)?n/4-1:need/4;", "CarriesGC=carries(w,s_items,G,ng,gneed,true,sp,true);",
            "constintcbase=take(G*need);",
            # shifts by an encrypted amount, division
            "constintbits0=take(G*nbits),cur0=take(G*nb_),shf0=take(G*nb_),selA0=take(G*nb_),selB0=take(G*nb_);",
            "constintG=(int)dv.size(),W=nb_+1,bits=2*nb_;",
            "constintabit0=take(G*bits),qbit0=take(G*bits),B0=take(G*W),R0=take(G*W),D0=take(G*W),"
            "selA0=take(G*W),selB0=take(G*W),st0=take(prop_rows(W)*G);"):
        assert line in src, line
    # the closed form is gone: no second count that could drift from the walk
    assert "(4*nb_+4)*nb_" not in src
    # six places take rows, all through the checked member
    assert src.count("autotake=[&](introws){returnthis->take(sp,rows);};") == 5


def _kinds(nb, scalar):
    return {"add": [E.Op(E.ADD)], "sub": [E.Op(E.SUB)], "add_scalar": [E.Op(E.ADD_SCALAR, scalar)],
            "sub_scalar": [E.Op(E.SUB_SCALAR, scalar)], "mul": [E.Op(E.MUL)], "square": [E.Op(E.MUL, square=True)],
            "mul_scalar": [E.Op(E.MUL_SCALAR, scalar)], "div": [E.Op(E.DIV)], "div_scalar": [E.Op(E.DIV_SCALAR, scalar)],
            "shl": [E.Op(E.SHL)], "shr": [E.Op(E.SHR)], "shl_scalar": [E.Op(E.SHL_SCALAR, 3)], "shr_scalar": [E.Op(E.SHR_SCALAR, 3)],
            "copy": [E.Op(E.COPY)], "mul_cs": [E.Op(E.MUL, out2=True)], "add_cs": [E.Op(E.ADD, a2=True, b2=True)],
            "sub_cs": [E.Op(E.SUB, a2=True, b2=True)], "sub_cs_out": [E.Op(E.SUB, a2=True, b2=True, out2=True)],
            "add_cs_one": [E.Op(E.ADD, b2=True)], "sub_cs_one": [E.Op(E.SUB, b2=True)]}


def test_what_a_level_writes_stays_inside_what_it_declares():
    """Every operator kind, nb = 1 .. 65, the structured scalar patterns at every width: rows written <= rows declared (the
    walk's own count), every term-group sum <= 15, and propagate inside its 5 W + 16 rows."""
    worst = 0
    for nb in range(1, 66):
        for W in (nb, nb + 1):
            for flags in (False, True):
                assert E.propagate_take(1, W, flags) <= E.prop_rows(W), (W, flags)
                assert E.propagate_take(3, W, flags) == 3 * E.propagate_take(1, W, flags)
        for pname, scalar in E.scalar_patterns(nb).items():
            for name, ops in _kinds(nb, scalar).items():
                declared, used, top = E.level_take(nb, ops)
                assert used <= declared and top <= 15, (nb, pname, name, used, declared, top)
                worst = max(worst, top)
                both, used2, _ = E.level_take(nb, ops + ops + _kinds(nb, scalar)["add"])   # a level of several operators adds up
                assert both == 2 * declared + E.prop_rows(nb) and used2 <= both
    assert worst == 15
    # the carry propagation's real use, as stated in the module docstring
    assert (E.propagate_take(1, 32, False), E.prop_rows(32)) == (121, 176)
    assert (E.propagate_take(1, 64, False), E.prop_rows(64)) == (245, 336)


def test_every_scalar_digit_pattern_at_four_blocks():
    for scalar in range(256):
        declared, used, top = E.level_take(4, [E.Op(E.MUL_SCALAR, scalar)])
        assert used <= declared and top <= 15, scalar
        # at four blocks the closed form held too: the overrun needs 16 blocks
        assert used <= E.closed_form_rows(4, [E.Op(E.MUL_SCALAR, scalar)]), scalar


def test_the_closed_form_undercounted_the_all_three_scalar():
    """The table of the module docstring, and where the closed form first fell short for each structured pattern."""
    vectors = {}
    for nb in (4, 8, 16, 32, 64):
        v, terms = E.op_terms(nb, E.Op(E.MUL_SCALAR, 4 ** nb - 1))
        assert terms == [(j, 9) for j in range(nb)]
        v2, rounds, top, final = E.reduce_terms(nb, terms)
        vectors[nb] = v + v2
        assert top == 15 and len(final) == 2
    assert vectors == {4: 16, 8: 33, 16: 69, 32: 137, 64: 276}
    assert {nb: 4 * nb + 4 for nb in vectors} == {4: 20, 8: 36, 16: 68, 32: 132, 64: 260}
    short = {}
    for nb in (16, 32, 64):
        op = [E.Op(E.MUL_SCALAR, 4 ** nb - 1)]
        _, used, _ = E.level_take(nb, op)
        short[nb] = used - E.closed_form_rows(nb, op)
    # rows past the old budget; 16 blocks were saved by what propagate leaves unused, 32 and 64 were not
    assert (short[32], short[64]) == (105, 933)
    assert short[16] < 0 < short[32] < short[64]
    # the product of two ciphertexts and the other patterns stayed inside the closed form at the integer widths
    for nb in (4, 8, 16, 32, 64):
        for pname, scalar in E.scalar_patterns(nb).items():
            for name in ("mul", "square", "mul_scalar"):
                ops = _kinds(nb, scalar)[name]
                over = E.level_take(nb, ops)[1] - E.closed_form_rows(nb, ops)
                assert over <= 0 or (name == "mul_scalar" and pname in ("all3", "mix3312", "mix321") and nb >= 32), (nb, pname, name, over)
