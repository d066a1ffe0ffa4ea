"""CPU unit tests of vartrix_amd/csrc/vtx_call_core.h — what one thread of reduce_count_kernel / reduce_emit_kernel does with its
(row, cell) group — built for the host by tests/callcore/Makefile, against tests/call_model.py: every call boundary, all 164 UMI-family
compositions of tests/call_cases.py (with and without None reads mixed in, as one family and as a family among others), every cell
composition, the keep rule and the three value formulas as bit patterns.  The device runs the same function through the kernels in
tests/test_gpu_reduce_onepass.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import call_cases as CC
import call_model as CM

HERE = os.path.dirname(os.path.abspath(__file__))
M = 25                                                   # min_score of the synthetic scores below
SCORE = {CM.REF: (40, 34), CM.ALT: (34, 40), CM.UNKNOWN: (40, 40), None: (24, 10)}
NAME = {0: CM.REF, 1: CM.ALT, 2: CM.UNKNOWN, 3: None}    # vtxcall::CALL_*


@pytest.fixture(scope="module")
def core():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "callcore"), "-s"])
    L = C.CDLL(os.path.join(HERE, "callcore", "libcall_host.so"))
    L.vtxt_call_of.restype = L.vtxt_collapse_of.restype = C.c_uint32
    L.vtxt_call_of.argtypes = [C.c_int32] * 3
    L.vtxt_collapse_of.argtypes = [C.c_uint32] * 3
    L.vtxt_count_group.restype = None
    L.vtxt_count_group.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_int, C.c_void_p]
    L.vtxt_keep_of.restype = C.c_int
    L.vtxt_keep_of.argtypes = [C.c_uint32] * 3 + [C.c_int]
    L.vtxt_values_of.restype = None
    L.vtxt_values_of.argtypes = [C.c_uint32] * 3 + [C.c_int, C.c_void_p]
    return L


def count(core, calls, heads, begin, end, use_umi, min_score=M):
    """count_group over records whose calls are `calls` (scores from SCORE), family heads `heads`."""
    ref = np.array([SCORE[c][0] for c in calls], np.int32)
    alt = np.array([SCORE[c][1] for c in calls], np.int32)
    hu = np.array(heads, np.uint32)
    out = np.zeros(3, np.uint32)
    core.vtxt_count_group(ref.ctypes.data, alt.ctypes.data, hu.ctypes.data, begin, end, min_score, use_umi, out.ctypes.data)
    return tuple(int(x) for x in out)


def test_every_call_boundary(core):
    for m in (0, 1, 25, 26, 151):
        for rs in (-1, 0, 1, 24, 25, 26, 150, 151):
            for as_ in (-1, 0, 1, 24, 25, 26, 150, 151):
                assert NAME[core.vtxt_call_of(rs, as_, m)] == CM.evaluate(rs, as_, m), (rs, as_, m)


def family_calls(r, a, k, shift):
    calls = [CM.REF] * r + [CM.ALT] * a + [CM.UNKNOWN] * k
    return calls[shift % len(calls):] + calls[:shift % len(calls)]


def test_all_164_family_compositions(core):
    assert len(CC.FAMILIES) == 164
    for i, (r, a, k) in enumerate(CC.FAMILIES):
        want = CM.collapse(family_calls(r, a, k, 0))
        assert NAME[core.vtxt_collapse_of(r, a, k)] == want, (r, a, k)
        one_hot = tuple(int(want == c) for c in (CM.REF, CM.ALT, CM.UNKNOWN))
        for nones in (0, 1 + i % 3):
            calls = family_calls(r, a, k, i)
            for j in range(nones):
                calls.insert((i + 2 * j) % (len(calls) + 1), None)
            heads = [1] + [0] * (len(calls) - 1)
            # the family alone in its group: with UMIs its collapsed call, without them its reads
            assert count(core, calls, heads, 0, len(calls), 1) == one_hot, (r, a, k, nones)
            assert count(core, calls, heads, 0, len(calls), 0) == (r, a, k), (r, a, k, nones)
            # the same family between a REF family and a family of None reads, inside a longer array (begin > 0, end < n)
            arr = [CM.ALT] + [CM.REF, CM.REF] + calls + [None, None] + [CM.ALT]
            hd = [1] + [1, 0] + heads + [1, 0] + [1]
            got = count(core, arr, hd, 1, len(arr) - 1, 1)
            assert got == (one_hot[0] + 1, one_hot[1], one_hot[2]), (r, a, k, nones, got)
    assert NAME[core.vtxt_collapse_of(0, 0, 0)] is None
    assert count(core, [None, None], [1, 0], 0, 2, 1) == (0, 0, 0)
    assert count(core, [CM.REF], [1], 0, 0, 1) == (0, 0, 0) and count(core, [CM.REF], [1], 0, 0, 0) == (0, 0, 0)      # an empty range


def test_a_300_read_family_at_exactly_three_quarters(core):
    calls = [CM.ALT if j % 4 else CM.REF for j in range(300)]                    # 225 : 75
    assert count(core, calls, [1] + [0] * 299, 0, 300, 1) == (0, 1, 0)
    calls[1] = CM.REF                                                             # 224 : 76
    assert count(core, calls, [1] + [0] * 299, 0, 300, 1) == (0, 0, 1)


def test_groups_keep_and_values_equal_the_model(core):
    """A locus of random cells and families through CM.run in every mode, with and without UMIs; the core, group by group, gives the
    same entries bit for bit."""
    rng = np.random.default_rng(12)
    records, calls = [], []
    for cell in range(300):
        for umi in range(int(rng.integers(1, 5))):
            for _ in range(int(rng.integers(1, 6))):
                records.append((cell, umi))
                calls.append((CM.REF, CM.ALT, CM.UNKNOWN, None)[int(rng.choice(4, p=(0.3, 0.3, 0.15, 0.25)))])
    n = len(records)
    ref = np.array([SCORE[c][0] for c in calls], np.int32)
    alt = np.array([SCORE[c][1] for c in calls], np.int32)
    head_cell = [i == 0 or records[i][0] != records[i - 1][0] for i in range(n)]
    head_umi = [int(i == 0 or records[i] != records[i - 1]) for i in range(n)]
    starts = [i for i in range(n) if head_cell[i]] + [n]
    vals = np.zeros(2, np.float64)
    for use_umi in (0, 1):
        for mode in (CM.CONSENSUS, CM.ALT_FRAC, CM.COVERAGE):
            for m in (25, 151):
                want, _ = CM.run([(7, 0, n)], records, ref, alt, m, use_umi, mode)
                got = []
                for g in range(len(starts) - 1):
                    r, a, k = count(core, calls, head_umi, starts[g], starts[g + 1], use_umi, m)
                    if core.vtxt_keep_of(r, a, k, mode):
                        core.vtxt_values_of(r, a, k, mode, vals.ctypes.data)
                        got.append((7, records[starts[g]][0], r, a, k, float(vals[0]), float(vals[1])))
                CM.assert_same(CM.as_arrays(got), CM.as_arrays(want), "core, umi %d mode %d min_score %d" % (use_umi, mode, m))
                assert m != 151 or mode != CM.CONSENSUS or not got
