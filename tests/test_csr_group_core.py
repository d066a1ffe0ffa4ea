"""vtx_csr_group_core.h on the CPU: what one lane of the pseudobulk kernels (vartrix_amd/csrc/vtx_csr_group.hip) does alone — the label
check, the window of a label, an entry's contribution to the bins of its group, the slot of a non-empty bin from a ballot and a carried
rank — compiled for the host by tests/csrgroupcore/Makefile with the lanes as loops and the tile as an array, against the numpy model of
tests/csr_group_util.py.  The device runs the same source (tests/test_gpu_csr_group.py).  What the lanes TOUCH is checked by a
stand-alone program (tests/csrgroupcore/main.cpp) in allocations of exactly the device's sizes, plain and under AddressSanitizer and
UBSan; nothing sanitized is loaded into Python."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from tests.csr_group_util import NAMES, NONE, cases, first_bad_label, model_group_sum
from tests.csr_ops_util import COUNTS, model_stats

HERE = os.path.dirname(os.path.abspath(__file__))
P32, P64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "csrgroupcore"), "-s"])
    lib = C.CDLL(os.path.join(HERE, "csrgroupcore", "libcsrgroup_host.so"))
    for f in (lib.csrgroup_window, lib.csrgroup_max, lib.csrgroup_tile_bytes):
        f.restype, f.argtypes = C.c_uint32, []
    lib.csrgroup_first_bad.restype = C.c_uint32
    lib.csrgroup_first_bad.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    lib.csrgroup_plan.restype = C.c_uint32
    lib.csrgroup_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.csrgroup_sum.restype = None
    lib.csrgroup_sum.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 5 + [C.c_uint32] + [C.c_void_p] * 10
    return lib


def ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def fold(L, indptr, indices, counts, group, n_groups, names=NAMES):
    n_major = len(indptr) - 1
    pos = np.full(n_major + 1, P32, np.uint32)
    n_out = L.csrgroup_plan(indptr.ctypes.data, n_major, ptr(indices), ptr(group), n_groups, pos.ctypes.data)
    assert pos[0] == 0 and pos[-1] == n_out and np.all(np.diff(pos.astype(np.int64)) >= 0)
    out = {"indptr": np.full(n_major + 1, P64, np.uint64), "indices": np.full(n_out, P32, np.uint32)}
    out.update({k: np.full(n_out, P32, np.uint32) if k in COUNTS else np.full(n_out, P64, np.uint64) for k in names})
    stores = np.zeros(n_out, np.uint8)
    L.csrgroup_sum(indptr.ctypes.data, n_major, ptr(indices), *[ptr(a) for a in counts], ptr(group), n_groups, out["indptr"].ctypes.data,
                   ptr(out["indices"]), ptr(stores), *[ptr(out.get(k)) for k in NAMES])
    assert np.all(stores == 1)                             # every output entry stored exactly once, by one lane
    assert np.array_equal(out["indptr"], pos.astype(np.uint64))
    return out


def same(got, want, names=("indptr", "indices") + NAMES):
    for k in names:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def test_constants(L):
    """At most 256 passes over a row; a tile of 40 bytes a group, four of them (a block) at most half of a CU's 160 KiB of LDS."""
    w = L.csrgroup_window()
    assert w >= 64 and w % 64 == 0 and L.csrgroup_max() <= 256 * w and L.csrgroup_max() < NONE
    assert L.csrgroup_tile_bytes() == 40 * w and 4 * L.csrgroup_tile_bytes() <= 80 * 1024


CASES = None


def all_cases(L):
    global CASES
    if CASES is None:
        CASES = cases(L.csrgroup_window())
    return CASES


def test_every_case_against_the_model(L):
    seen = set()
    for name, indptr, indices, n_minor, counts, group, n_groups in all_cases(L):
        assert L.csrgroup_first_bad(ptr(group), n_minor, n_groups) == NONE, name
        got, want = fold(L, indptr, indices, counts, group, n_groups), model_group_sum(indptr, indices, *counts, group, n_groups)
        same(got, want)
        seen.add(name)
        for r in range(len(indptr) - 1):                   # group numbers ascend inside a row
            assert np.all(np.diff(got["indices"][int(got["indptr"][r]):int(got["indptr"][r + 1])].astype(np.int64)) > 0), name
        if name == "every_cell_left_out":
            assert len(got["indices"]) == 0 and not got["indptr"].any()
        if name == "identity":                             # one group per column on a canonical CSR: the matrix itself
            assert np.array_equal(got["indptr"], indptr) and np.array_equal(got["indices"], indices)
            assert np.array_equal(got["sum_alt"], counts[0]) and np.array_equal(got["sum_ref"], counts[1]) and np.array_equal(got["sum_unk"], counts[2])
            assert np.all(got["n_entries"] == 1)
        if name == "a_group_without_cells":
            assert not np.isin(got["indices"], [1, 4]).any()
        if name == "sums_past_2_32":
            assert want["sum_alt"].max() > 1 << 32 and want["sum_unk"].max() > 1 << 32
        if name.startswith("groups_") and n_groups > 64:   # the row that holds every column has both sides of every 64-bin step
            full = int(np.argmax(np.diff(indptr.astype(np.int64)) == n_minor))
            row = got["indices"][int(got["indptr"][full]):int(got["indptr"][full + 1])]
            assert all(e - 1 in row and e in row for e in range(64, n_groups, 64))
    assert len(seen) == len(CASES) >= 20


def test_one_group_is_the_row_statistics(L):
    """All labels 0: one entry per non-empty row, its numbers those of vtx_csr_row_stats' model."""
    for name, indptr, indices, n_minor, counts, _, _ in all_cases(L):
        got = fold(L, indptr, indices, counts, np.zeros(n_minor, np.uint32), 1)
        want = model_stats(indptr, *counts)
        full = np.diff(indptr.astype(np.int64)) > 0
        assert np.array_equal(np.diff(got["indptr"].astype(np.int64)), full.astype(np.int64)) and not got["indices"].any()
        for k in NAMES:
            assert np.array_equal(got[k], want[k][full]), (name, k)


def test_null_outputs_are_skipped(L):
    name, indptr, indices, n_minor, counts, group, n_groups = all_cases(L)[4]
    want = model_group_sum(indptr, indices, *counts, group, n_groups)
    for names in (("n_alt", "sum_ref"), ("sum_unk",), ("n_entries",), ()):
        got = fold(L, indptr, indices, counts, group, n_groups, names)
        assert set(got) == {"indptr", "indices"} | set(names)
        same(got, want, ("indptr", "indices") + tuple(names))


def test_label_check_names_the_lowest_column(L):
    group = np.array([0, 1, NONE, 2, 1], np.uint32)
    assert L.csrgroup_first_bad(group.ctypes.data, 5, 3) == NONE and first_bad_label(group, 3) is None
    assert L.csrgroup_first_bad(group.ctypes.data, 5, 2) == 3 == first_bad_label(group, 2)          # a label == n_groups
    assert L.csrgroup_first_bad(group.ctypes.data, 5, 1) == 1 == first_bad_label(group, 1)          # two of them: the lowest
    group[4] = 0xFFFFFFFE
    assert L.csrgroup_first_bad(group.ctypes.data, 5, 3) == 4 == first_bad_label(group, 3)
    assert L.csrgroup_first_bad(None, 0, 3) == NONE


def run_program(name, todo):
    """Cases through tests/csrgroupcore/main.cpp in ONE process -> [None for refused labels, else the fold]."""
    subprocess.check_call(["make", "-C", os.path.join(HERE, "csrgroupcore"), "-s", name])
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<I", len(todo)))
            for _, indptr, indices, n_minor, counts, group, n_groups in todo:
                f.write(struct.pack("<IIII", len(indptr) - 1, n_minor, len(indices), n_groups))
                f.write(np.asarray(indptr, "<u8").tobytes())
                for a in (indices, *counts, group):
                    f.write(np.asarray(a, "<u4").tobytes())
        r = subprocess.run([os.path.join(HERE, "csrgroupcore", name), src, dst], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        blob = open(dst, "rb").read()
    out, p = [], 0

    def take(dtype, n):
        nonlocal p
        a = np.frombuffer(blob, dtype, n, p)
        p += a.nbytes
        return a
    for _, indptr, *_ in todo:
        if int(take("<u4", 1)[0]) != NONE:
            out.append(None)
            continue
        n = int(take("<u4", 1)[0])
        got = {"indptr": take("<u8", len(indptr)), "indices": take("<u4", n)}
        got.update({k: take("<u4" if k in COUNTS else "<u8", n) for k in NAMES})
        out.append(got)
    assert p == len(blob)
    return out


@pytest.mark.parametrize("name", ["csr_group_host", "csr_group_host_san"])
def test_what_the_lanes_touch(L, name):
    """The count, the walk and the sweep in allocations of exactly the device's sizes — under AddressSanitizer and UBSan in the second
    build: every case above, and one whose labels are refused."""
    todo = list(all_cases(L))
    bad = list(todo[0])
    bad[5] = bad[5].copy()
    bad[5][17] = bad[6]                                    # a label == n_groups
    todo.append(tuple(bad))
    got = run_program(name, todo)
    assert got[-1] is None
    for case, g in zip(todo[:-1], got):
        _, indptr, indices, n_minor, counts, group, n_groups = case
        same(g, model_group_sum(indptr, indices, *counts, group, n_groups))
