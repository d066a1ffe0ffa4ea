"""vtx_csr_core.h on the CPU: the index arithmetic one lane of the CSR kernels (vartrix_amd/csrc/vtx_csr.hip) does alone — the
boundary -> offsets rule, the validation predicates of a caller's CSR, the row of an entry — compiled for the host by
tests/csrcore/Makefile and compared with numpy / scipy.  The device runs the same source (tests/test_gpu_csr*.py).  What the lanes
TOUCH is checked by a stand-alone program (tests/csrcore/main.cpp) in allocations of exactly the device's size, plain and under
AddressSanitizer and UBSan; nothing sanitized is loaded into Python."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
BAD_FIRST, BAD_ORDER, BAD_LAST, BAD_INDEX, BAD_WINDOW = 1, 2, 4, 8, 16


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "csrcore"), "-s"])
    lib = C.CDLL(os.path.join(HERE, "csrcore", "libcsr_host.so"))
    lib.csr_offsets.restype = C.c_uint64
    lib.csr_offsets.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.csr_check.restype = C.c_uint32
    lib.csr_check.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32]
    lib.csr_window.restype = C.c_uint32
    lib.csr_window.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]
    lib.csr_rows.restype = None
    lib.csr_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    return lib


def rows_with_gaps():
    """Sorted row arrays: empty rows at the start, in the middle (runs of 1, 2 and 70) and at the end; rows with several entries."""
    r = [5] * 3 + [6] + [8] * 2 + [11] + [12] * 4 + [83] + [84] * 2 + [90]      # gaps: 0-4 | 7 | 9-10 | 13-82 | 85-89
    return np.array(r, np.uint32), 100                                          # ... and 91-99 at the end


def offsets(L, key, begin, end):
    key = np.ascontiguousarray(key, np.uint32)
    slots = end - begin + 1
    indptr = np.full(slots, 0xA5A5A5A5A5A5A5A5, np.uint64)
    writes = np.zeros(slots, np.uint8)
    outside = L.csr_offsets(key.ctypes.data if key.size else None, key.size, begin, end, indptr.ctypes.data, writes.ctypes.data)
    assert outside == 0                                    # no lane stores outside the end - begin + 1 offsets, whatever the keys
    assert np.all(writes == 1)                             # every offset written exactly once, by one lane: no zeroing, no atomics
    return indptr


def want_offsets(key, begin, end):
    return np.searchsorted(np.asarray(key, np.int64), np.arange(begin, end + 1, dtype=np.int64), side="left").astype(np.uint64)


def test_offsets_equal_scipy_on_rows_with_gaps(L):
    row, n_rows = rows_with_gaps()
    col = np.arange(row.size, dtype=np.uint32) % 7
    got = offsets(L, row, 0, n_rows)
    m = sp.coo_matrix((np.ones(row.size), (row, col)), shape=(n_rows, 7)).tocsr()
    assert np.array_equal(got, m.indptr.astype(np.uint64))
    assert np.array_equal(got, want_offsets(row, 0, n_rows))
    lens = np.diff(got.astype(np.int64))
    for r in (0, 4, 7, 9, 10, 13, 82, 85, 89, 91, 99):     # each empty row has an empty range
        assert lens[r] == 0
    assert lens[5] == 3 and lens[12] == 4 and lens[90] == 1


@pytest.mark.parametrize("begin,end", [(0, 100), (5, 91), (5, 90), (6, 84), (13, 83), (14, 82), (40, 41), (50, 50), (0, 0), (100, 100), (91, 100)])
def test_offsets_in_windows_that_cut_the_rows(L, begin, end):
    """A window [begin, end): the offsets of its rows are the positions in the WHOLE array, whether or not it holds every entry (a
    window that does not is refused by csr_window_kernel before the offsets are used, but the rule stays inside its slots)."""
    row, _ = rows_with_gaps()
    assert np.array_equal(offsets(L, row, begin, end), want_offsets(row, begin, end))
    inside = bool(np.all((row >= begin) & (row < end)))
    assert L.csr_window(row.ctypes.data, row.size, begin, end) == (0 if inside else BAD_WINDOW)


def test_offsets_without_entries_and_with_one_full_row(L):
    assert np.array_equal(offsets(L, np.zeros(0, np.uint32), 0, 9), np.zeros(10, np.uint64))            # nnz = 0: all zero
    assert np.array_equal(offsets(L, np.zeros(0, np.uint32), 4, 4), np.zeros(1, np.uint64))
    one = np.full(1000, 3, np.uint32)                                                                   # one row holds everything
    want = np.array([0, 0, 0, 0, 1000, 1000, 1000], np.uint64)
    assert np.array_equal(offsets(L, one, 0, 6), want)
    assert np.array_equal(offsets(L, one, 3, 4), np.array([0, 1000], np.uint64))
    top = np.array([0xFFFFFFFE] * 2, np.uint32)                                                         # no 32-bit wrap at the top
    assert np.array_equal(offsets(L, top, 0xFFFFFFF0, 0xFFFFFFFF), want_offsets(top, 0xFFFFFFF0, 0xFFFFFFFF))


@pytest.mark.parametrize("gap", [254, 255, 256, 257, 258, 1000, 100003])
def test_long_gaps_are_split_over_row_lanes(L, gap):
    """Intervals of more than 256 rows are left to the per-row lanes (csr_fill_kernel), shorter ones to the boundary lane: around the
    threshold, in front of the first key, between two keys and behind the last, every offset is still written exactly once."""
    for key, n_rows in (([gap], gap + 1), ([0, gap], gap + 1), ([0, 0, gap - 1, gap - 1], 2 * gap), ([5, 5 + gap, 5 + gap, 9 + 2 * gap], 12 + 3 * gap),
                        ([], gap)):
        key = np.array(key, np.uint32)
        assert np.array_equal(offsets(L, key, 0, n_rows), want_offsets(key, 0, n_rows))
        assert np.array_equal(offsets(L, key, 3, n_rows + 300), want_offsets(key, 3, n_rows + 300))


def test_offsets_random_against_numpy(L):
    rng = np.random.default_rng(12)
    for _ in range(200):
        n_rows = int(rng.integers(1, 300))
        n = int(rng.integers(0, 400))
        key = np.sort(rng.integers(0, n_rows, n)).astype(np.uint32)
        assert np.array_equal(offsets(L, key, 0, n_rows), want_offsets(key, 0, n_rows))


def check(L, indptr, nnz, indices, n_minor):
    indptr = np.ascontiguousarray(indptr, np.uint64)
    indices = np.ascontiguousarray(indices, np.uint32)
    return L.csr_check(indptr.ctypes.data, indptr.size - 1, nnz, indices.ctypes.data if indices.size else None, n_minor)


def test_validation_predicates_name_each_kind_of_bad_input(L):
    good_ptr, idx = [0, 2, 2, 5], [1, 3, 0, 0, 3]
    assert check(L, good_ptr, 5, idx, 4) == 0
    assert check(L, [0], 0, [], 0) == 0                                  # no rows, no columns, no entries
    assert check(L, [0, 0, 0], 0, [], 7) == 0
    assert check(L, [1, 2, 2, 5], 5, idx, 4) == BAD_FIRST
    assert check(L, [0, 3, 2, 5], 5, idx, 4) == BAD_ORDER
    assert check(L, [0, 2, 2, 4], 5, idx, 4) == BAD_LAST
    assert check(L, [0, 2, 2, 6], 5, idx, 4) == BAD_LAST
    assert check(L, good_ptr, 5, [1, 3, 0, 4, 3], 4) == BAD_INDEX        # an index == n_minor
    assert check(L, good_ptr, 5, [1, 3, 0, 0xFFFFFFFF, 3], 4) == BAD_INDEX
    assert check(L, [0, 2, 2, 5], 5, idx, 0) == BAD_INDEX                # no columns at all
    assert check(L, [2, 1, 9], 5, [9] * 5, 4) == BAD_FIRST | BAD_ORDER | BAD_LAST | BAD_INDEX
    assert check(L, [0, 1 << 40, 5], 5, idx, 4) == BAD_ORDER             # 64-bit offsets are compared as such


def test_row_of_skips_empty_rows(L):
    rng = np.random.default_rng(3)
    for n_major, n in ((1, 1), (1, 300), (300, 1), (70, 200), (1000, 40)):
        row = np.sort(rng.integers(0, n_major, n)).astype(np.uint32)
        indptr = want_offsets(row, 0, n_major)
        p = np.arange(n, dtype=np.uint32)
        out = np.zeros(n, np.uint32)
        L.csr_rows(indptr.ctypes.data, n_major, p.ctypes.data, n, out.ctypes.data)
        assert np.array_equal(out, row)


def run_program(name, cases):
    """cases: [(begin, end, keys)] through tests/csrcore/main.cpp in ONE process -> [(indptr, rows)]."""
    import tempfile
    subprocess.check_call(["make", "-C", os.path.join(HERE, "csrcore"), "-s", name])
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<I", len(cases)))
            for begin, end, key in cases:
                f.write(struct.pack("<III", begin, end, len(key)) + np.asarray(key, "<u4").tobytes())
        r = subprocess.run([os.path.join(HERE, "csrcore", name), src, dst], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        blob = open(dst, "rb").read()
    out, p = [], 0
    for begin, end, key in cases:
        slots = end - begin + 1
        indptr = np.frombuffer(blob, "<u8", slots, p)
        p += 8 * slots
        rows = np.frombuffer(blob, "<u4", len(key), p)
        p += 4 * len(key)
        out.append((indptr, rows))
    assert p == len(blob)
    return out


@pytest.mark.parametrize("name", ["csr_host", "csr_host_san"])
def test_what_the_lanes_touch(name):
    """The offsets rule and the row search in allocations of exactly the device's sizes — under AddressSanitizer and UBSan in the
    second build: windows that cut the rows, no entries, one row holding everything, and random arrays."""
    row, n_rows = rows_with_gaps()
    rng = np.random.default_rng(7)
    cases = [(0, n_rows, row), (5, 91, row), (6, 84, row), (40, 41, row), (50, 50, row), (0, 0, row), (100, 100, row),
             (0, 9, []), (4, 4, []), (0, 255, [255]), (0, 256, [256]), (0, 257, [257]), (7, 3000, [9, 9, 1500, 2999]), (0, 6, [3] * 1000), (3, 4, [3] * 1000), (0xFFFFFFF0, 0xFFFFFFFF, [0xFFFFFFFE] * 2)]
    for _ in range(40):
        m = int(rng.integers(1, 200))
        cases.append((0, m, np.sort(rng.integers(0, m, int(rng.integers(0, 300))))))
    for (begin, end, key), (indptr, rows) in zip(cases, run_program(name, cases)):
        key = np.asarray(key, np.int64)
        assert np.array_equal(indptr, want_offsets(key, begin, end)), (begin, end)
        if np.all((key >= begin) & (key < end)):
            assert np.array_equal(rows, key.astype(np.uint32)), (begin, end)
        else:
            assert np.all(rows == 0xFFFFFFFF)
