"""vtx_csr_ops_core.h on the CPU: what one lane of the summary and selection kernels (vartrix_amd/csrc/vtx_csr_ops.hip) does alone — an
entry's contribution to the statistics of its row and the fold of a group of G lanes, the group-size rule, the keep predicate, the
offsets of the selected matrix — compiled for the host by tests/csropscore/Makefile with the lanes as loops, against the numpy models of
tests/csr_ops_util.py.  The device runs the same source (tests/test_gpu_csr_ops.py).  What the lanes TOUCH is checked by a stand-alone
program (tests/csropscore/main.cpp) in allocations of exactly the device's sizes, plain and under AddressSanitizer and UBSan; nothing
sanitized is loaded into Python."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.csr_ops_util import COUNTS, SUMS, csr_with_row_lengths, model_select, model_stats, random_counts

HERE = os.path.dirname(os.path.abspath(__file__))
GROUPS = (1, 2, 4, 8, 16, 32, 64)
P32, P64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "csropscore"), "-s"])
    lib = C.CDLL(os.path.join(HERE, "csropscore", "libcsrops_host.so"))
    lib.csrops_group_lanes.restype = C.c_uint32
    lib.csrops_group_lanes.argtypes = [C.c_uint64, C.c_uint64]
    lib.csrops_row_stats.restype = None
    lib.csrops_row_stats.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 7
    lib.csrops_plan.restype = None
    lib.csrops_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.csrops_select.restype = None
    lib.csrops_select.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64] + [C.c_void_p] * 11
    return lib


def ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def stats(L, indptr, alt, ref, unk, G, names=COUNTS + SUMS):
    n = len(indptr) - 1
    out = {k: np.full(n, P32, np.uint32) if k in COUNTS else np.full(n, P64, np.uint64) for k in names}
    L.csrops_row_stats(indptr.ctypes.data, n, ptr(alt), ptr(ref), ptr(unk), G, *[ptr(out.get(k)) for k in COUNTS + SUMS])
    return out


def select(L, indptr, indices, n_minor, km, kn, pay32, pay64):
    n_major, nnz = len(indptr) - 1, len(indices)
    km, kn = (None if m is None else np.ascontiguousarray(m, np.uint8) for m in (km, kn))
    sizes = np.zeros(3, np.uint32)
    L.csrops_plan(indptr.ctypes.data, n_major, n_minor, ptr(indices), nnz, km.ctypes.data if km is not None else None,
                  kn.ctypes.data if kn is not None else None, sizes.ctypes.data)
    a, b, n = (int(s) for s in sizes)
    out = {"indptr": np.full(a + 1, P64, np.uint64), "indices": np.full(n, P32, np.uint32), "major_ids": np.full(a, P32, np.uint32),
           "minor_ids": np.full(b, P32, np.uint32), "p32": np.full(n, P32, np.uint32), "p64": np.full(n, P64, np.uint64)}
    writes = np.zeros(a + 1, np.uint8)
    # (an array without elements goes in as NULL, as a caller's empty allocation may; the lanes then have nothing to store)
    L.csrops_select(indptr.ctypes.data, n_major, n_minor, ptr(indices), nnz, km.ctypes.data if km is not None else None,
                    kn.ctypes.data if kn is not None else None, out["indptr"].ctypes.data, writes.ctypes.data, ptr(out["indices"]),
                    ptr(out["major_ids"]), ptr(out["minor_ids"]), ptr(pay32), ptr(out["p32"]), ptr(pay64), ptr(out["p64"]))
    assert np.all(writes == 1)                             # every offset written exactly once, by one lane
    return (a, b, n), out


def check_select(L, indptr, indices, n_minor, km, kn, seed=0):
    rng = np.random.default_rng(seed)
    nnz = len(indices)
    pay32 = rng.integers(0, 1 << 32, nnz, dtype=np.uint64).astype(np.uint32)
    pay64 = (np.arange(nnz, dtype=np.uint64) + (1 << 40)) | (np.uint64(0x7FF8) << np.uint64(48))      # NaNs with the position as payload bits
    sizes, got = select(L, indptr, indices, n_minor, km, kn, pay32, pay64)
    want = model_select(indptr, indices, n_minor, km, kn, [pay32, pay64])
    assert sizes == (len(want["major_ids"]), len(want["minor_ids"]), len(want["indices"]))
    for k in ("indptr", "indices", "major_ids", "minor_ids"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["p32"], want["payloads"][0]) and np.array_equal(got["p64"], want["payloads"][1])
    return sizes


@pytest.mark.parametrize("G", GROUPS)
def test_row_stats_every_group_size_and_row_length(L, G):
    """Rows of 0, 1, G - 1, G, G + 1, 63, 64, 65 and 129 entries (each twice, so that a wavefront holds rows of unlike lengths), empty
    rows at both ends: every G gives numpy's answer, and equal answers whatever G."""
    rng = np.random.default_rng(G)
    lens = [0, 0, 1, max(G - 1, 0), G, G + 1, 63, 64, 65, 129] * 2 + [0]
    indptr, _ = csr_with_row_lengths(rng, lens, 129)
    alt, ref, unk = random_counts(rng, int(indptr[-1]))
    got, want = stats(L, indptr, alt, ref, unk, G), model_stats(indptr, alt, ref, unk)
    for k in COUNTS + SUMS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["n_both"] <= np.minimum(got["n_alt"], got["n_ref"]), np.ones(len(lens), bool))


@pytest.mark.parametrize("G", GROUPS)
def test_row_sums_pass_two_to_the_32(L, G):
    rng = np.random.default_rng(100 + G)
    indptr, _ = csr_with_row_lengths(rng, [3, 0, 200, 64, 1], 200)
    alt, ref, unk = random_counts(rng, int(indptr[-1]), big=True)
    got, want = stats(L, indptr, alt, ref, unk, G), model_stats(indptr, alt, ref, unk)
    assert want["sum_alt"].max() > 1 << 32 and want["sum_unk"].max() > 1 << 32
    for k in COUNTS + SUMS:
        assert np.array_equal(got[k], want[k]), k


def test_row_stats_null_outputs_and_no_rows(L):
    """An output array that is NULL is skipped, the others are written; a matrix without rows runs no lane."""
    rng = np.random.default_rng(3)
    indptr, _ = csr_with_row_lengths(rng, [5, 0, 70], 70)
    alt, ref, unk = random_counts(rng, 75)
    want = model_stats(indptr, alt, ref, unk)
    for names in (("n_alt", "n_ref"), ("sum_unk",), ()):
        got = stats(L, indptr, alt, ref, unk, 8, names)
        assert set(got) == set(names)
        for k in names:
            assert np.array_equal(got[k], want[k])
    none = stats(L, np.zeros(1, np.uint64), None, None, None, 4)
    assert all(v.size == 0 for v in none.values())


def test_group_size_rule(L):
    """The smallest power of two G with 8 G >= nnz / n_major, 1 .. 64, from the two numbers alone; both sides of every step."""
    for G in GROUPS:
        for n_major in (1, 3, 1000, 100_000):
            assert L.csrops_group_lanes(8 * G * n_major, n_major) == G                    # mean == 8 G: G lanes
            if G < 64:
                assert L.csrops_group_lanes(8 * G * n_major + 1, n_major) == 2 * G        # just above: the next power
    assert L.csrops_group_lanes(0, 0) == 1 and L.csrops_group_lanes(0, 7) == 1 and L.csrops_group_lanes(3, 7) == 1
    assert L.csrops_group_lanes(300 * 1500, 1500) == 64 and L.csrops_group_lanes((1 << 32) - 1, 1) == 64
    assert L.csrops_group_lanes((1 << 32) - 1, (1 << 32) - 1) == 1 and L.csrops_group_lanes((1 << 32) - 1, 1 << 20) == 64
    # config 3 (23.9 M entries): 100 000 rows of 239 -> 32 lanes; its transpose, 10 000 rows of 2392 -> 64; four reads per locus -> 1
    assert L.csrops_group_lanes(23_923_282, 100_000) == 32 and L.csrops_group_lanes(23_923_282, 10_000) == 64
    assert L.csrops_group_lanes(378_345, 100_000) == 1 and L.csrops_group_lanes(378_345, 10_000) == 8


def test_select_masks_all_false_all_true_null(L):
    rng = np.random.default_rng(5)
    indptr, indices = csr_with_row_lengths(rng, [0, 1, 63, 64, 65, 129, 0, 2], 130)
    n_major, n_minor, nnz = 8, 130, len(indices)
    t, f = np.ones, np.zeros
    assert check_select(L, indptr, indices, n_minor, None, None) == (n_major, n_minor, nnz)
    assert check_select(L, indptr, indices, n_minor, t(n_major, bool), t(n_minor, bool)) == (n_major, n_minor, nnz)
    assert check_select(L, indptr, indices, n_minor, f(n_major, bool), None) == (0, n_minor, 0)
    assert check_select(L, indptr, indices, n_minor, None, f(n_minor, bool)) == (n_major, 0, 0)
    assert check_select(L, indptr, indices, n_minor, f(n_major, bool), f(n_minor, bool)) == (0, 0, 0)
    km, kn = rng.random(n_major) < 0.5, rng.random(n_minor) < 0.5
    check_select(L, indptr, indices, n_minor, km, None)
    check_select(L, indptr, indices, n_minor, None, kn)
    a, b, n = check_select(L, indptr, indices, n_minor, km, kn)
    assert 0 < a < n_major and 0 < b < n_minor and 0 < n < nnz
    # any non-zero byte keeps: a mask of 0 / 2 / 255 selects what the boolean one does
    assert check_select(L, indptr, indices, n_minor, km.astype(np.uint8) * 255, kn.astype(np.uint8) * 2) == (a, b, n)


def test_select_no_rows_and_one_column(L):
    assert check_select(L, np.zeros(1, np.uint64), np.zeros(0, np.uint32), 5, None, np.array([1, 0, 1, 1, 0], bool)) == (0, 3, 0)
    assert check_select(L, np.zeros(1, np.uint64), np.zeros(0, np.uint32), 0, np.zeros(0, bool), np.zeros(0, bool)) == (0, 0, 0)
    indptr = np.array([0, 1, 1, 2, 3], np.uint64)                              # n_minor = 1: rows 0, 2, 3 hold the one column
    indices = np.zeros(3, np.uint32)
    assert check_select(L, indptr, indices, 1, None, None) == (4, 1, 3)
    assert check_select(L, indptr, indices, 1, np.array([0, 1, 1, 0], bool), np.array([1], bool)) == (2, 1, 1)
    assert check_select(L, indptr, indices, 1, None, np.array([0], bool)) == (4, 0, 0)


def test_select_unsorted_and_duplicate_indices(L):
    """Inside a row the entries keep their SOURCE order, sorted or not, and duplicates stay duplicates; the statistics count them."""
    rng = np.random.default_rng(9)
    lens = [4, 0, 300, 7, 1]                                                   # a row longer than n_minor: duplicates
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    indices = rng.integers(0, 40, int(indptr[-1]), dtype=np.uint64).astype(np.uint32)
    for seed in range(4):
        r = np.random.default_rng(seed)
        check_select(L, indptr, indices, 40, r.random(5) < 0.7, r.random(40) < 0.5, seed)
    alt, ref, unk = random_counts(rng, len(indices))
    want = model_stats(indptr, alt, ref, unk)
    for G in GROUPS:
        got = stats(L, indptr, alt, ref, unk, G)
        assert all(np.array_equal(got[k], want[k]) for k in COUNTS + SUMS)
    assert want["n_entries"][2] == 300


def run_program(name, cases):
    """cases: [(indptr, indices, n_minor, alt, ref, unk, keep_major, keep_minor)] through tests/csropscore/main.cpp in ONE process
    -> [({G: statistics}, selection)]."""
    import tempfile
    subprocess.check_call(["make", "-C", os.path.join(HERE, "csropscore"), "-s", name])
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<I", len(cases)))
            for indptr, indices, n_minor, alt, ref, unk, km, kn in cases:
                f.write(struct.pack("<IIIII", len(indptr) - 1, n_minor, len(indices), km is not None, kn is not None))
                f.write(np.asarray(indptr, "<u8").tobytes())
                for a in (indices, alt, ref, unk):
                    f.write(np.asarray(a, "<u4").tobytes())
                for m in (km, kn):
                    if m is not None:
                        f.write(np.asarray(m, np.uint8).tobytes())
        r = subprocess.run([os.path.join(HERE, "csropscore", name), src, dst], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        blob = open(dst, "rb").read()
    out, p = [], 0

    def take(dtype, n):
        nonlocal p
        a = np.frombuffer(blob, dtype, n, p)
        p += a.nbytes
        return a
    for indptr, *_ in cases:
        n_major = len(indptr) - 1
        by_g = {}
        for G in GROUPS:
            by_g[G] = {k: take("<u4", n_major) for k in COUNTS}
            by_g[G].update({k: take("<u8", n_major) for k in SUMS})
        a, b, n = (int(s) for s in take("<u4", 3))
        sel = {"sizes": (a, b, n), "indptr": take("<u8", a + 1), "indices": take("<u4", n), "major_ids": take("<u4", a),
               "minor_ids": take("<u4", b), "p32": take("<u4", n), "p64": take("<u8", n)}
        out.append((by_g, sel))
    assert p == len(blob)
    return out


@pytest.mark.parametrize("name", ["csr_ops_host", "csr_ops_host_san"])
def test_what_the_lanes_touch(name):
    """The walk, the fold and the selection in allocations of exactly the device's sizes — under AddressSanitizer and UBSan in the
    second build: no rows, one column, rows around every group size, sums past 2^32, duplicate indices, and every kind of mask."""
    rng = np.random.default_rng(11)
    cases = []

    def add(lens, n_minor, km=None, kn=None, big=False, dup=False):
        if dup:
            indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
            indices = rng.integers(0, n_minor, int(indptr[-1]), dtype=np.uint64).astype(np.uint32)
        else:
            indptr, indices = csr_with_row_lengths(rng, lens, n_minor, sort=bool(rng.integers(2)))
        cases.append((indptr, indices, n_minor, *random_counts(rng, len(indices), big), km, kn))
    add([], 4)
    add([], 0, np.zeros(0, bool), np.zeros(0, bool))
    add([1, 0, 1], 1, np.array([1, 1, 0], bool), np.array([1], bool))
    lens = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 0]
    add(lens, 129)
    add(lens, 129, rng.random(20) < 0.5, rng.random(129) < 0.5, big=True)
    add(lens, 129, np.zeros(20, bool), None)
    add(lens, 129, None, np.zeros(129, bool))
    add(lens, 129, np.ones(20, bool), np.ones(129, bool))
    add([300, 0, 5], 16, rng.random(3) < 0.7, rng.random(16) < 0.5, dup=True)
    for _ in range(20):
        n_major, n_minor = int(rng.integers(1, 80)), int(rng.integers(1, 90))
        add(rng.integers(0, n_minor + 1, n_major), n_minor, rng.random(n_major) < 0.6 if rng.integers(2) else None,
            rng.random(n_minor) < 0.6 if rng.integers(2) else None)
    for (indptr, indices, n_minor, alt, ref, unk, km, kn), (by_g, sel) in zip(cases, run_program(name, cases)):
        want = model_stats(indptr, alt, ref, unk)
        for G in GROUPS:
            for k in COUNTS + SUMS:
                assert np.array_equal(by_g[G][k], want[k]), (G, k)
        wide = np.arange(len(indices), dtype=np.uint64) + (1 << 40)
        ws = model_select(indptr, indices, n_minor, km, kn, [alt, wide])
        assert sel["sizes"] == (len(ws["major_ids"]), len(ws["minor_ids"]), len(ws["indices"]))
        for k in ("indptr", "indices", "major_ids", "minor_ids"):
            assert np.array_equal(sel[k], ws[k]), k
        assert np.array_equal(sel["p32"], ws["payloads"][0]) and np.array_equal(sel["p64"], ws["payloads"][1])
