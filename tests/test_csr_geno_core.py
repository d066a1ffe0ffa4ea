"""vtx_csr_geno_core.h on the CPU: what one lane of the donor tally kernels (vartrix_amd/csrc/vtx_csr_geno.hip) does alone — the check of
a genotype byte, the lane's donor and entries, an entry's contribution by predicated additions, the fold over the sub-groups, the place
of a number in the output — compiled for the host by tests/csrgenocore/Makefile with the lanes as loops and the exchange between lanes
as array reads, against the numpy model of tests/csr_geno_util.py.  The device runs the same source (tests/test_gpu_csr_geno.py).  What
the lanes TOUCH is checked by a stand-alone program (tests/csrgenocore/main.cpp) in allocations of exactly the device's sizes, plain and
under AddressSanitizer and UBSan; nothing sanitized is loaded into Python."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from tests.csr_geno_util import DONORS, NAMES, NONE, cases, first_bad_geno, model_geno_tally

HERE = os.path.dirname(os.path.abspath(__file__))
P32, P64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
NO_BAD = (1 << 64) - 1


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "csrgenocore"), "-s"])
    lib = C.CDLL(os.path.join(HERE, "csrgenocore", "libcsrgeno_host.so"))
    for f in (lib.csrgeno_max, lib.csrgeno_none, lib.csrgeno_tally_bytes):
        f.restype, f.argtypes = C.c_uint32, []
    lib.csrgeno_lane_map.restype = C.c_uint32
    lib.csrgeno_lane_map.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.csrgeno_fold_strides.restype = C.c_uint32
    lib.csrgeno_fold_strides.argtypes = [C.c_uint32, C.c_void_p]
    lib.csrgeno_first_bad.restype = C.c_uint64
    lib.csrgeno_first_bad.argtypes = [C.c_void_p, C.c_uint64]
    lib.csrgeno_tally.restype = None
    lib.csrgeno_tally.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32] + [C.c_void_p] * 4
    return lib


def ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def tally(L, indptr, indices, counts, geno, n_donors, names=NAMES):
    n_major = len(indptr) - 1
    shape = (n_major, n_donors, 4)
    out = {k: np.full(shape, P32, np.uint32) if k == "n_obs" else np.full(shape, P64, np.uint64) for k in names}
    stores = np.zeros(shape, np.uint8)
    L.csrgeno_tally(indptr.ctypes.data, n_major, ptr(indices), *[ptr(a) for a in counts], ptr(geno), n_donors,
                    *[ptr(out.get(k)) for k in NAMES], ptr(stores))
    assert np.all(stores == 1)                             # every output element stored exactly once, by one lane
    return out


def same(got, want, names=NAMES):
    for k in names:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


CASES = None


def all_cases():
    global CASES
    if CASES is None:
        CASES = [(c, model_geno_tally(c[1], c[2], *c[4], c[5], c[6])) for c in cases()]
    return CASES


def test_constants(L):
    """At most 16 passes of 64 donors; the byte of no call; twelve numbers a lane: eight of 64 bits and four of 32."""
    assert L.csrgeno_max() == 64 * 16 and L.csrgeno_none() == NONE == 0xFF and L.csrgeno_tally_bytes() == 8 * 8 + 4 * 4


def test_the_lane_map(L):
    """Per pass: Dp the smallest power of two that holds the pass's donors, 64 / Dp sub-groups of Dp lanes, a lane live when its donor
    exists; the fold's distances are Dp, 2 Dp, ... 32."""
    sub, d, live, strides = np.zeros(64, np.uint32), np.zeros(64, np.uint32), np.zeros(64, np.uint8), np.zeros(8, np.uint32)
    for n in DONORS + [4, 16, 17, 32, 127, 128, 1024]:
        for base in range(0, n, 64):
            count = min(64, n - base)
            dp = L.csrgeno_lane_map(n, base, sub.ctypes.data, d.ctypes.data, live.ctypes.data)
            assert dp >= count and dp & (dp - 1) == 0 and (dp == 1 or dp // 2 < count), (n, base, dp)
            lane = np.arange(64)
            assert np.array_equal(sub, lane // dp) and np.array_equal(d, lane % dp)
            assert np.array_equal(live != 0, base + d < n) and int(live.sum()) == count * (64 // dp)
            k = L.csrgeno_fold_strides(dp, strides.ctypes.data)
            want = [s for s in (1, 2, 4, 8, 16, 32) if s >= dp]
            assert list(strides[:k]) == want, (dp, strides[:k])


def test_every_case_against_the_model(L):
    seen = set()
    for (name, indptr, indices, n_minor, counts, geno, n_donors), want in all_cases():
        assert L.csrgeno_first_bad(ptr(geno), geno.size) == NO_BAD and first_bad_geno(geno) is None, name
        got = tally(L, indptr, indices, counts, geno, n_donors)
        same(got, want)
        seen.add(name)
        alt, ref = (a.astype(np.uint64) for a in counts)
        rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr.astype(np.int64)))
        for k, a in (("sum_alt", alt), ("sum_ref", ref), ("n_obs", ((alt + ref) > 0).astype(np.uint64))):      # every entry lands in one class of every donor
            total = np.zeros(len(indptr) - 1, np.uint64)
            np.add.at(total, rows, a)
            assert np.array_equal(got[k].astype(np.uint64).sum(axis=2), np.repeat(total[:, None], n_donors, axis=1)), (name, k)
        if name == "one_donor_all_missing":
            assert not got["sum_alt"][:, 2, :3].any() and not got["n_obs"][:, 2, :3].any() and got["sum_alt"][:, 2, 3].any()
        if name == "every_class_in_one_row":               # donor 0: variant g has class g; the row holds (3, 1, 0, 2) with alt (5, 0, 7, 1), ref (0, 2, 3, 0)
            assert list(got["sum_alt"][1, 0]) == [7, 0, 1, 5] and list(got["sum_ref"][1, 0]) == [3, 2, 0, 0] and list(got["n_obs"][1, 0]) == [1, 1, 1, 1]
        if name == "entries_without_reads":
            assert not any(got[k].any() for k in NAMES)
        if name.startswith("sums_past_2_32"):
            assert want["sum_alt"].max() > 1 << 32 and want["sum_ref"].max() > 1 << 32
        if name in ("all_rows_empty", "no_variants"):
            assert got["sum_alt"].size > 0 and not any(got[k].any() for k in NAMES)
    assert len(seen) == len(CASES) >= 20 and {"donors_%d" % n for n in DONORS} <= seen


def test_null_outputs_are_skipped(L):
    (name, indptr, indices, n_minor, counts, geno, n_donors), want = all_cases()[5]
    for names in (("sum_alt",), ("sum_ref", "n_obs"), ("n_obs",), ()):
        got = tally(L, indptr, indices, counts, geno, n_donors, names)
        assert set(got) == set(names)
        same(got, want, names)


def test_the_byte_check_names_the_lowest_position(L):
    geno = np.array([[0, 1, 2], [NONE, 2, 0], [1, 1, NONE]], np.uint8)
    assert L.csrgeno_first_bad(geno.ctypes.data, 9) == NO_BAD and first_bad_geno(geno) is None
    geno[2, 0], geno[1, 2] = 3, 254                        # two of them: the lowest flat position
    assert L.csrgeno_first_bad(geno.ctypes.data, 9) == 5 == first_bad_geno(geno)
    geno[1, 2] = 0
    assert L.csrgeno_first_bad(geno.ctypes.data, 9) == 6 == first_bad_geno(geno)
    assert L.csrgeno_first_bad(None, 0) == NO_BAD
    every = np.arange(256, dtype=np.uint8)
    for b in range(256):
        assert (L.csrgeno_first_bad(every[b:].ctypes.data, 1) == NO_BAD) == (b in (0, 1, 2, NONE))


def run_program(name, todo):
    """Cases through tests/csrgenocore/main.cpp in ONE process -> [None for a refused table, else the tally]."""
    subprocess.check_call(["make", "-C", os.path.join(HERE, "csrgenocore"), "-s", name])
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<I", len(todo)))
            for _, indptr, indices, n_minor, counts, geno, n_donors in todo:
                f.write(struct.pack("<IIII", len(indptr) - 1, n_minor, len(indices), n_donors))
                f.write(np.asarray(indptr, "<u8").tobytes())
                for a in (indices, *counts):
                    f.write(np.asarray(a, "<u4").tobytes())
                f.write(np.asarray(geno, np.uint8).tobytes())
        r = subprocess.run([os.path.join(HERE, "csrgenocore", name), src, dst], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        blob = open(dst, "rb").read()
    out, p = [], 0

    def take(dtype, n):
        nonlocal p
        a = np.frombuffer(blob, dtype, n, p)
        p += a.nbytes
        return a
    for _, indptr, _, _, _, _, n_donors in todo:
        if int(take("<u8", 1)[0]) != NO_BAD:
            out.append(None)
            continue
        shape = (len(indptr) - 1, n_donors, 4)
        n = shape[0] * shape[1] * 4
        out.append({k: take("<u4" if k == "n_obs" else "<u8", n).reshape(shape) for k in NAMES})
    assert p == len(blob)
    return out


@pytest.mark.parametrize("name", ["csr_geno_host", "csr_geno_host_san"])
def test_what_the_lanes_touch(name):
    """The walk, the fold and the stores in allocations of exactly the device's sizes — the table exactly n_minor * n_donors bytes, so a
    dead lane that reads is caught — under AddressSanitizer and UBSan in the second build: every case above, and one whose table is
    refused."""
    todo = [c for c, _ in all_cases()]
    bad = list(todo[0])
    bad[5] = bad[5].copy()
    bad[5][17, 0] = 3
    todo.append(tuple(bad))
    got = run_program(name, todo)
    assert got[-1] is None
    for (_, want), g in zip(all_cases(), got):
        same(g, want)
