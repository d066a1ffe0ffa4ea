"""vtx_csr_dense_core.h on the CPU: what one lane of the CSR x integer-table kernel (vartrix_amd/csrc/vtx_csr_dense.hip) does alone —
the product of a count and a weight into the wrapping 64-bit sum, the place of a weight in a table and of a sum in the output, the
lane's walk over its share of a row — compiled for the host by tests/csrdensecore/Makefile with the lanes as loops and the exchange
between lanes as array reads, against the model in Python integers of tests/csr_dense_util.py.  The device runs the same source
(tests/test_gpu_csr_dense.py).  What the lanes TOUCH is checked by a stand-alone program (tests/csrdensecore/main.cpp) in allocations of
exactly the device's sizes, plain and under AddressSanitizer and UBSan; nothing sanitized is loaded into Python."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from tests.csr_dense_util import COLS, INT32_MAX, INT32_MIN, dense_row_lengths, modelled, true_sum_fits, unroll, variants
from tests.csr_geno_pair_util import first_pass_subgroups

HERE = os.path.dirname(os.path.abspath(__file__))
P64 = -0x5A5A5A5A5A5A5A5B                                  # 0xA5A5A5A5A5A5A5A5 as int64


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "csrdensecore"), "-s"])
    lib = C.CDLL(os.path.join(HERE, "csrdensecore", "libcsrdense_host.so"))
    for f in (lib.csrdense_max, lib.csrdense_unroll):
        f.restype, f.argtypes = C.c_uint32, []
    lib.csrdense_mul.restype = C.c_uint64
    lib.csrdense_mul.argtypes = [C.c_uint32, C.c_int32]
    lib.csrdense_table_index.restype = C.c_uint64
    lib.csrdense_table_index.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    lib.csrdense_out_index.restype = C.c_uint64
    lib.csrdense_out_index.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
    lib.csrdense_sum.restype = None
    lib.csrdense_sum.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_void_p]
    return lib


def ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def dense_sum(L, indptr, indices, counts, w_alt, w_ref, n_cols):
    n_major = len(indptr) - 1
    out = np.full((n_major, n_cols), P64, np.int64)
    stores = np.zeros((n_major, n_cols), np.uint8)
    L.csrdense_sum(indptr.ctypes.data, n_major, ptr(indices), *[ptr(a) for a in counts], ptr(w_alt), ptr(w_ref), n_cols, ptr(out), ptr(stores))
    assert np.all(stores == 1)                             # every output element stored exactly once, by one lane
    return out


CASES = None


def all_cases():
    global CASES
    if CASES is None:
        CASES = modelled()
    return CASES


def test_constants_and_the_header_the_cases_are_derived_from(L):
    """At most 16 passes of 64 columns; the cases take the trip of the walk from the header's own constant."""
    assert L.csrdense_max() == 64 * 16 and L.csrdense_unroll() == unroll() >= 1
    for n in COLS:
        trip = first_pass_subgroups(n) * unroll()
        assert unroll() == 1 or {trip - 1, trip, trip + 1} <= set(dense_row_lengths(n))


def test_the_product_wraps_as_the_contract_says(L):
    """The count zero-extended, the weight sign-extended, modulo 2^64."""
    for count in (0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF):
        for w in (INT32_MIN, INT32_MIN + 1, -2, -1, 0, 1, 2, INT32_MAX):
            assert L.csrdense_mul(count, w) == (count * w) % (1 << 64), (count, w)


def test_the_places_of_a_weight_and_of_a_sum(L):
    """64-bit: the last element of the largest table and of an output of 2^32 - 1 rows."""
    assert L.csrdense_table_index(36, 70, 69) == 36 * 70 + 69
    assert L.csrdense_table_index(0xFFFFFFFE, 1024, 1023) == 0xFFFFFFFE * 1024 + 1023
    assert L.csrdense_out_index(0xFFFFFFFE, 1024, 1023) == 0xFFFFFFFE * 1024 + 1023
    assert L.csrdense_out_index(0, 5, 0) == 0 and L.csrdense_out_index(3, 5, 4) == 19


def test_every_case_and_its_null_table_variants_against_the_model(L):
    seen = set()
    for case, want in all_cases():
        name, indptr, indices, n_minor, counts, w_alt, w_ref, n_cols = case
        for tag, wa, wf in variants(case):
            if n_minor == 0 and tag != "both":
                continue                                   # no table has an element: one call
            got = dense_sum(L, indptr, indices, counts, wa, wf, n_cols)
            assert got.dtype == want[tag].dtype and np.array_equal(got, want[tag]), (name, tag)
        if n_minor:                                        # the two single-table sums add up to the sum with both, modulo 2^64
            both = (want["no_w_alt"].view(np.uint64) + want["no_w_ref"].view(np.uint64)).view(np.int64)
            assert np.array_equal(both, want["both"]), name
        seen.add(name)
        if name == "the_true_sum_leaves_int64":            # 3 (2^32 - 1) INT32_MIN = -(3 * 2^63) + 3 * 2^31 wraps to 2^63 + 3 * 2^31
            assert not true_sum_fits(indptr, indices, *counts, w_alt, None, n_cols)
            assert int(want["no_w_ref"][1, 0]) == (3 * 0xFFFFFFFF * INT32_MIN) % (1 << 64) - (1 << 64) == -(1 << 63) + 3 * (1 << 31)
            assert int(want["both"][1, 0]) == 3 * (1 << 32)
        if name == "entries_without_reads":
            assert not want["both"].any()
        if name in ("all_rows_empty", "no_variants"):
            assert want["both"].size > 0 and not want["both"].any()
        if name.startswith("counts_up_to_2_32"):
            assert max(int(c.max()) for c in counts) == 0xFFFFFFFF
    assert len(seen) == len(CASES) >= 20 and {"cols_%d" % n for n in COLS} <= seen


def test_the_planted_weights_are_there():
    for case, _ in all_cases():
        if case[0].startswith("cols_") and case[7] >= 2:
            for w in case[5:7]:
                assert {INT32_MIN, INT32_MAX, 0, -1} <= set(int(x) for x in w.reshape(-1)), case[0]


def run_program(name, todo):
    """Calls through tests/csrdensecore/main.cpp in ONE process -> the sums.  todo: [(indptr, indices, n_minor, counts, w_alt, w_ref, n_cols)]"""
    subprocess.check_call(["make", "-C", os.path.join(HERE, "csrdensecore"), "-s", name])
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<I", len(todo)))
            for indptr, indices, n_minor, counts, w_alt, w_ref, n_cols in todo:
                f.write(struct.pack("<IIIIII", len(indptr) - 1, n_minor, len(indices), n_cols, w_alt is not None, w_ref is not None))
                f.write(np.asarray(indptr, "<u8").tobytes())
                for a in (indices, *counts):
                    f.write(np.asarray(a, "<u4").tobytes())
                for w in (w_alt, w_ref):
                    if w is not None:
                        f.write(np.asarray(w, "<i4").tobytes())
        r = subprocess.run([os.path.join(HERE, "csrdensecore", name), src, dst], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        blob = open(dst, "rb").read()
    out, p = [], 0
    for indptr, _, _, _, _, _, n_cols in todo:
        shape = (len(indptr) - 1, n_cols)
        a = np.frombuffer(blob, "<i8", shape[0] * shape[1], p).reshape(shape)
        p += a.nbytes
        out.append(a)
    assert p == len(blob)
    return out


@pytest.mark.parametrize("name", ["csr_dense_host", "csr_dense_host_san"])
def test_what_the_lanes_touch(name):
    """The walk, its unrolled trips, the fold and the stores in allocations of exactly the device's sizes — a table exactly n_minor *
    n_cols words, an absent table no allocation at all — under AddressSanitizer and UBSan in the second build: every case above with
    both tables, without w_alt and without w_ref."""
    todo, wants = [], []
    for case, want in all_cases():
        name_, indptr, indices, n_minor, counts, w_alt, w_ref, n_cols = case
        for tag, wa, wf in variants(case):
            if n_minor == 0 and tag != "both":
                continue
            todo.append((indptr, indices, n_minor, counts, wa, wf, n_cols))
            wants.append((name_, tag, want[tag]))
    got = run_program(name, todo)
    assert len(got) == len(wants) >= 60
    for g, (name_, tag, want) in zip(got, wants):
        assert np.array_equal(g, want), (name_, tag)
