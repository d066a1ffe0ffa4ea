"""vtx_csr_geno_pair_core.h on the CPU: what one lane of the doublet tally kernel (vartrix_amd/csrc/vtx_csr_geno.hip) does alone —
the check of a pair, the class of an entry under a pair, an entry's contribution by predicated additions, the fold over the sub-groups,
the place of a number in the output — compiled for the host by tests/csrgenopaircore/Makefile with the lanes as loops and the exchange
between lanes as array reads, against the numpy model of tests/csr_geno_pair_util.py.  The device runs the same source
(tests/test_gpu_csr_geno_pair.py).  What the lanes TOUCH is checked by a stand-alone program (tests/csrgenopaircore/main.cpp) in
allocations of exactly the device's sizes, plain and under AddressSanitizer and UBSan; nothing sanitized is loaded into Python."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from tests.csr_geno_pair_util import CLASSES, NAMES, PAIRS, cases, first_bad_pair, model_pair_tally
from tests.csr_geno_util import NONE, model_geno_tally

HERE = os.path.dirname(os.path.abspath(__file__))
P32, P64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
NO_BAD = (1 << 64) - 1


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "csrgenopaircore"), "-s"])
    lib = C.CDLL(os.path.join(HERE, "csrgenopaircore", "libcsrgenopair_host.so"))
    for f in (lib.csrgenopair_max, lib.csrgenopair_classes, lib.csrgenopair_tally_bytes):
        f.restype, f.argtypes = C.c_uint32, []
    lib.csrgenopair_class.restype = C.c_uint32
    lib.csrgenopair_class.argtypes = [C.c_uint8, C.c_uint8]
    lib.csrgenopair_first_bad.restype = C.c_uint64
    lib.csrgenopair_first_bad.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    lib.csrgenopair_tally.restype = None
    lib.csrgenopair_tally.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 4
    return lib


def ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def tally(L, indptr, indices, counts, geno, n_donors, pairs, names=NAMES):
    n_major = len(indptr) - 1
    shape = (n_major, len(pairs), CLASSES)
    out = {k: np.full(shape, P32, np.uint32) if k == "n_obs" else np.full(shape, P64, np.uint64) for k in names}
    stores = np.zeros(shape, np.uint8)
    L.csrgenopair_tally(indptr.ctypes.data, n_major, ptr(indices), *[ptr(a) for a in counts], ptr(geno), n_donors, pairs.ctypes.data, len(pairs),
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
        CASES = [(c, model_pair_tally(c[1], c[2], *c[4], c[5], c[6], c[7])) for c in cases()]
    return CASES


def test_constants(L):
    """At most 64 passes of 64 pairs; six classes; eighteen numbers a lane: twelve of 64 bits and six of 32."""
    assert L.csrgenopair_max() == 64 * 64 and L.csrgenopair_classes() == CLASSES == 6 and L.csrgenopair_tally_bytes() == 12 * 8 + 6 * 4


def test_the_class_of_an_entry(L):
    """The dosage when both donors have a call, 5 when either has none."""
    for ga in (0, 1, 2, NONE):
        for gb in (0, 1, 2, NONE):
            assert L.csrgenopair_class(ga, gb) == (5 if NONE in (ga, gb) else ga + gb)


def test_every_case_against_the_model(L):
    seen = set()
    for (name, indptr, indices, n_minor, counts, geno, n_donors, pairs), want in all_cases():
        assert L.csrgenopair_first_bad(pairs.ctypes.data, len(pairs), n_donors) == NO_BAD and first_bad_pair(pairs, n_donors) is None, name
        got = tally(L, indptr, indices, counts, geno, n_donors, pairs)
        same(got, want)
        seen.add(name)
        alt, ref = (a.astype(np.uint64) for a in counts)
        rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr.astype(np.int64)))
        for k, a in (("sum_alt", alt), ("sum_ref", ref), ("n_obs", ((alt + ref) > 0).astype(np.uint64))):      # every entry lands in one class of every pair
            total = np.zeros(len(indptr) - 1, np.uint64)
            np.add.at(total, rows, a)
            assert np.array_equal(got[k].astype(np.uint64).sum(axis=2), np.repeat(total[:, None], len(pairs), axis=1)), (name, k)
        one = None
        for p, (a, b) in enumerate(pairs):
            if a == b:                                     # donor a's one-donor tally on the classes 0, 2, 4, its missing class on 5
                one = one or model_geno_tally(indptr, indices, *counts, geno, n_donors)
                for k in NAMES:
                    assert np.array_equal(got[k][:, p, [0, 2, 4, 5]], one[k][:, a, :]) and not got[k][:, p, [1, 3]].any(), (name, p, k)
            for q in range(p):
                if (pairs[q][0], pairs[q][1]) in ((a, b), (b, a)):      # the order inside a pair and a repeat change nothing
                    assert all(np.array_equal(got[k][:, p], got[k][:, q]) for k in NAMES), (name, p, q)
        if name == "one_donor_all_missing":                # pairs 0 - 2 hold donor 2
            assert not got["sum_alt"][:, :3, :5].any() and not got["n_obs"][:, :3, :5].any() and got["sum_alt"][:, :3, 5].any()
        if name == "no_missing_byte":
            assert not any(got[k][:, :, 5].any() for k in NAMES) and got["sum_alt"].any()
        if name == "entries_without_reads":
            assert not any(got[k].any() for k in NAMES)
        if name == "sums_past_2_32":                       # the variants 0 and 1: dosage 3 under (0, 1) and (1, 0)
            for p in (0, 1):
                assert got["sum_alt"][1, p, 3] == got["sum_ref"][1, p, 3] == 2 * 0xFFFFFFFF and got["n_obs"][1, p, 3] == 2
        if name.startswith("sums_past_2_32"):
            assert want["sum_alt"].max() > 1 << 32 and want["sum_ref"].max() > 1 << 32
        if name in ("all_rows_empty", "no_variants"):
            assert got["sum_alt"].size > 0 and not any(got[k].any() for k in NAMES)
    assert len(seen) == len(CASES) >= 20 and {"pairs_%d" % n for n in PAIRS} <= seen


def test_null_outputs_are_skipped(L):
    (name, indptr, indices, n_minor, counts, geno, n_donors, pairs), want = all_cases()[3]
    for names in (("sum_alt",), ("sum_ref", "n_obs"), ("n_obs",), ()):
        got = tally(L, indptr, indices, counts, geno, n_donors, pairs, names)
        assert set(got) == set(names)
        same(got, want, names)


def test_the_pair_check_names_the_lowest_pair(L):
    pairs = np.array([[0, 1], [2, 2], [1, 0], [2, 1]], np.uint32)
    assert L.csrgenopair_first_bad(pairs.ctypes.data, 4, 3) == NO_BAD and first_bad_pair(pairs, 3) is None
    pairs[3, 0], pairs[1, 1] = 3, 0xFFFFFFFF               # two of them, in either slot: the lowest index
    assert L.csrgenopair_first_bad(pairs.ctypes.data, 4, 3) == 1 == first_bad_pair(pairs, 3)
    pairs[1, 1] = 2
    assert L.csrgenopair_first_bad(pairs.ctypes.data, 4, 3) == 3 == first_bad_pair(pairs, 3)
    assert L.csrgenopair_first_bad(pairs.ctypes.data, 3, 3) == NO_BAD      # inside the given length only
    assert L.csrgenopair_first_bad(None, 0, 3) == NO_BAD
    assert L.csrgenopair_first_bad(pairs.ctypes.data, 4, 2) == 1           # fewer donors: (2, 2)


def run_program(name, todo):
    """Cases through tests/csrgenopaircore/main.cpp in ONE process -> [None for a refused table or list, else the tally]."""
    subprocess.check_call(["make", "-C", os.path.join(HERE, "csrgenopaircore"), "-s", name])
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<I", len(todo)))
            for _, indptr, indices, n_minor, counts, geno, n_donors, pairs in todo:
                f.write(struct.pack("<IIIII", len(indptr) - 1, n_minor, len(indices), n_donors, len(pairs)))
                f.write(np.asarray(indptr, "<u8").tobytes())
                for a in (indices, *counts):
                    f.write(np.asarray(a, "<u4").tobytes())
                f.write(np.asarray(geno, np.uint8).tobytes())
                f.write(np.asarray(pairs, "<u4").tobytes())
        r = subprocess.run([os.path.join(HERE, "csrgenopaircore", name), src, dst], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        blob = open(dst, "rb").read()
    out, p = [], 0

    def take(dtype, n):
        nonlocal p
        a = np.frombuffer(blob, dtype, n, p)
        p += a.nbytes
        return a
    for _, indptr, _, _, _, _, _, pairs in todo:
        flags = take("<u8", 2)
        if int(flags[0]) != NO_BAD or int(flags[1]) != NO_BAD:
            out.append(None)
            continue
        shape = (len(indptr) - 1, len(pairs), CLASSES)
        n = shape[0] * shape[1] * CLASSES
        out.append({k: take("<u4" if k == "n_obs" else "<u8", n).reshape(shape) for k in NAMES})
    assert p == len(blob)
    return out


@pytest.mark.parametrize("name", ["csr_geno_pair_host", "csr_geno_pair_host_san"])
def test_what_the_lanes_touch(name):
    """The walk, the fold and the stores in allocations of exactly the device's sizes — the table exactly n_minor * n_donors bytes, the
    pairs exactly 2 * n_pairs words, so a dead lane that reads is caught — under AddressSanitizer and UBSan in the second build: every
    case above, one whose table is refused and one whose list is."""
    todo = [c for c, _ in all_cases()]
    bad = list(todo[0])
    bad[5] = bad[5].copy()
    bad[5][17, 0] = 3
    todo.append(tuple(bad))
    bad = list(todo[2])
    bad[7] = bad[7].copy()
    bad[7][1, 1] = bad[6]
    todo.append(tuple(bad))
    got = run_program(name, todo)
    assert got[-1] is None and got[-2] is None
    for (_, want), g in zip(all_cases(), got):
        same(g, want)
