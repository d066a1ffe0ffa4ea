"""Model of the CSR x integer-table sum (vtx_csr_dense_sum) in Python integers reduced modulo 2^64, and the matrices and tables both the
CPU tests of the core header and the GPU tests of the kernel run.  Nothing here knows the code under test: the one thing read from it is
the constant that says how many entries a lane takes per trip, so that rows on both sides of that step exist."""
import os
import re

import numpy as np

from tests.csr_geno_pair_util import first_pass_subgroups, row_lengths
from tests.csr_geno_util import random_counts, random_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
COLS = [1, 2, 3, 5, 63, 64, 65, 70]        # every kind of Dp; a dead lane in Dp = 4; the pass edge; a pass of 64 and one of 1, of 6
N_MINOR = 37


def unroll():
    """DENSE_UNROLL of vtx_csr_dense_core.h: the entries a lane takes per trip of its walk (1: the walk is not unrolled)."""
    text = open(os.path.join(ROOT, "vartrix_amd", "csrc", "vtx_csr_dense_core.h")).read()
    return int(re.search(r"constexpr uint32_t DENSE_UNROLL = (\d+);", text).group(1))


def model_dense_sum(indptr, indices, alt, ref, w_alt, w_ref, n_cols):
    """Entry by entry in Python integers: count * weight, summed, reduced modulo 2^64 and read as two's complement.  ``w_alt`` /
    ``w_ref``: n_minor x n_cols, or None for an absent term.  -> int64, n_major x n_cols."""
    indptr = [int(x) for x in np.asarray(indptr)]
    n_major = len(indptr) - 1
    tables = [None if w is None else np.asarray(w, np.int32).reshape(-1, n_cols).astype(object) for w in (w_alt, w_ref)]
    out = np.zeros((n_major, n_cols), np.int64)
    for r in range(n_major):
        acc = np.zeros(n_cols, object)
        for k in range(indptr[r], indptr[r + 1]):
            v = int(indices[k])
            for count, table in zip((alt, ref), tables):
                if table is not None:
                    acc = acc + int(count[k]) * table[v]
        for h in range(n_cols):
            x = int(acc[h]) % (1 << 64)
            out[r, h] = x - (1 << 64) if x >= 1 << 63 else x
    return out


def true_sum_fits(indptr, indices, alt, ref, w_alt, w_ref, n_cols):
    """Whether every unreduced sum lies in int64 (the case that pins the wrap must say no)."""
    indptr = [int(x) for x in np.asarray(indptr)]
    tables = [None if w is None else np.asarray(w, np.int32).reshape(-1, n_cols).astype(object) for w in (w_alt, w_ref)]
    for r in range(len(indptr) - 1):
        acc = np.zeros(n_cols, object)
        for k in range(indptr[r], indptr[r + 1]):
            for count, table in zip((alt, ref), tables):
                if table is not None:
                    acc = acc + int(count[k]) * table[int(indices[k])]
        if any(not -(1 << 63) <= int(x) < 1 << 63 for x in acc):
            return False
    return True


def random_weights(rng, n_minor, n_cols):
    """Two tables over the whole int32 range with INT32_MIN, INT32_MAX, 0 and -1 planted in each."""
    out = []
    for _ in range(2):
        w = rng.integers(INT32_MIN, INT32_MAX + 1, (n_minor, n_cols), dtype=np.int64).astype(np.int32)
        flat = w.reshape(-1)
        if len(flat):
            at = rng.integers(0, len(flat), 8)
            flat[at] = np.array([INT32_MIN, INT32_MAX, 0, -1, INT32_MIN, INT32_MAX, 0, -1], np.int32)
        out.append(w)
    return out


def wide_counts(rng, n):
    """alt / ref anywhere in uint32, 2^32 - 1 and 0 included."""
    out = []
    for _ in range(2):
        a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        if n:
            a[rng.integers(0, n, 3)] = 0xFFFFFFFF
            a[rng.integers(0, n, 3)] = 0
        out.append(a)
    return out


def dense_row_lengths(n_cols):
    """csr_geno_pair_util.row_lengths' rows, and both sides of one trip of the unrolled walk (DENSE_UNROLL entries in every sub-group)
    and of two."""
    trip = first_pass_subgroups(n_cols) * unroll()
    return row_lengths(n_cols) + ([trip - 1, trip, trip + 1, 2 * trip - 1, 2 * trip, 2 * trip + 1, 0] if unroll() > 1 else [])


def cases():
    """[(name, indptr, indices, n_minor, (alt, ref), w_alt, w_ref (n_minor x n_cols, int32), n_cols)]: the smallest inputs at which the
    sum can go wrong."""
    rng = np.random.default_rng(2027)
    out = []

    def add(name, indptr, indices, n_minor, n_cols, counts=None, weights=None):
        counts = tuple(random_counts(rng, len(indices))) if counts is None else tuple(counts)
        w_alt, w_ref = random_weights(rng, n_minor, n_cols) if weights is None else weights
        out.append((name, np.asarray(indptr, np.uint64), np.asarray(indices, np.uint32), n_minor, counts,
                    np.ascontiguousarray(w_alt, np.int32).reshape(n_minor, n_cols), np.ascontiguousarray(w_ref, np.int32).reshape(n_minor, n_cols), n_cols))
    for n in COLS:
        indptr, indices = random_rows(rng, dense_row_lengths(n), N_MINOR)
        add("cols_%d" % n, indptr, indices, N_MINOR, n)
    indptr, indices = random_rows(rng, dense_row_lengths(5), N_MINOR)
    add("counts_up_to_2_32", indptr, indices, N_MINOR, 5, counts=wide_counts(rng, len(indices)))
    indptr, indices = random_rows(rng, [0, 90, 3], N_MINOR)
    add("counts_up_to_2_32_two_passes", indptr, indices, N_MINOR, 70, counts=wide_counts(rng, len(indices)))
    # the true sum of the middle row's column 0 is 3 (2^32 - 1) INT32_MIN < -2^63 under w_alt, and twice that under both tables
    full = np.full(3, 0xFFFFFFFF, np.uint32)
    low = np.zeros((3, 2), np.int32)
    low[:, 0], low[:, 1] = INT32_MIN, INT32_MAX
    add("the_true_sum_leaves_int64", [0, 0, 3, 3], [0, 1, 2], 3, 2, counts=(full, full.copy()), weights=(low, low.copy()))
    empty = np.zeros(0, np.uint32)
    add("all_rows_empty", np.zeros(6, np.uint64), empty, 7, 3)
    add("no_rows", np.zeros(1, np.uint64), empty, 7, 5)
    add("no_variants", np.zeros(4, np.uint64), empty, 0, 9)
    add("only_the_first_row", *random_rows(rng, [70, 0, 0, 0, 0], N_MINOR), N_MINOR, 6)
    add("only_the_last_row", *random_rows(rng, [0, 0, 0, 0, 0, 70], N_MINOR), N_MINOR, 6)
    add("a_row_of_one_entry", [0, 1], [N_MINOR - 1], N_MINOR, 4)
    add("one_variant_over_and_over", [0, 1, 1, 80], np.zeros(80, np.uint32), 1, 10)
    for n in (64, 65):                                            # the highest element of the tables: one past it is outside
        last = np.full(5, N_MINOR - 1, np.uint32)
        add("last_variant_last_column_%d" % n, [0, 2, 5], last, N_MINOR, n)
    indptr, indices = random_rows(rng, [9, 0, 130, 3], N_MINOR)
    zeros = np.zeros(len(indices), np.uint32)
    add("entries_without_reads", indptr, indices, N_MINOR, 4, counts=(zeros, zeros.copy()))
    return out


def variants(case):
    """A case as the three calls it makes: both tables, w_alt absent, w_ref absent -> [(tag, w_alt or None, w_ref or None)]."""
    w_alt, w_ref = case[5], case[6]
    return [("both", w_alt, w_ref), ("no_w_alt", None, w_ref), ("no_w_ref", w_alt, None)]


def modelled():
    """Every case with the model's answer to each of its three calls, computed once: [(case, {tag: int64 n_major x n_cols})]."""
    out = []
    for c in cases():
        out.append((c, {tag: model_dense_sum(c[1], c[2], *c[4], wa, wf, c[7]) for tag, wa, wf in variants(c)}))
    return out
