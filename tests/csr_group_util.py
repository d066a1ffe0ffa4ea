"""numpy model of the pseudobulk fold (vtx_csr_group_plan / vtx_csr_group_sum), and the matrices and labels both the CPU tests of the
core header and the GPU tests of the kernels run.  Nothing here knows the code under test."""
import numpy as np

from tests.csr_ops_util import COUNTS, SUMS, csr_with_row_lengths

NONE = 0xFFFFFFFF              # VTX_GROUP_NONE
NAMES = COUNTS + SUMS


def first_bad_label(group, n_groups):
    """The lowest column whose label is neither a group nor NONE; None when every label is fine."""
    group = np.asarray(group, np.uint32)
    bad = np.flatnonzero((group >= n_groups) & (group != NONE))
    return int(bad[0]) if len(bad) else None


def model_group_sum(indptr, indices, alt, ref, unk, group, n_groups):
    """Sort the kept entries by (row, group), cut where the pair changes, ``add.reduceat`` in uint64 (exact).
    -> dict(indptr uint64, indices uint32, the four counts uint32, the three sums uint64)."""
    indptr = np.asarray(indptr).astype(np.int64)
    n_major = len(indptr) - 1
    rows = np.repeat(np.arange(n_major, dtype=np.int64), np.diff(indptr))
    label = np.asarray(group, np.uint32)[np.asarray(indices).astype(np.int64)] if len(rows) else np.zeros(0, np.uint32)
    keep = label != NONE
    key = rows[keep] * np.int64(n_groups) + label[keep].astype(np.int64)
    order = np.argsort(key, kind="stable")
    key = key[order]
    starts = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if len(key) else np.zeros(0, np.int64)
    out_rows = key[starts] // n_groups
    alt, ref, unk = (np.asarray(a)[keep][order] for a in (alt, ref, unk))

    def total(a):
        return np.add.reduceat(a.astype(np.uint64), starts) if len(starts) else np.zeros(0, np.uint64)
    out = {"indptr": np.searchsorted(out_rows, np.arange(n_major + 1), side="left").astype(np.uint64),
           "indices": (key[starts] % n_groups).astype(np.uint32),
           "n_entries": total(np.ones(len(key))).astype(np.uint32), "n_alt": total(alt > 0).astype(np.uint32),
           "n_ref": total(ref > 0).astype(np.uint32), "n_both": total((alt > 0) & (ref > 0)).astype(np.uint32),
           "sum_alt": total(alt), "sum_ref": total(ref), "sum_unk": total(unk)}
    return out


# the stride loop on both sides of 64; empty rows in the middle and at both ends; one row that holds EVERY column (labels_straddling)
ROW_LENGTHS = [0, 1, 63, 64, 65, 257, 0, 0, 300, 64, 2, 0]
N_MINOR = 300


def matrix(rng, lens=ROW_LENGTHS, n_minor=N_MINOR, sort=True):
    return csr_with_row_lengths(rng, lens, n_minor, sort=sort)


def labels_straddling(rng, n_minor, n_groups, window):
    """Random labels over all the groups, but the first columns carry, in this order: the last group of every window and the first of
    the next one, the last group of all, group 0 — so that a row that holds those columns has entries on both sides of every window
    edge and of every 64-bin step."""
    group = rng.integers(0, n_groups, n_minor, dtype=np.uint64).astype(np.uint32)
    edges = [g for e in range(64, n_groups, 64) for g in (e - 1, e)] + [n_groups - 1, 0]
    edges = [g for g in edges if g < n_groups][:n_minor]
    group[:len(edges)] = edges
    return group


def group_counts(window):
    """n_groups on both sides of a sweep step, of the window, and past two windows."""
    return [1, 2, 63, 64, 65, window - 1, window, window + 1, 2 * window + 1]


def cases(window):
    """[(name, indptr, indices, n_minor, (alt, ref, unk), group, n_groups)]: the smallest matrices at which the fold can go wrong."""
    from tests.csr_ops_util import random_counts
    rng = np.random.default_rng(2024)
    out = []

    def add(name, indptr, indices, n_minor, group, n_groups, big=False):
        out.append((name, indptr, indices, n_minor, tuple(random_counts(rng, len(indices), big)), np.asarray(group, np.uint32), n_groups))
    indptr, indices = matrix(rng)
    for n_groups in group_counts(window):
        add("groups_%d" % n_groups, indptr, indices, N_MINOR, labels_straddling(rng, N_MINOR, n_groups, window), n_groups)
    add("no_entries", np.zeros(6, np.uint64), np.zeros(0, np.uint32), 7, rng.integers(0, 3, 7), 3)
    one_ptr, one_idx = matrix(rng, [130], 200)
    add("one_row", one_ptr, one_idx, 200, rng.integers(0, 70, 200), 70)
    add("descending_in_one_window", indptr, indices, N_MINOR, (N_MINOR - 1 - np.arange(N_MINOR)) // 2, N_MINOR // 2)
    add("descending_over_windows", indptr, indices, N_MINOR, N_MINOR - 1 - np.arange(N_MINOR), N_MINOR)
    add("a_group_without_cells", indptr, indices, N_MINOR, np.array([0, 2, 3])[rng.integers(0, 3, N_MINOR)], 5)
    add("every_cell_left_out", indptr, indices, N_MINOR, np.full(N_MINOR, NONE), 4)
    half = rng.integers(0, 9, N_MINOR, dtype=np.uint64).astype(np.uint32)
    half[rng.random(N_MINOR) < 0.5] = NONE
    add("half_the_cells_left_out", indptr, indices, N_MINOR, half, 9)
    add("identity", indptr, indices, N_MINOR, np.arange(N_MINOR), N_MINOR)
    lens = [4, 0, 700, 7, 1, 70]                                # a row longer than n_minor: duplicates; nothing sorted
    dup_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    dup_idx = rng.integers(0, 40, int(dup_ptr[-1]), dtype=np.uint64).astype(np.uint32)
    add("duplicates_unsorted", dup_ptr, dup_idx, 40, rng.integers(0, 6, 40), 6)
    uns_ptr, uns_idx = matrix(rng, sort=False)
    add("unsorted_rows", uns_ptr, uns_idx, N_MINOR, rng.integers(0, window + 9, N_MINOR), window + 9)
    add("sums_past_2_32", indptr, indices, N_MINOR, rng.integers(0, 3, N_MINOR), 3, big=True)
    return out


FIELDS = {"alt_counts": "sum_alt", "ref_counts": "sum_ref", "unknown_counts": "sum_unk", "n_cells": "n_entries", "n_alt_cells": "n_alt",
          "n_ref_cells": "n_ref", "n_both_cells": "n_both"}      # GroupResult's names for the seven numbers


def model_pseudobulk(alt, ref, unk, labels, n_groups):
    """The fold of three variant-major scipy CSR matrices of one sparsity as DENSE int64 arrays (variants x groups), by GroupResult's names."""
    alt, ref, unk = (m.tocsr() for m in (alt, ref, unk))
    assert np.array_equal(alt.indptr, ref.indptr) and np.array_equal(alt.indices, ref.indices) and np.array_equal(alt.indices, unk.indices)
    m = model_group_sum(alt.indptr, alt.indices, alt.data, ref.data, unk.data, labels, max(n_groups, 1))
    rows = np.repeat(np.arange(alt.shape[0]), np.diff(m["indptr"].astype(np.int64)))
    out = {}
    for field, k in FIELDS.items():
        d = np.zeros((alt.shape[0], n_groups), np.int64)
        d[rows, m["indices"].astype(np.int64)] = m[k].astype(np.int64)
        out[field] = d
    return out


def dense(m):
    """A scipy matrix or a torch sparse CSR tensor as a dense int64 numpy array."""
    if hasattr(m, "toarray"):
        return np.asarray(m.toarray()).astype(np.int64)
    return m.to_dense().cpu().numpy().astype(np.int64)
