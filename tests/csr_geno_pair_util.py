"""numpy model of the doublet tally (vtx_csr_geno_pair_tally), and the matrices, genotype tables and lists of pairs both the CPU tests of
the core header and the GPU tests of the kernels run.  Nothing here knows the code under test."""
import numpy as np

from tests.csr_geno_util import BYTES, NONE, random_counts, random_rows, random_table

NAMES = ("sum_alt", "sum_ref", "n_obs")
CLASSES = 6                    # the dosage 0 .. 4, and 5: either donor without a call


def first_bad_pair(pairs, n_donors):
    """The lowest index of a pair with a donor that does not exist; None when every pair is fine."""
    bad = np.flatnonzero((np.asarray(pairs, np.int64).reshape(-1, 2) >= n_donors).any(axis=1))
    return int(bad[0]) if len(bad) else None


def model_pair_tally(indptr, indices, alt, ref, geno, n_donors, pairs):
    """Pair by pair: every entry has one class under the pair, and the counts are summed by (row, class) with ``np.bincount``.  The
    weights are float64: every sum here stays below 2^53 (asserted), so they are exact.  -> dict(sum_alt, sum_ref uint64; n_obs
    uint32), each n_major x n_pairs x 6."""
    indptr = np.asarray(indptr).astype(np.int64)
    n_major, pairs = len(indptr) - 1, np.asarray(pairs, np.int64).reshape(-1, 2)
    table = np.asarray(geno, np.uint8).reshape(-1, n_donors).astype(np.int64)
    assert np.isin(table, BYTES).all() and (pairs < n_donors).all() and (pairs >= 0).all()
    cols = np.asarray(indices).astype(np.int64)
    rows = np.repeat(np.arange(n_major), np.diff(indptr))
    a, f = np.asarray(alt).astype(np.int64), np.asarray(ref).astype(np.int64)
    assert int(a.sum()) < 1 << 53 and int(f.sum()) < 1 << 53
    seen = ((a + f) > 0).astype(np.int64)
    out = {k: np.zeros((n_major, len(pairs), CLASSES), np.uint64) for k in NAMES}
    for p, (da, db) in enumerate(pairs):
        ga, gb = table[cols, da], table[cols, db]
        key = rows * CLASSES + np.where((ga == NONE) | (gb == NONE), 5, ga + gb)
        for k, w in (("sum_alt", a), ("sum_ref", f), ("n_obs", seen)):
            out[k][:, p, :] = np.bincount(key, weights=w.astype(np.float64), minlength=n_major * CLASSES).astype(np.uint64).reshape(n_major, CLASSES)
    out["n_obs"] = out["n_obs"].astype(np.uint32)
    return out


PAIRS = [1, 2, 3, 5, 63, 64, 65, 70]        # every kind of Dp; a dead lane in Dp = 4; the pass edge; a pass of 64 and one of 1, of 6
N_MINOR = 37
N_DONORS = 7


def first_pass_subgroups(n_pairs):
    """64 / Dp of the first pass: the number of entries of a row one step of the wavefront takes."""
    count, dp = min(n_pairs, 64), 1
    while dp < count:
        dp *= 2
    return 64 // dp


def row_lengths(n_pairs):
    """Empty first and last rows; 1; both sides of one step of the wavefront; both sides of 64; 200."""
    s = first_pass_subgroups(n_pairs)
    return [0, 1, max(s - 1, 0), s, s + 1, 0, 63, 64, 65, 200, 2, 0]


def random_pairs(rng, n_pairs, n_donors):
    """Any list: both orders, (a, a) and repeats occur by chance among 7 donors; the highest donor occurs on either side."""
    pairs = rng.integers(0, n_donors, (n_pairs, 2), dtype=np.int64).astype(np.uint32)
    pairs[rng.integers(0, n_pairs), 0] = n_donors - 1
    pairs[rng.integers(0, n_pairs), 1] = n_donors - 1
    return pairs


def cases():
    """[(name, indptr, indices, n_minor, (alt, ref), geno (n_minor x n_donors, uint8), n_donors, pairs (n_pairs x 2, uint32))]: the
    smallest inputs at which the tally can go wrong."""
    rng = np.random.default_rng(2026)
    out = []

    def add(name, indptr, indices, n_minor, geno, n_donors, pairs, big=False, counts=None):
        counts = tuple(random_counts(rng, len(indices), big)) if counts is None else counts
        out.append((name, np.asarray(indptr, np.uint64), np.asarray(indices, np.uint32), n_minor, counts,
                    np.ascontiguousarray(geno, np.uint8).reshape(n_minor, n_donors), n_donors,
                    np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)))
    for n in PAIRS:
        indptr, indices = random_rows(rng, row_lengths(n), N_MINOR)
        add("pairs_%d" % n, indptr, indices, N_MINOR, random_table(rng, N_MINOR, N_DONORS), N_DONORS, random_pairs(rng, n, N_DONORS))
    empty = np.zeros(0, np.uint32)
    add("one_donor_with_itself", *random_rows(rng, row_lengths(1), N_MINOR), N_MINOR, random_table(rng, N_MINOR, 1), 1, [[0, 0]])
    add("all_rows_empty", np.zeros(6, np.uint64), empty, 7, random_table(rng, 7, 3), 3, [[0, 1], [1, 2], [2, 0]])
    add("no_rows", np.zeros(1, np.uint64), empty, 7, random_table(rng, 7, 5), 5, random_pairs(rng, 4, 5))
    add("no_variants", np.zeros(4, np.uint64), empty, 0, np.zeros((0, 9), np.uint8), 9, random_pairs(rng, 9, 9))
    add("only_the_first_row", *random_rows(rng, [70, 0, 0, 0, 0], N_MINOR), N_MINOR, random_table(rng, N_MINOR, 6), 6, random_pairs(rng, 6, 6))
    add("only_the_last_row", *random_rows(rng, [0, 0, 0, 0, 0, 70], N_MINOR), N_MINOR, random_table(rng, N_MINOR, 6), 6, random_pairs(rng, 6, 6))
    add("a_row_of_one_entry", [0, 1], [N_MINOR - 1], N_MINOR, random_table(rng, N_MINOR, 4), 4, [[0, 1], [2, 3], [3, 3]])
    add("rows_shorter_than_the_sub_groups", *random_rows(rng, [3, 0, 7, 1], N_MINOR), N_MINOR, random_table(rng, N_MINOR, 4), 4,
        [[0, 1], [2, 3]])                                         # Dp = 2: 32 sub-groups
    add("one_variant_over_and_over", [0, 1, 1, 80], np.zeros(80, np.uint32), 1, random_table(rng, 1, 5), 5, random_pairs(rng, 10, 5))
    indptr, indices = random_rows(rng, [9, 0, 130, 3], N_MINOR)
    zeros = np.zeros(len(indices), np.uint32)
    add("entries_without_reads", indptr, indices, N_MINOR, random_table(rng, N_MINOR, 4), 4, random_pairs(rng, 5, 4), counts=(zeros, zeros.copy()))
    add("same_donor_both_orders_and_repeats", *random_rows(rng, row_lengths(6), N_MINOR), N_MINOR, random_table(rng, N_MINOR, 5), 5,
        [[2, 2], [1, 3], [3, 1], [1, 3], [0, 0], [4, 2]])
    table = random_table(rng, N_MINOR, 5)
    table[:, 2] = NONE
    add("one_donor_all_missing", *random_rows(rng, row_lengths(5), N_MINOR), N_MINOR, table, 5, [[0, 2], [2, 2], [2, 4], [1, 3], [3, 0]])
    table = BYTES[rng.integers(0, 3, (N_MINOR, 6))]
    add("no_missing_byte", *random_rows(rng, row_lengths(9), N_MINOR), N_MINOR, table, 6, random_pairs(rng, 9, 6))
    # two entries of 2^32 - 1 in one class: the variants 0 and 1 are het in donor 0 and hom-alt in donor 1 (dosage 3), variant 2 is not
    table = np.array([[1, 2, 0], [1, 2, NONE], [0, 0, 2]], np.uint8)
    full = np.full(3, 0xFFFFFFFF, np.uint32)
    add("sums_past_2_32", [0, 0, 3], [0, 1, 2], 3, table, 3, [[0, 1], [1, 0], [0, 2], [2, 2]], counts=(full, full.copy()))
    add("sums_past_2_32_two_passes", *random_rows(rng, [0, 90, 3], N_MINOR), N_MINOR, random_table(rng, N_MINOR, N_DONORS), N_DONORS,
        random_pairs(rng, 70, N_DONORS), big=True)
    for n in (64, 65):                                            # the highest byte of the table, under the last pair of a pass
        last = np.full(5, N_MINOR - 1, np.uint32)
        pairs = random_pairs(rng, n, N_DONORS)
        pairs[-1] = N_DONORS - 1
        add("last_variant_last_donor_%d" % n, [0, 2, 5], last, N_MINOR, random_table(rng, N_MINOR, N_DONORS), N_DONORS, pairs)
    return out
