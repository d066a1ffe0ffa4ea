"""numpy model of the donor tally (vtx_csr_geno_tally), and the matrices and genotype tables both the CPU tests of the core header and
the GPU tests of the kernels run.  Nothing here knows the code under test."""
import numpy as np

from tests.csr_ops_util import csr_with_row_lengths

NONE = 0xFF                    # VTX_GENO_NONE
NAMES = ("sum_alt", "sum_ref", "n_obs")
BYTES = np.array([0, 1, 2, NONE], np.uint8)      # the byte of class 0, 1, 2, 3


def first_bad_geno(geno):
    """The lowest flat position of a byte that is neither 0, 1, 2 nor NONE; None when every byte is fine."""
    flat = np.asarray(geno, np.uint8).reshape(-1)
    bad = np.flatnonzero(~np.isin(flat, BYTES))
    return int(bad[0]) if len(bad) else None


def model_geno_tally(indptr, indices, alt, ref, geno, n_donors):
    """Entry by entry: the entry's counts go, for every donor, to the class of the donor's byte at the entry's variant (``np.add.at``
    in uint64: exact).  -> dict(sum_alt, sum_ref uint64; n_obs uint32), each n_major x n_donors x 4."""
    indptr = np.asarray(indptr).astype(np.int64)
    n_major = len(indptr) - 1
    table = np.asarray(geno, np.uint8).reshape(-1, n_donors)
    cls = np.full(256, -1, np.int64)
    cls[BYTES] = np.arange(4)
    donors = np.arange(n_donors)
    out = {"sum_alt": np.zeros((n_major, n_donors, 4), np.uint64), "sum_ref": np.zeros((n_major, n_donors, 4), np.uint64),
           "n_obs": np.zeros((n_major, n_donors, 4), np.uint64)}
    for r in range(n_major):
        for k in range(indptr[r], indptr[r + 1]):
            g = cls[table[int(indices[k])]]
            assert np.all(g >= 0)
            a, f = np.uint64(alt[k]), np.uint64(ref[k])
            np.add.at(out["sum_alt"], (r, donors, g), a)
            np.add.at(out["sum_ref"], (r, donors, g), f)
            np.add.at(out["n_obs"], (r, donors, g), np.uint64(int(a) + int(f) > 0))
    out["n_obs"] = out["n_obs"].astype(np.uint32)
    return out


DONORS = [1, 2, 3, 5, 8, 33, 63, 64, 65, 129]      # every Dp; idle lanes inside a sub-group; the pass edge; a short last pass
N_MINOR = 37


def first_pass_subgroups(n_donors):
    """64 / Dp of the first pass: the number of entries of a row one step of the wavefront takes."""
    count, dp = min(n_donors, 64), 1
    while dp < count:
        dp *= 2
    return 64 // dp


def row_lengths(n_donors):
    """Empty first and last rows; 1; both sides of one step of the wavefront; both sides of 64; a few hundred."""
    s = first_pass_subgroups(n_donors)
    return [0, 1, max(s - 1, 0), s, s + 1, 0, 63, 64, 65, 300, 2, 0]


def random_rows(rng, lens, n_minor):
    """A CSR whose row r has lens[r] entries with random columns: duplicates inside a row, nothing sorted; the last column occurs."""
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    indices = rng.integers(0, n_minor, int(indptr[-1]), dtype=np.uint64).astype(np.uint32)
    if len(indices):
        indices[rng.integers(0, len(indices), 3)] = n_minor - 1
    return indptr, indices


def random_table(rng, n_minor, n_donors):
    return BYTES[rng.choice(4, (n_minor, n_donors), p=[0.35, 0.3, 0.2, 0.15])]


def random_counts(rng, n, big=False):
    """alt / ref with zeros in every combination (both zero: an entry that counts nowhere); ``big``: 2^32 - 1 wherever not zero."""
    out = []
    for _ in range(2):
        a = np.full(n, 0xFFFFFFFF, np.uint32) if big else rng.integers(1, 50, n, dtype=np.uint64).astype(np.uint32)
        a[rng.random(n) < 0.4] = 0
        out.append(a)
    return out


def cases():
    """[(name, indptr, indices, n_minor, (alt, ref), geno (n_minor x n_donors, uint8), n_donors)]: the smallest inputs at which the
    tally can go wrong."""
    rng = np.random.default_rng(2025)
    out = []

    def add(name, indptr, indices, n_minor, geno, n_donors, big=False, counts=None):
        counts = tuple(random_counts(rng, len(indices), big)) if counts is None else counts
        out.append((name, np.asarray(indptr, np.uint64), np.asarray(indices, np.uint32), n_minor, counts,
                    np.ascontiguousarray(geno, np.uint8).reshape(n_minor, n_donors), n_donors))
    for n in DONORS:
        indptr, indices = random_rows(rng, row_lengths(n), N_MINOR)
        add("donors_%d" % n, indptr, indices, N_MINOR, random_table(rng, N_MINOR, n), n)
    empty = np.zeros(0, np.uint32)
    add("all_rows_empty", np.zeros(6, np.uint64), empty, 7, random_table(rng, 7, 3), 3)
    add("no_rows", np.zeros(1, np.uint64), empty, 7, random_table(rng, 7, 5), 5)
    add("no_variants", np.zeros(4, np.uint64), empty, 0, np.zeros((0, 9), np.uint8), 9)
    add("only_the_first_row", *random_rows(rng, [70, 0, 0, 0, 0], N_MINOR), N_MINOR, random_table(rng, N_MINOR, 6), 6)
    add("only_the_last_row", *random_rows(rng, [0, 0, 0, 0, 0, 70], N_MINOR), N_MINOR, random_table(rng, N_MINOR, 6), 6)
    indptr, indices = random_rows(rng, row_lengths(5), N_MINOR)
    table = random_table(rng, N_MINOR, 5)
    table[:, 2] = NONE
    add("one_donor_all_missing", indptr, indices, N_MINOR, table, 5)
    table = random_table(rng, N_MINOR, 12)
    table[[0, 5, N_MINOR - 1], :] = NONE
    add("variants_all_missing", *random_rows(rng, row_lengths(12), N_MINOR), N_MINOR, table, 12)
    table = random_table(rng, 8, 3)
    table[:4, 0] = BYTES                                          # donor 0 has every class among the variants 0 .. 3 ...
    add("every_class_in_one_row", [0, 0, 4, 4], [3, 1, 0, 2], 8, table, 3,      # ... all of which the middle row holds
        counts=(np.array([5, 0, 7, 1], np.uint32), np.array([0, 2, 3, 0], np.uint32)))
    indptr, indices = random_rows(rng, [9, 0, 130, 3], N_MINOR)
    zeros = np.zeros(len(indices), np.uint32)
    add("entries_without_reads", indptr, indices, N_MINOR, random_table(rng, N_MINOR, 4), 4, counts=(zeros, zeros.copy()))
    add("sums_past_2_32", *random_rows(rng, row_lengths(3), N_MINOR), N_MINOR, random_table(rng, N_MINOR, 3), 3, big=True)
    add("sums_past_2_32_two_passes", *random_rows(rng, [0, 90, 3], N_MINOR), N_MINOR, random_table(rng, N_MINOR, 70), 70, big=True)
    for n in (64, 65):                                            # the highest byte of the table: one past it is outside
        last = np.full(5, N_MINOR - 1, np.uint32)
        add("last_variant_last_donor_%d" % n, [0, 2, 5], last, N_MINOR, random_table(rng, N_MINOR, n), n)
    indptr, indices = csr_with_row_lengths(rng, [0, 1, 36, 37, 20, 0], N_MINOR)
    add("canonical_sorted", indptr, indices, N_MINOR, random_table(rng, N_MINOR, 10), 10)
    add("one_variant", [0, 1, 1, 80], np.zeros(80, np.uint32), 1, random_table(rng, 1, 17), 17)
    return out
