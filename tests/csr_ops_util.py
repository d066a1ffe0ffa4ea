"""numpy models of the CSR summaries and selections (vtx_csr_row_stats, vtx_csr_select), shared by the CPU tests of the core header and
the GPU tests of the kernels.  Nothing here knows the code under test."""
import numpy as np

COUNTS = ("n_entries", "n_alt", "n_ref", "n_both")
SUMS = ("sum_alt", "sum_ref", "sum_unk")


def model_stats(indptr, alt, ref, unk):
    """The seven statistics of every row: counts by ``bincount``, sums by ``add.reduceat`` in uint64 (exact)."""
    indptr = np.asarray(indptr).astype(np.int64)
    n, lens = len(indptr) - 1, np.diff(indptr)
    rows = np.repeat(np.arange(n), lens)
    full = lens > 0

    def count(sel):
        return np.bincount(rows[sel], minlength=n).astype(np.uint32)

    def total(a):
        out = np.zeros(n, np.uint64)
        if full.any():       # the starts of the non-empty rows: consecutive ones bound each other, empty rows in between have no extent
            out[full] = np.add.reduceat(np.asarray(a).astype(np.uint64), indptr[:-1][full])
        return out
    alt, ref, unk = (np.asarray(a) for a in (alt, ref, unk))
    return {"n_entries": lens.astype(np.uint32), "n_alt": count(alt > 0), "n_ref": count(ref > 0), "n_both": count((alt > 0) & (ref > 0)),
            "sum_alt": total(alt), "sum_ref": total(ref), "sum_unk": total(unk)}


def model_select(indptr, indices, n_minor, keep_major, keep_minor, payloads=()):
    """Mask the entries, renumber, keep the order.  A mask of None keeps everything; any non-zero byte keeps.
    -> dict(indptr, indices, major_ids, minor_ids, payloads)."""
    indptr, indices = np.asarray(indptr).astype(np.int64), np.asarray(indices).astype(np.int64)
    n_major = len(indptr) - 1
    rm = np.ones(n_major, bool) if keep_major is None else np.asarray(keep_major) != 0
    cm = np.ones(n_minor, bool) if keep_minor is None else np.asarray(keep_minor) != 0
    rows = np.repeat(np.arange(n_major), np.diff(indptr))
    keep = rm[rows] & cm[indices]
    new_row, new_col = np.cumsum(rm) - 1, np.cumsum(cm) - 1
    out_rows = new_row[rows[keep]]                                    # ascending: rows keep their order
    return {"indptr": np.searchsorted(out_rows, np.arange(int(rm.sum()) + 1), side="left").astype(np.uint64),
            "indices": new_col[indices[keep]].astype(np.uint32), "major_ids": np.flatnonzero(rm).astype(np.uint32),
            "minor_ids": np.flatnonzero(cm).astype(np.uint32), "payloads": [np.asarray(p)[keep] for p in payloads]}


def csr_with_row_lengths(rng, lens, n_minor, sort=True):
    """A CSR whose row r has lens[r] entries with distinct columns (needs max(lens) <= n_minor), ascending inside a row if ``sort``."""
    lens = np.asarray(lens, np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    cols = [rng.permutation(n_minor)[:n] for n in lens]
    cols = [np.sort(c) if sort else c for c in cols]
    return indptr, (np.concatenate(cols) if cols else np.zeros(0)).astype(np.uint32)


def random_counts(rng, n, big=False):
    """alt / ref / unk with zeros in every combination; ``big``: values near 2^32, so that a row's sum passes it."""
    hi = 1 << 32 if big else 50
    lo = (1 << 32) - 1000 if big else 1
    out = []
    for _ in range(3):
        a = rng.integers(lo, hi, n, dtype=np.uint64).astype(np.uint32)
        a[rng.random(n) < 0.4] = 0
        out.append(a)
    return out
