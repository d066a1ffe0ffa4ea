"""``vartrix_amd.api.select`` on the CPU: hand-built scipy ``Result``s cut by boolean masks — matrices, names, ``variant_index`` — in
both orientations, and the masks it must refuse.  (The torch path runs on the device: tests/test_gpu_api_filter.py.)"""
import numpy as np
import pytest
import scipy.sparse as sp

from vartrix_amd import api

MATRICES = ("matrix", "ref_matrix", "alt_counts", "ref_counts", "unknown_counts")


def build(orient="variants", coverage=False, variant_index=None, n_var=7, n_cell=5, seed=0):
    rng = np.random.default_rng(seed)
    pattern = sp.random(n_var, n_cell, density=0.5, random_state=np.random.RandomState(seed), format="csr")
    pattern.sort_indices()
    nnz = pattern.nnz

    def mat(data):
        m = sp.csr_matrix((data, pattern.indices.copy(), pattern.indptr.copy()), shape=(n_var, n_cell))
        if orient == "cells":
            m = m.T.tocsr()
            m.sort_indices()
        return m
    value = rng.random(nnz)
    value[::3] = np.nan                                   # alt_frac's NaN and explicit zeros are entries
    value[1::4] = 0.0
    counts = [rng.integers(0, 9, nnz).astype(np.uint32) for _ in range(3)]
    shape = (n_var, n_cell) if orient == "variants" else (n_cell, n_var)
    return api.Result(matrix=mat(value), ref_matrix=mat(rng.random(nnz)) if coverage else None, alt_counts=mat(counts[0]),
                      ref_counts=mat(counts[1]), unknown_counts=mat(counts[2]), variants=["chr1_%d" % i for i in range(n_var)],
                      barcodes=["BC%d-1" % i for i in range(n_cell)], metrics={"num_reads": 11}, shape=shape, variant_index=variant_index,
                      orient=orient)


def same(a, b):
    assert a.shape == b.shape and a.nnz == b.nnz and a.dtype == b.dtype
    assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
    assert np.array_equal(a.data, b.data, equal_nan=True)


@pytest.mark.parametrize("orient", ["variants", "cells"])
@pytest.mark.parametrize("coverage", [False, True])
def test_select_cuts_matrices_and_names(orient, coverage):
    r = build(orient, coverage)
    vm = np.array([1, 0, 1, 1, 0, 0, 1], bool)
    cm = np.array([0, 1, 1, 0, 1], bool)
    for v, c in ((vm, cm), (vm, None), (None, cm), (None, None)):
        got = api.select(r, variants=v, cells=c)
        rv, rc = (np.ones(7, bool) if v is None else v), (np.ones(5, bool) if c is None else c)
        rows, cols = (rv, rc) if orient == "variants" else (rc, rv)
        assert got.shape == (rows.sum(), cols.sum()) and got.orient == orient and got.metrics == r.metrics and got.metrics is not r.metrics
        assert got.variants == [n for n, k in zip(r.variants, rv) if k] and got.barcodes == [n for n, k in zip(r.barcodes, rc) if k]
        for k in MATRICES:
            x = getattr(r, k)
            if x is None:
                assert getattr(got, k) is None
                continue
            y = getattr(got, k)
            assert sp.issparse(y) and y.format == "csr"
            same(y, x[np.flatnonzero(rows)][:, np.flatnonzero(cols)])
            assert np.array_equal(y.toarray(), x.toarray()[np.ix_(rows, cols)], equal_nan=True)
        assert (got.variant_index is None) == (v is None)
        if v is not None:
            assert got.variant_index.dtype == np.int64 and got.variant_index.tolist() == np.flatnonzero(v).tolist()
    assert np.isnan(r.matrix.data).any() and (r.matrix.data == 0).any()


def test_select_composes_the_variant_index_of_a_filtered_run():
    """A result that a filter already cut names its source rows; a second cut indexes into those."""
    source = np.array([3, 4, 10, 11, 12, 40, 41], np.int64)
    r = build(variant_index=source)
    got = api.select(r, variants=np.array([0, 1, 1, 0, 0, 0, 1], bool))
    assert got.variant_index.tolist() == [4, 10, 41]
    assert api.select(r, cells=np.array([1, 1, 0, 0, 0], bool)).variant_index.tolist() == source.tolist()
    again = api.select(got, variants=np.array([1, 0, 1], bool))
    assert again.variant_index.tolist() == [4, 41] and again.variants == ["chr1_1", "chr1_6"]


def test_orientation_is_inferred_when_the_result_does_not_name_it():
    r = build("cells")
    r.orient = None
    got = api.select(r, variants=np.array([1, 0, 0, 0, 0, 0, 1], bool))
    assert got.shape == (5, 2) and got.variants == ["chr1_0", "chr1_6"]
    same(got.matrix, r.matrix[:, [0, 6]])


def test_all_false_masks_give_empty_matrices():
    got = api.select(build(), variants=np.zeros(7, bool), cells=np.zeros(5, bool))
    assert got.shape == (0, 0) and got.matrix.shape == (0, 0) and got.variants == [] and got.barcodes == [] and got.variant_index.size == 0


def test_masks_of_the_wrong_length_or_type_are_refused():
    r = build()
    for kw in (dict(variants=np.ones(6, bool)), dict(variants=np.ones(8, bool)), dict(cells=np.ones(7, bool)), dict(cells=np.ones(0, bool)),
               dict(variants=np.ones((7, 1), bool)), dict(variants=np.ones(5, bool), cells=np.ones(7, bool)),
               dict(variants=np.arange(7)), dict(cells=[0, 2])):
        with pytest.raises(ValueError):
            api.select(r, **kw)
    assert r.shape == (7, 5) and r.matrix.shape == (7, 5)          # the result it was given is as it was
