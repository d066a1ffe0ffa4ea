"""``vartrix_amd.api.run(groups=)`` and ``api.pseudobulk`` on the GPU, on the reference's fixture with the barcodes of barcodes.tsv split
into three groups and some cells left out: the fold computed on the device must be the numpy model of tests/csr_group_util.py applied
to the scipy run's count matrices, exactly, however the reads were ingested, the VCF streamed, the matrix oriented or filtered; and
``pseudobulk`` on a finished torch result must be what ``run(groups=)`` returned."""
import numpy as np
import pytest
import torch

from tests.csr_group_util import FIELDS, NONE, dense, model_pseudobulk
from tests.test_gpu_api import REF, dna  # noqa: F401  (dna: the module-scoped fixture of the authored BAM)
from vartrix_amd import api

pytestmark = pytest.mark.gpu

KW = dict(scoring_method="coverage")
NAMES = ["donor_a", "donor_b", "donor_c"]


@pytest.fixture(scope="module")
def plain():
    """The plain scipy run, variants x cells: computed once, read by every test, never changed."""
    return api.run(**REF, **KW, ingest="host")


@pytest.fixture(scope="module")
def labels(plain):
    """barcode -> label: every fourth cell is left out, the others go round the three groups; one key is no barcode of the run."""
    g = {b: NAMES[i % 4] for i, b in enumerate(plain.barcodes) if i % 4 != 3}
    g["NOT-A-BARCODE-1"] = NAMES[0]
    number = np.array([NONE if i % 4 == 3 else i % 4 for i in range(len(plain.barcodes))], np.uint32)
    assert len(plain.barcodes) >= 8 and plain.alt_counts.nnz > 0
    return g, number


@pytest.fixture(scope="module")
def want(plain, labels):
    return model_pseudobulk(plain.alt_counts, plain.ref_counts, plain.unknown_counts, labels[1], 3)


def check(got, want, plain, labels, orient="variants", rows=None, device=True):
    rows = np.arange(len(plain.variants)) if rows is None else rows
    assert isinstance(got, api.GroupResult) and got.groups == NAMES and got.orient == orient and got.n_unmatched == 1
    assert got.variants == [plain.variants[i] for i in rows]
    assert got.shape == ((len(rows), 3) if orient == "variants" else (3, len(rows)))
    number = labels[1]
    assert got.group_sizes.tolist() == np.bincount(number[number != NONE].astype(np.int64), minlength=3).tolist()
    for f in FIELDS:
        m = getattr(got, f)
        assert tuple(m.shape) == got.shape, f
        if device:
            assert isinstance(m, torch.Tensor) and m.layout == torch.sparse_csr and m.device.type == "cuda" and m.dtype == torch.int64, f
        d = dense(m)
        assert np.array_equal(d if orient == "variants" else d.T, want[f][rows]), f


def test_the_model_has_something_to_say(want):
    """(The fixture is small: a handful of entries.  The authored DNA BAM below has more.)"""
    assert want["n_cells"].sum() > 0 and want["alt_counts"].sum() + want["ref_counts"].sum() > 0


@pytest.mark.parametrize("orient", ["variants", "cells"])
def test_run_with_groups_is_the_model_of_the_scipy_run(plain, labels, want, orient):
    got = api.run(**REF, **KW, to="torch", groups=labels[0], orient=orient)
    check(got.groups, want, plain, labels, orient)
    # pseudobulk on the finished result: the same fold, from the result's own tensors
    again = api.pseudobulk(got, labels[0])
    check(again, want, plain, labels, orient)
    for f in FIELDS:
        a, b = getattr(got.groups, f), getattr(again, f)
        assert torch.equal(a.crow_indices(), b.crow_indices()) and torch.equal(a.col_indices(), b.col_indices()) and torch.equal(a.values(), b.values()), f
    # ... and to="scipy" copies the same numbers to the host
    check(api.pseudobulk(got, labels[0], to="scipy"), want, plain, labels, orient, device=False)


@pytest.mark.parametrize("ingest,stream_loci", [("host", 1), ("device", None), ("device", 1)])
def test_the_fold_does_not_depend_on_ingest_or_streaming(plain, labels, want, ingest, stream_loci):
    got = api.run(**REF, **KW, to="torch", groups=labels[0], ingest=ingest, stream_loci=stream_loci)
    check(got.groups, want, plain, labels)


@pytest.mark.parametrize("orient", ["variants", "cells"])
def test_a_filtered_run_folds_its_kept_rows(plain, labels, want, orient):
    got = api.run(**REF, **KW, to="torch", groups=labels[0], min_alt_cells=1, orient=orient)
    rows = np.flatnonzero(np.asarray((plain.alt_counts > 0).sum(axis=1)).ravel() >= 1)
    assert 0 < len(rows) and got.variant_index.tolist() == rows.tolist()
    check(got.groups, want, plain, labels, orient, rows)
    check(api.pseudobulk(got, labels[0]), want, plain, labels, orient, rows)


def test_a_scipy_run_with_groups_and_a_file_of_labels(plain, labels, want, tmp_path):
    path = tmp_path / "clusters.csv"
    path.write_text("Barcode,Cluster\n" + "".join("%s,%s\n" % kv for kv in labels[0].items()))
    got = api.run(**REF, **KW, groups=str(path))
    assert got.groups.alt_counts.format == "csr"
    check(got.groups, want, plain, labels, device=False)
    assert api.run(**REF, **KW).groups is None


@pytest.mark.parametrize("orient", ["variants", "cells"])
def test_a_denser_matrix_many_groups_and_numbers_as_labels(dna, orient):  # noqa: F811
    """The authored DNA BAM: rows with many cells, so that a group sums several of them; integer labels, sorted as numbers."""
    kw = dict(scoring_method="alt_frac", umi=True, ingest="host")
    p = api.run(**dna, **kw)
    n = len(p.barcodes)
    number = np.array([NONE if i % 7 == 3 else (i * 5) % 11 for i in range(n)], np.uint32)
    names = sorted(set(int(g) for g in number if g != NONE))
    assert names == list(range(11)) and p.alt_counts.nnz > 50
    seq = [None if g == NONE else int(g) * 10 for g in number]          # labels 0, 10, 20, ... 100: by number, not "0" < "10" < "100" < "20"
    want = model_pseudobulk(p.alt_counts, p.ref_counts, p.unknown_counts, number, 11)
    assert (want["n_cells"] > 1).any() and (want["n_alt_cells"] > 0).any() and (want["n_ref_cells"] > 0).any()
    got = api.run(**dna, **kw, to="torch", orient=orient, groups=seq).groups
    assert got.groups == [10 * g for g in names] and got.n_unmatched == 0 and got.orient == orient
    for f in FIELDS:
        d = dense(getattr(got, f))
        assert np.array_equal(d if orient == "variants" else d.T, want[f]), f
