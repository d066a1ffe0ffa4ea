"""``vartrix_amd.api.pseudobulk`` and ``read_groups`` on the CPU: hand-built scipy ``Result``s folded by a label per cell, against the numpy
model of tests/csr_group_util.py — the order of the groups, cells that are left out, keys that match no barcode, both orientations — and
the label files.  (The torch path runs on the device: tests/test_gpu_api_pseudobulk.py.)"""
import gzip

import numpy as np
import pytest
import scipy.sparse as sp

from tests.csr_group_util import FIELDS, NONE, dense, model_pseudobulk
from tests.test_api_select import build
from vartrix_amd import api


def variant_major(r):
    mats = [r.alt_counts, r.ref_counts, r.unknown_counts]
    if r.orient == "cells":
        mats = [m.T.tocsr() for m in mats]
        for m in mats:
            m.sort_indices()
    return mats


def check(r, groups, names, labels, n_unmatched=0):
    got = api.pseudobulk(r, groups)
    want = model_pseudobulk(*variant_major(r), np.asarray(labels, np.uint32), len(names))
    shape = (len(r.variants), len(names))
    assert isinstance(got, api.GroupResult) and got.groups == names and got.variants == r.variants and got.orient == r.orient
    assert got.shape == (shape if r.orient == "variants" else shape[::-1]) and got.n_unmatched == n_unmatched
    lab = np.asarray(labels, np.int64)
    assert got.group_sizes.dtype == np.int64 and got.group_sizes.tolist() == np.bincount(lab[lab != NONE], minlength=len(names)).tolist()
    for f in FIELDS:
        m = getattr(got, f)
        assert sp.issparse(m) and m.format == "csr" and m.shape == got.shape and m.dtype == np.int64, f
        d = dense(m)
        assert np.array_equal(d if r.orient == "variants" else d.T, want[f]), f
    assert want["n_cells"].sum() > 0 or not len(names)
    return got


@pytest.mark.parametrize("orient", ["variants", "cells"])
def test_a_sequence_of_labels_with_cells_left_out(orient):
    r = build(orient)
    got = check(r, ["b", None, "a", "b", "a"], ["a", "b"], [1, NONE, 0, 1, 0])
    # by hand: the alt counts of cells 2 and 4 are group a's
    alt = variant_major(r)[0].toarray().astype(np.int64)
    a = dense(got.alt_counts)
    assert np.array_equal((a if orient == "variants" else a.T)[:, 0], alt[:, 2] + alt[:, 4])
    n = dense(got.n_alt_cells)
    assert np.array_equal((n if orient == "variants" else n.T)[:, 1], (alt[:, 0] > 0).astype(np.int64) + (alt[:, 3] > 0))


def test_labels_sort_as_numbers_when_every_one_is_a_number():
    r = build()
    check(r, ["10", "9", "10", "2", "9"], ["2", "9", "10"], [2, 1, 2, 0, 1])
    check(r, [10, 9, 10, 2, 9], [2, 9, 10], [2, 1, 2, 0, 1])
    check(r, ["10", "9", "x", "2", "9"], ["10", "2", "9", "x"], [0, 2, 3, 1, 2])          # one label that is none: by string


@pytest.mark.parametrize("orient", ["variants", "cells"])
def test_a_dict_leaves_out_the_barcodes_it_lacks_and_counts_the_keys_it_cannot_place(orient):
    r = build(orient)
    g = {"BC3-1": "t", "BC0-1": "s", "nobody-1": "s", b"BC4-1": "t", "ghost-1": "u"}
    got = check(r, g, ["s", "t"], [0, NONE, NONE, 1, 1], n_unmatched=2)
    assert got.group_sizes.tolist() == [1, 2]


def test_no_cell_with_a_label_gives_no_groups():
    r = build()
    got = check(r, [None] * 5, [], [NONE] * 5)
    assert got.shape == (7, 0) and got.alt_counts.nnz == 0


def test_a_filtered_result_folds_its_kept_rows_and_the_orientation_is_inferred():
    r = api.select(build("cells"), variants=np.array([1, 0, 1, 1, 0, 0, 1], bool))
    r.orient = None
    got = api.pseudobulk(r, [0, 0, 1, 1, 1])
    assert got.orient == "cells" and got.shape == (2, 4) and got.variants == r.variants
    want = model_pseudobulk(*[m.T.tocsr() for m in (r.alt_counts, r.ref_counts, r.unknown_counts)], np.array([0, 0, 1, 1, 1], np.uint32), 2)
    for f in FIELDS:
        assert np.array_equal(dense(getattr(got, f)).T, want[f]), f


def test_what_is_refused():
    r = build()
    with pytest.raises(ValueError):
        api.pseudobulk(r, [0, 1, 0, 1])                   # four labels for five cells
    with pytest.raises(ValueError):
        api.pseudobulk(r, [0, 1, 0, 1, 0], to="numpy")
    with pytest.raises(ValueError):
        api.pseudobulk(r, [0, 1, 0, 1, 0], to="torch")    # a scipy result is folded on the host


def test_read_groups(tmp_path):
    tab = tmp_path / "groups.tsv"
    tab.write_text("BC0-1\t3\nBC1-1\t1\n\nBC2-1\t3\n")
    assert api.read_groups(tab) == {"BC0-1": "3", "BC1-1": "1", "BC2-1": "3"}
    csv = tmp_path / "clusters.csv"
    csv.write_text("Barcode,Cluster\nBC0-1,2\nBC4-1,1\r\n")
    assert api.read_groups(str(csv)) == {"BC0-1": "2", "BC4-1": "1"}
    gz = tmp_path / "clusters.csv.gz"
    with gzip.open(gz, "wt") as f:
        f.write("barcode,cluster\nBC1-1,b\nBC3-1,a\n")
    assert api.read_groups(gz) == {"BC1-1": "b", "BC3-1": "a"}
    tgz = tmp_path / "donors.txt.gz"
    with gzip.open(tgz, "wt") as f:
        f.write("BC1-1\tdonor 2\n")
    assert api.read_groups(tgz) == {"BC1-1": "donor 2"}
    bad = tmp_path / "bad.tsv"
    bad.write_text("BC0-1,3\n")
    with pytest.raises(ValueError):
        api.read_groups(bad)
    # a path is a set of labels as it is
    r = build()
    got = api.pseudobulk(r, str(csv))
    assert got.groups == ["1", "2"] and got.group_sizes.tolist() == [1, 1] and got.n_unmatched == 0
    assert np.array_equal(dense(got.alt_counts)[:, 1], r.alt_counts.toarray()[:, 0].astype(np.int64))
