"""``vartrix_amd.api.run(stats=, min_alt_cells=, min_ref_cells=)`` and ``api.select`` on the GPU.  The statistics must be numpy's
reductions of the plain run's count matrices on both axes; a filtered run must be scipy's indexing of the unfiltered one — matrices,
names, ``variant_index``, statistics — however the reads were ingested, the VCF streamed, the matrix oriented or the container chosen;
``select`` on a torch result must be ``select`` on the scipy result.  Inputs: the reference's fixture and the authored DNA BAM of
tests/test_gpu_api.py."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests.csr_ops_util import COUNTS, SUMS, model_stats
from tests.test_gpu_api import MATRICES, REF, bits, dna, same_csr  # noqa: F401  (dna: the module-scoped fixture of the authored BAM)
from vartrix_amd import api

pytestmark = pytest.mark.gpu

DNA_KW = dict(scoring_method="alt_frac", umi=True)


@pytest.fixture(scope="module")
def plain(dna):  # noqa: F811
    """The unfiltered run, variants x cells, scipy: computed once, read by every test, never changed."""
    return api.run(**dna, **DNA_KW, ingest="host")


def want_stats(result, axis):
    """numpy's statistics of a variants x cells scipy result per variant (axis 0) or per cell (axis 1)."""
    a, r, u = (m if axis == 0 else m.T.tocsr() for m in (result.alt_counts, result.ref_counts, result.unknown_counts))
    assert np.array_equal(a.indptr, r.indptr) and np.array_equal(a.indptr, u.indptr)
    return model_stats(a.indptr, a.data, r.data, u.data)


def as_numpy(stats):
    """Statistics of either container as numpy uint32 / uint64."""
    out = {}
    for k, v in stats.items():
        if isinstance(v, torch.Tensor):
            assert v.device.type == "cuda" and v.dtype == torch.int64
            v = v.cpu().numpy()
        out[k] = v.astype(np.uint32 if k in COUNTS else np.uint64)
    return out


def same_stats(got, want):
    got = as_numpy(got)
    assert set(got) == set(COUNTS + SUMS)
    for k in COUNTS + SUMS:
        assert np.array_equal(got[k], want[k]), k


def to_scipy(m):
    if m is None or sp.issparse(m):
        return m
    assert m.layout == torch.sparse_csr and m.device.type == "cuda"
    data = m.values().cpu().numpy()
    if data.dtype == np.int32:
        data = data.view(np.uint32)
    return sp.csr_matrix((data, m.col_indices().cpu().numpy(), m.crow_indices().cpu().numpy()), shape=tuple(m.shape))


def transposed(m):
    """scipy's transpose with the entries in the library's order (source order inside a row: ascending)."""
    pos = sp.csr_matrix((np.arange(1, m.nnz + 1, dtype=np.float64), m.indices, m.indptr), shape=m.shape).T.tocsr()
    pos.sort_indices()
    return sp.csr_matrix((m.data[pos.data.astype(np.int64) - 1], pos.indices, pos.indptr), shape=pos.shape)


def thresholds(plain):  # noqa: F811
    st = want_stats(plain, 0)
    a, r = int(np.median(st["n_alt"])), int(np.median(st["n_ref"]))
    keep = (st["n_alt"] >= a) & (st["n_ref"] >= r)
    print("thresholds: min_alt_cells", a, "min_ref_cells", r, "kept", int(keep.sum()), "of", keep.size)
    assert (a > 0 or r > 0) and 0 < keep.sum() < keep.size            # the filter filters, and not everything
    return a, r, keep


def check_filtered(got, plain, keep, orient):  # noqa: F811
    """``got`` (either container) is ``plain`` (variants x cells, scipy) cut to the variants of ``keep``."""
    rows = np.flatnonzero(keep)
    assert got.variants == [plain.variants[i] for i in rows] and got.barcodes == plain.barcodes and got.metrics == plain.metrics
    assert got.variant_index.dtype == np.int64 and np.array_equal(got.variant_index, rows) and got.orient == orient
    assert got.shape == ((len(rows), len(plain.barcodes)) if orient == "variants" else (len(plain.barcodes), len(rows)))
    for k in MATRICES:
        x, y = getattr(plain, k), to_scipy(getattr(got, k))
        assert (x is None) == (y is None), k
        if x is None:
            continue
        cut = x[rows]
        same_csr(y, cut if orient == "variants" else transposed(cut))
    cut = api.Result(**{k: (getattr(plain, k)[rows] if getattr(plain, k) is not None else None) for k in MATRICES}, variants=[], barcodes=[],
                     metrics={}, shape=())
    if got.variant_stats is not None:
        same_stats(got.variant_stats, want_stats(cut, 0))
        same_stats(got.cell_stats, want_stats(cut, 1))        # of the FILTERED matrix


@pytest.mark.parametrize("to", ["scipy", "torch"])
@pytest.mark.parametrize("orient", ["variants", "cells"])
def test_stats_equal_numpy_reductions_on_both_axes(dna, plain, orient, to):  # noqa: F811
    got = api.run(**dna, **DNA_KW, ingest="host", orient=orient, to=to, stats=True)
    assert got.variant_index is None and got.variants == plain.variants and got.orient == orient
    same_stats(got.variant_stats, want_stats(plain, 0))
    same_stats(got.cell_stats, want_stats(plain, 1))
    if to == "scipy":
        assert got.variant_stats["n_alt"].dtype == np.uint32 and got.cell_stats["sum_unk"].dtype == np.uint64
        assert len(got.variant_stats["n_alt"]) == len(plain.variants) and len(got.cell_stats["n_alt"]) == len(plain.barcodes)
    x = to_scipy(got.alt_counts)
    same_csr(x, plain.alt_counts if orient == "variants" else transposed(plain.alt_counts))     # stats=True changes no matrix
    st = want_stats(plain, 0)
    assert st["n_both"].sum() > 0 and (st["n_alt"] != st["n_ref"]).any() and st["sum_unk"].sum() >= 0


def test_defaults_add_nothing(plain):  # noqa: F811
    assert plain.variant_stats is None and plain.cell_stats is None and plain.variant_index is None and plain.orient == "variants"


def test_stats_on_the_reference_fixture():
    for mode in ("consensus", "coverage"):
        p = api.run(**REF, scoring_method=mode)
        got = api.run(**REF, scoring_method=mode, stats=True, orient="cells", to="torch")
        same_stats(got.variant_stats, want_stats(p, 0))
        same_stats(got.cell_stats, want_stats(p, 1))
        if mode == "coverage":                                  # coverage's matrices ARE the counts
            assert np.array_equal(as_numpy(got.variant_stats)["sum_alt"], np.asarray(p.matrix.sum(axis=1)).ravel().astype(np.uint64))
            assert np.array_equal(as_numpy(got.cell_stats)["sum_ref"], np.asarray(p.ref_matrix.sum(axis=0)).ravel().astype(np.uint64))


@pytest.mark.parametrize("ingest,stream_loci,orient,to", [("host", None, "variants", "scipy"), ("device", None, "cells", "torch"),
                                                          ("host", 7, "cells", "scipy"), ("device", 7, "variants", "torch"),
                                                          ("auto", 1, "variants", "scipy")])
def test_filtered_run_is_scipy_indexing_of_the_unfiltered_run(dna, plain, ingest, stream_loci, orient, to):  # noqa: F811
    a, r, keep = thresholds(plain)
    got = api.run(**dna, **DNA_KW, ingest=ingest, stream_loci=stream_loci, orient=orient, to=to, stats=True, min_alt_cells=a, min_ref_cells=r)
    check_filtered(got, plain, keep, orient)


def test_one_threshold_alone_and_a_threshold_nothing_passes(dna, plain):  # noqa: F811
    st = want_stats(plain, 0)
    a = int(np.median(st["n_alt"]))
    assert 0 < (st["n_alt"] >= a).sum() < len(plain.variants)
    check_filtered(api.run(**dna, **DNA_KW, min_alt_cells=a), plain, st["n_alt"] >= a, "variants")
    none = api.run(**dna, **DNA_KW, min_ref_cells=len(plain.barcodes) + 1, orient="cells", stats=True)
    assert none.shape == (len(plain.barcodes), 0) and none.variants == [] and none.variant_index.size == 0 and none.matrix.nnz == 0
    assert none.metrics == plain.metrics and as_numpy(none.cell_stats)["n_entries"].tolist() == [0] * len(plain.barcodes)
    with pytest.raises(ValueError):
        api.run(**dna, **DNA_KW, min_alt_cells=-1)


@pytest.mark.parametrize("orient", ["variants", "cells"])
def test_select_on_torch_equals_select_on_scipy(dna, orient):  # noqa: F811
    rng = np.random.default_rng(3)
    s = api.run(**dna, scoring_method="coverage", orient=orient, to="scipy")
    t = api.run(**dna, scoring_method="coverage", orient=orient, to="torch")
    vm, cm = rng.random(len(s.variants)) < 0.5, rng.random(len(s.barcodes)) < 0.6
    for v, c in ((vm, cm), (vm, None), (None, cm), (torch.from_numpy(vm).to("cuda:0"), cm)):
        a, b = api.select(s, variants=vm if v is not None else None, cells=c), api.select(t, variants=v, cells=c)
        assert a.shape == b.shape and a.variants == b.variants and a.barcodes == b.barcodes and a.metrics == b.metrics
        assert (a.variant_index is None) == (b.variant_index is None) and (a.variant_index is None or np.array_equal(a.variant_index, b.variant_index))
        for k in MATRICES:
            y = getattr(b, k)
            assert y.layout == torch.sparse_csr and y.device.type == "cuda" and tuple(y.shape) == a.shape
            same_csr(to_scipy(y), getattr(a, k))
    assert 0 < a.matrix.nnz < s.matrix.nnz
    with pytest.raises(ValueError):
        api.select(t, variants=vm[:-1])
