"""``vartrix_amd.api.run`` on the GPU: the four input files in, scipy / torch CSR of every array of the run out.  On the reference's
fixture the matrices must be the stored Matrix-Market files read back with scipy, in structure and in bits (NaN and explicit zeros
included); on the authored DNA BAM the result must not depend on how the reads were ingested, on the streaming of the VCF, or on the
container asked for."""
import os

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp
import torch

from tests.test_host import G, make_dna_bam
from vartrix_amd import api, hostlib, lib
from vartrix_amd.abi import default_config

pytestmark = pytest.mark.gpu

REF = dict(vcf=os.path.join(G, "test.vcf"), bam=os.path.join(G, "test.bam"), fasta=os.path.join(G, "test.fa"),
           cell_barcodes=os.path.join(G, "barcodes.tsv"))
MATRICES = ("matrix", "ref_matrix", "alt_counts", "ref_counts", "unknown_counts")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.astype(np.int64)


def same_csr(a, b):
    """Two scipy CSR matrices: same shape, same offsets, same indices in the same order, same value BITS."""
    assert a.shape == b.shape and a.nnz == b.nnz
    assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
    assert np.array_equal(bits(a.data), bits(b.data))


def same_result(a, b):
    for k in MATRICES:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), k
        if x is not None:
            same_csr(x, y)
    assert a.metrics == b.metrics and a.variants == b.variants and a.barcodes == b.barcodes and a.shape == b.shape


def golden(name):
    m = scipy.io.mmread(os.path.join(G, name)).tocsr()      # explicit zeros and NaN survive mmread + tocsr
    m.sort_indices()
    return m


@pytest.fixture(scope="module")
def dna(tmp_path_factory):
    bam = make_dna_bam(tmp_path_factory.mktemp("api_dna"))
    return dict(vcf=os.path.join(G, "test_dna.vcf"), bam=bam, fasta=os.path.join(G, "test_dna.fa"), cell_barcodes=os.path.join(G, "dna_barcodes.tsv"))


@pytest.fixture(scope="module")
def dna_baseline(dna):
    return api.run(**dna, scoring_method="alt_frac", umi=True, ingest="host")


def test_reference_fixture_equals_the_stored_matrices():
    cons = api.run(**REF)
    want = golden("test_consensus.mtx")
    same_csr(cons.matrix, want)
    assert cons.shape == want.shape == (4, 20) and cons.ref_matrix is None
    assert len(cons.variants) == 4 and len(cons.barcodes) == 20 and set(cons.metrics) == set(hostlib.METRIC_NAMES)
    frac = api.run(**REF, scoring_method="alt_frac")
    want = golden("test_frac.mtx")
    assert want.nnz == 4 and int((want.data == 0).sum()) == 3              # the three explicit zeros are entries
    same_csr(frac.matrix, want)
    for umi, sfx in ((False, ""), (True, "_umi")):
        cov = api.run(**REF, scoring_method="coverage", umi=umi)
        same_csr(cov.matrix, golden("test_coverage%s.mtx" % sfx))
        same_csr(cov.ref_matrix, golden("test_coverage_ref%s.mtx" % sfx))
        assert cov.alt_counts.data.dtype == np.uint32
        assert np.array_equal(cov.alt_counts.data, cov.matrix.data) and np.array_equal(cov.ref_counts.data, cov.ref_matrix.data)


def test_cells_orientation_is_the_transpose(dna, dna_baseline):
    cells = api.run(**dna, scoring_method="alt_frac", umi=True, ingest="host", orient="cells")
    assert cells.shape == dna_baseline.shape[::-1] and cells.matrix.shape == cells.shape
    assert np.isnan(dna_baseline.matrix.data).any() or (dna_baseline.matrix.data == 0).any()
    for k in MATRICES:
        x = getattr(dna_baseline, k)
        if x is None:
            assert getattr(cells, k) is None
            continue
        # scipy's transpose of the variant-major matrix, carrying the source POSITIONS: the entries must come in exactly that order
        pos = sp.csr_matrix((np.arange(1, x.nnz + 1, dtype=np.float64), x.indices, x.indptr), shape=x.shape).T.tocsr()
        got = getattr(cells, k)
        assert np.array_equal(got.indptr, pos.indptr) and np.array_equal(got.indices, pos.indices)
        assert np.array_equal(bits(got.data), bits(x.data[pos.data.astype(np.int64) - 1]))
    assert cells.metrics == dna_baseline.metrics and cells.variants == dna_baseline.variants


def dense_of_torch(t):
    assert t.layout == torch.sparse_csr and t.device.type == "cuda"
    return t.to_dense().cpu().numpy()


@pytest.mark.parametrize("orient", ["variants", "cells"])
def test_torch_equals_scipy(orient):
    for mode in ("alt_frac", "coverage"):
        s = api.run(**REF, scoring_method=mode, orient=orient, to="scipy")
        t = api.run(**REF, scoring_method=mode, orient=orient, to="torch")
        assert s.shape == t.shape and s.metrics == t.metrics and s.variants == t.variants and s.barcodes == t.barcodes
        for k in MATRICES:
            x, y = getattr(s, k), getattr(t, k)
            assert (x is None) == (y is None)
            if x is None:
                continue
            assert tuple(y.shape) == x.shape
            assert np.array_equal(y.crow_indices().cpu().numpy(), x.indptr) and np.array_equal(y.col_indices().cpu().numpy(), x.indices)
            assert np.array_equal(bits(y.values().cpu().numpy()), bits(x.data))
            if k in ("matrix", "ref_matrix"):
                assert np.array_equal(dense_of_torch(y), x.toarray(), equal_nan=True)


@pytest.mark.parametrize("stream_loci", [None, 7, 1])
@pytest.mark.parametrize("ingest", ["host", "device", "auto"])
def test_result_does_not_depend_on_ingest_or_streaming(dna, dna_baseline, ingest, stream_loci):
    got = api.run(**dna, scoring_method="alt_frac", umi=True, ingest=ingest, stream_loci=stream_loci)
    same_result(got, dna_baseline)
    assert got.shape == (46, len(got.barcodes)) and got.metrics["num_multiallelic_recs"] == 1 and got.metrics["num_reads"] > 0


@pytest.mark.parametrize("stream_loci", [None, 20])
def test_a_pack_of_several_batches_is_windowed_batch_by_batch(dna, dna_baseline, monkeypatch, stream_loci):
    """The host packer cuts a pack into batches of consecutive loci (here forced by the developer build's VTXH_BATCH_BYTES): every
    batch is a run of its own, and its part's window ends where the next batch's rows begin."""
    hostlib.use_variant("dev")
    try:
        monkeypatch.setenv("VTXH_BATCH_BYTES", "9000")
        batches = hostlib.pack_files(**dna, use_umi=True, all_batches=True)[0]
        assert len(batches) > 3
        got = api.run(**dna, scoring_method="alt_frac", umi=True, ingest="host", stream_loci=stream_loci)
    finally:
        hostlib.use_variant("dev" if os.environ.get("VTX_LIB_VARIANT") == "dev" else "")
    same_result(got, dna_baseline)


def test_auto_packs_on_the_host_what_the_device_declines(dna, dna_baseline, monkeypatch):
    """``auto``: a range whose submit the device declines with VTX_E_UNSUPPORTED is packed on the host, on the SAME context (barcodes
    already set by an earlier range, device ranges before and after it); ``device`` fails with the device's reason instead.  The
    decline is played by the binding here — every BAM the device declines in this suite is one the host packer rejects too."""
    real, calls = lib.Context.submit_bam, []

    def declining(self, ingest, n_loci):
        calls.append(n_loci)
        if len(calls) in (2, 5):
            raise lib.VtxError(-5, "vtx_submit_bam: declined for the test: the host packer decides")
        return real(self, ingest, n_loci)
    monkeypatch.setattr(lib.Context, "submit_bam", declining)
    got = api.run(**dna, scoring_method="alt_frac", umi=True, ingest="auto", stream_loci=7)
    assert len(calls) == 7                                   # 46 records in ranges of 7: every range was offered to the device
    same_result(got, dna_baseline)
    calls.clear()
    with pytest.raises(lib.VtxError) as e:
        api.run(**dna, scoring_method="alt_frac", umi=True, ingest="device", stream_loci=7)
    assert e.value.status == -5 and len(calls) == 2


def test_counts_equal_fetch_coo_and_the_coverage_matrices(dna):
    cons = api.run(**dna, stream_loci=7)
    batch, metrics, n_rows, barcodes, variants = hostlib.pack_files(**dna)
    with lib.Context(default_config(n_barcodes=len(barcodes))) as ctx:
        ctx.submit(batch)
        ctx.run()
        coo = ctx.fetch_coo()
    assert cons.metrics == metrics and cons.variants == variants and cons.barcodes == [b.decode() for b in barcodes]
    rows = np.repeat(np.arange(n_rows), np.diff(cons.matrix.indptr))
    assert np.array_equal(rows, coo["row"]) and np.array_equal(cons.matrix.indices, coo["col"])
    for k, f in (("matrix", "value"), ("alt_counts", "alt"), ("ref_counts", "ref"), ("unknown_counts", "unk")):
        assert np.array_equal(bits(getattr(cons, k).data), bits(coo[f])), k
    # the counts behind a consensus value are what a coverage run reports for the same cell
    cov = api.run(**dna, scoring_method="coverage")
    r, c = rows, cons.matrix.indices
    assert np.array_equal(cons.alt_counts.data, np.asarray(cov.matrix.toarray()[r, c], np.uint32))
    assert np.array_equal(cons.ref_counts.data, np.asarray(cov.ref_matrix.toarray()[r, c], np.uint32))


def test_bad_arguments_are_refused_before_any_work():
    for kw in (dict(orient="rows"), dict(to="numpy"), dict(ingest="gpu"), dict(scoring_method="best"), dict(stream_loci=0)):
        with pytest.raises(ValueError):
            api.run(**REF, **kw)
