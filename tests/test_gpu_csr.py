"""vtx_device_csr after real runs: the variant-major CSR of a run's triplets on the device — only the row offsets are new — against
``fetch_coo`` put through scipy, on the reference's fixture and on the authored DNA BAM (46 VCF records, some skipped or without
reads: empty rows), in the three scoring modes with and without UMIs; windows, call order, and what the call must leave alone."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests.test_host import G, make_dna_bam
from vartrix_amd import abi, hostlib, lib
from vartrix_amd.abi import default_config
from vartrix_amd.api import _DevArray

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIELDS = (("alt", "<i4"), ("ref", "<i4"), ("unk", "<i4"), ("value", "<f8"), ("ref_value", "<f8"))


@pytest.fixture(scope="module")
def dna_bam(tmp_path_factory):
    return make_dna_bam(tmp_path_factory.mktemp("csr_dna"))


@functools.lru_cache(maxsize=None)
def packed(vcf, bam, fasta, barcodes, umi):
    return hostlib.pack_files(vcf, bam, fasta, barcodes, use_umi=umi, threads=2)


def inputs(which, dna_bam):
    if which == "reference":
        return os.path.join(G, "test.vcf"), os.path.join(G, "test.bam"), os.path.join(G, "test.fa"), os.path.join(G, "barcodes.tsv")
    return os.path.join(G, "test_dna.vcf"), dna_bam, os.path.join(G, "test_dna.fa"), os.path.join(G, "dna_barcodes.tsv")


def device_array(addr, n, typestr):
    if not n:
        return np.zeros(0, np.dtype(typestr))
    return torch.as_tensor(_DevArray(addr, n, typestr), device=DEV).cpu().numpy()


def read_csr(d):
    """The arrays behind the addresses of ``Context.device_csr``, copied to the host (uint32 / uint64 as the header declares them)."""
    out = {"indptr": device_array(d["indptr"], d["row_end"] - d["row_begin"] + 1, "<i8").view(np.uint64),
           "indices": device_array(d["indices"], d["nnz"], "<i4").view(np.uint32)}
    for k, ts in FIELDS:
        a = device_array(d[k], d["nnz"], ts)
        out[k] = a.view(np.uint32) if ts == "<i4" else a
    return out


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_window(ctx, coo, lo, hi, n_cols):
    d = ctx.device_csr(lo, hi)
    assert (d["nnz"], d["row_begin"], d["row_end"], d["n_cols"]) == (len(coo["row"]), lo, hi, n_cols)
    got = read_csr(d)
    want = sp.coo_matrix((np.ones(len(coo["row"])), (coo["row"].astype(np.int64) - lo, coo["col"].astype(np.int64))), shape=(hi - lo, n_cols)).tocsr()
    assert np.array_equal(got["indptr"], want.indptr.astype(np.uint64))
    assert same_bits(got["indices"], coo["col"])                # scipy's indices too: the triplets are in CSR order already
    assert np.array_equal(got["indices"], want.indices.astype(np.uint32))
    for k, _ in FIELDS:
        assert same_bits(got[k], coo[k]), k
    return d


@pytest.mark.parametrize("umi", [False, True])
@pytest.mark.parametrize("mode", ["consensus", "alt_frac", "coverage"])
@pytest.mark.parametrize("which", ["reference", "dna"])
def test_device_csr_equals_fetch_coo_through_scipy(which, mode, umi, dna_bam, tmp_path):
    batch, _, n_rows, barcodes, _ = packed(*inputs(which, dna_bam), umi)
    n_cols = len(barcodes)
    cfg = default_config(scoring_mode=mode, use_umi=int(umi), n_barcodes=n_cols)
    with lib.Context(cfg) as ctx:
        ctx.submit(batch)
        with pytest.raises(lib.VtxError) as e:                  # before a completed run
            ctx.device_csr(0, n_rows)
        assert e.value.status == abi.VTX_E_STATE
        ctx.run()
        coo = ctx.fetch_coo()
        assert len(coo["row"]) > 0
        d = check_window(ctx, coo, 0, n_rows, n_cols)            # the whole matrix
        assert d["indices"] == ctx.device_coo()["col"] != 0      # the very array of the triplets: nothing was copied
        for k in ("alt", "ref", "unk", "value", "ref_value"):
            assert d[k] == ctx.device_coo()[k]
        lens = np.diff(read_csr(d)["indptr"].astype(np.int64))
        assert np.array_equal(lens, np.bincount(coo["row"], minlength=n_rows))
        if which == "dna":
            assert (lens == 0).any()                             # skipped records / loci without reads: empty ranges
        rmin, rmax = int(coo["row"].min()), int(coo["row"].max())
        check_window(ctx, coo, rmin, rmax + 1, n_cols)           # the tightest window that holds every triplet
        check_window(ctx, coo, 0, n_rows + 70, n_cols)           # empty rows behind the matrix
        check_window(ctx, coo, 0, n_rows + 5000, n_cols)         # ... a stretch long enough for the per-row lanes (csr_fill_kernel)
        for lo, hi in ((rmin + 1, n_rows), (0, rmax), (rmax + 1, rmax + 1), (3, 2)):      # a window that cuts a triplet's row; begin > end
            with pytest.raises(lib.VtxError) as e:
                ctx.device_csr(lo, hi)
            assert e.value.status == abi.VTX_E_INVAL
        again = ctx.fetch_coo()                                  # nothing the triplet calls return has changed
        for k in coo:
            assert same_bits(coo[k], again[k]), k
        # the text writers work in the ingest's buffers; the offsets live in a buffer of their own: correct again after one of them
        before = read_csr(ctx.device_csr(0, n_rows))
        ctx.write_mtx(str(tmp_path / "m.mtx"), n_rows, n_cols, 0, real=(mode == "alt_frac"))
        ctx.mtx_part(0, real=True, gz=True)
        after = check_window(ctx, coo, 0, n_rows, n_cols)
        assert all(same_bits(before[k], read_csr(after)[k]) for k in before)
        ctx.run()                                                # and after another run of the same batch
        check_window(ctx, coo, 0, n_rows, n_cols)


def test_a_run_without_triplets_has_all_zero_offsets():
    from vartrix_amd.abi import LOCUS_DTYPE, RECORD_DTYPE, PackedBatch
    batch = PackedBatch(np.zeros(0, LOCUS_DTYPE), np.zeros(0, RECORD_DTYPE), np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    with lib.Context(default_config(aligner="full", n_barcodes=4)) as ctx:
        ctx.submit(batch)
        ctx.run()
        d = ctx.device_csr(5, 12)
        assert (d["nnz"], d["n_cols"]) == (0, 4)
        assert np.array_equal(read_csr(d)["indptr"], np.zeros(8, np.uint64))
        assert read_csr(ctx.device_csr(0, 0))["indptr"].tolist() == [0]
