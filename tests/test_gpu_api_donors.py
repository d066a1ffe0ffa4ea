"""``vartrix_amd.api.donor_tally`` and ``assign_donors`` on the GPU, on the inputs tests/test_gpu_api_pseudobulk.py runs (the reference's
fixture and the authored DNA BAM) with a seeded random genotype table of 5 donors: the tally of a torch result, computed on the device,
must be the tally of the scipy result, computed on the host, and the numpy model of tests/csr_geno_util.py applied to the result's own
counts, exactly, in both orientations; the assignments on top must be identical arrays; and a result cut by ``select`` with the table cut
by the same mask must tally like the uncut pair with the dropped variants set to missing."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests.csr_geno_util import BYTES, NONE, model_geno_tally
from tests.test_gpu_api import REF, dna  # noqa: F401  (dna: the module-scoped fixture of the authored BAM)
from vartrix_amd import api

pytestmark = pytest.mark.gpu

N_DONORS = 5
FIELDS = (("alt", "sum_alt"), ("ref", "sum_ref"), ("n_obs", "n_obs"))


@pytest.fixture(scope="module")
def inputs(dna):  # noqa: F811
    return {"ref": (REF, dict(scoring_method="coverage")), "dna": (dna, dict(scoring_method="alt_frac", umi=True, ingest="host"))}


def table(n_var, seed=5):
    return BYTES[np.random.default_rng(seed).choice(4, (n_var, N_DONORS), p=[0.3, 0.3, 0.25, 0.15])]


def host(m):
    """A count matrix of a result, scipy or torch, as a scipy CSR with the entries as they are stored."""
    if sp.issparse(m):
        return m.tocsr()
    return sp.csr_matrix((m.values().cpu().numpy(), m.col_indices().cpu().numpy(), m.crow_indices().cpu().numpy()), shape=tuple(m.shape))


def model_of(r, geno):
    """The model on the result's own counts, cell-major."""
    alt, ref = host(r.alt_counts), host(r.ref_counts)
    if r.orient == "variants":
        alt, ref = alt.T.tocsr(), ref.T.tocsr()
    assert np.array_equal(alt.indptr, ref.indptr) and np.array_equal(alt.indices, ref.indices)
    return model_geno_tally(alt.indptr, alt.indices, alt.data.astype(np.uint32), ref.data.astype(np.uint32), geno, geno.shape[1])


def numbers(t):
    return {f: (getattr(t, f).cpu().numpy() if isinstance(getattr(t, f), torch.Tensor) else getattr(t, f)) for f, _ in FIELDS}


@pytest.mark.parametrize("which", ["ref", "dna"])
@pytest.mark.parametrize("orient", ["variants", "cells"])
def test_the_device_tally_is_the_host_tally_and_the_model(inputs, which, orient):
    files, kw = inputs[which]
    on_host = api.run(**files, **kw, orient=orient)
    on_dev = api.run(**files, **kw, orient=orient, to="torch")
    geno = table(len(on_host.variants))
    want = model_of(on_dev, geno)
    assert want["sum_alt"][..., :3].sum() + want["sum_ref"][..., :3].sum() > 0
    a, b = api.donor_tally(on_host, geno), api.donor_tally(on_dev, geno)
    assert a.barcodes == b.barcodes == on_host.barcodes and a.donors == b.donors == list(range(N_DONORS))
    for f, k in FIELDS:
        t = getattr(b, f)
        assert isinstance(t, torch.Tensor) and t.device.type == "cuda" and t.dtype == torch.int64, f
        assert tuple(t.shape) == (len(on_host.barcodes), N_DONORS, 4), f
        assert isinstance(getattr(a, f), np.ndarray) and getattr(a, f).dtype == np.int64, f
        assert np.array_equal(t.cpu().numpy(), want[k].astype(np.int64)), f
        assert np.array_equal(getattr(a, f), want[k].astype(np.int64)), f
    c = api.donor_tally(on_dev, geno, to="scipy")                      # the same numbers copied to the host
    assert all(isinstance(getattr(c, f), np.ndarray) and np.array_equal(getattr(c, f), getattr(a, f)) for f, _ in FIELDS)
    x, y = api.assign_donors(a, error=0.05), api.assign_donors(b, error=0.05)
    z = api.assign_donors(on_dev, geno, error=0.05)
    for other in (y, z):
        assert x.best.tobytes() == other.best.tobytes() and x.margin.tobytes() == other.margin.tobytes()
        assert x.log_lik.tobytes() == other.log_lik.tobytes()
    assert x.best.shape == (len(on_host.barcodes),) and x.best.max() >= 0


@pytest.mark.parametrize("orient", ["variants", "cells"])
def test_a_cut_result_with_the_cut_table_tallies_like_the_uncut_pair_with_the_dropped_variants_missing(inputs, orient):
    """Classes 0 - 2 are equal.  The reads at the dropped variants are class 3 in the uncut pair and absent from the cut one, so the
    whole cut tally is compared with the model on the cut result's own counts."""
    files, kw = inputs["dna"]
    r = api.run(**files, **kw, orient=orient, to="torch")
    n_var = len(r.variants)
    geno = table(n_var, seed=6)
    mask = np.random.default_rng(8).random(n_var) < 0.6
    assert 0 < mask.sum() < n_var
    cut = api.select(r, variants=mask)
    got = numbers(api.donor_tally(cut, geno[mask]))
    gone = geno.copy()
    gone[~mask] = NONE
    whole = numbers(api.donor_tally(r, gone))
    assert whole["alt"][..., :3].sum() + whole["ref"][..., :3].sum() > 0
    for f, k in FIELDS:
        assert np.array_equal(got[f][..., :3], whole[f][..., :3]), f
    want = model_of(cut, geno[mask])
    for f, k in FIELDS:
        assert np.array_equal(got[f], want[k].astype(np.int64)), f
