"""``vartrix_amd.api.doublet_tally`` and ``assign_doublets`` on the GPU, on synthetic results: the tally of a torch result, computed on the
device, must be the numpy model of tests/csr_geno_pair_util.py and the tally of the same result as scipy matrices, computed on the host,
exactly, in both orientations; the assignments on top must be identical arrays; and the authored pool of tests/test_api_doublets.py must
come back from the device tally."""
import numpy as np
import pytest
import torch

from tests.csr_geno_pair_util import random_pairs
from tests.csr_geno_util import BYTES
from tests.test_api_doublets import FIELDS, agrees, authored_pool, model_of, recovered, scalar_model
from tests.test_api_select import build
from vartrix_amd import api

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def on_device(r):
    """A scipy result as the torch result ``run(to="torch")`` gives: sparse CSR tensors of the same entries on the device."""
    def mat(m):
        if m is None:
            return None
        m = m.tocsr()
        values = torch.from_numpy(m.data.astype(np.float64 if m.dtype.kind == "f" else np.int32))
        return torch.sparse_csr_tensor(torch.from_numpy(m.indptr.astype(np.int64)), torch.from_numpy(m.indices.astype(np.int64)), values,
                                       size=tuple(m.shape)).to(DEV)
    return api.Result(matrix=mat(r.matrix), ref_matrix=mat(r.ref_matrix), alt_counts=mat(r.alt_counts), ref_counts=mat(r.ref_counts),
                      unknown_counts=mat(r.unknown_counts), variants=list(r.variants), barcodes=list(r.barcodes), metrics=dict(r.metrics),
                      shape=r.shape, orient=r.orient)


@pytest.mark.parametrize("orient", ["variants", "cells"])
def test_the_device_tally_is_the_host_tally_and_the_model(orient):
    rng = np.random.default_rng(17)
    on_host = build(orient, n_var=90, n_cell=31, seed=9)
    on_dev = on_device(on_host)
    geno = BYTES[rng.choice(4, (90, 13), p=[0.3, 0.3, 0.25, 0.15])]
    pairs = random_pairs(rng, 70, 13)                                  # a pass of 64 and one of 6
    for prs, n_pairs in ((pairs, 70), (None, 78)):
        want = model_of(on_host, geno, np.stack(np.triu_indices(13, 1), axis=1) if prs is None else prs)
        a, b = api.doublet_tally(on_host, geno, prs), api.doublet_tally(on_dev, geno, prs)
        assert a.barcodes == b.barcodes == on_host.barcodes and a.donors == b.donors == list(range(13))
        assert np.array_equal(a.pairs, b.pairs) and b.pairs.shape == (n_pairs, 2)
        for f, k in FIELDS:
            t = getattr(b, f)
            assert isinstance(t, torch.Tensor) and t.device.type == "cuda" and t.dtype == torch.int64, f
            assert tuple(t.shape) == (31, n_pairs, 6), f
            assert np.array_equal(t.cpu().numpy(), want[k].astype(np.int64)), f
            assert np.array_equal(getattr(a, f), want[k].astype(np.int64)), f
        c = api.doublet_tally(on_dev, geno, prs, to="scipy")           # the same numbers copied to the host: the scipy path's arrays
        assert all(isinstance(getattr(c, f), np.ndarray) and getattr(c, f).dtype == np.int64 and np.array_equal(getattr(c, f), getattr(a, f))
                   for f, _ in FIELDS)
    one_host, one_dev = api.donor_tally(on_host, geno), api.donor_tally(on_dev, geno)
    x, y = api.assign_doublets(one_host, a, error=0.05, doublet_prior=0.2), api.assign_doublets(one_dev, b, error=0.05, doublet_prior=0.2)
    for f in ("kind", "best", "best_pair", "log_odds", "log_lik_pairs"):
        assert getattr(x, f).dtype == getattr(y, f).dtype and getattr(x, f).tobytes() == getattr(y, f).tobytes(), f
    assert x.kind.shape == (31,) and x.best.max() >= 0


def test_empty_lists_take_no_library_call():
    on_dev = on_device(build("cells", n_var=20, n_cell=6, seed=2))
    geno = np.zeros((20, 3), np.uint8)
    for t in (api.doublet_tally(on_dev, geno, []), api.doublet_tally(on_dev, geno[:, :1]), api.doublet_tally(on_dev, geno[:, :0])):
        assert all(isinstance(getattr(t, f), torch.Tensor) and tuple(getattr(t, f).shape) == (6, 0, 6) for f, _ in FIELDS)


@pytest.mark.parametrize("orient", ["cells", "variants"])
def test_the_authored_pool_comes_back_from_the_device(orient):
    r, geno, kind, donors, pairs = authored_pool()
    if orient == "variants":
        r = api.Result(matrix=r.matrix.T.tocsr(), ref_matrix=None, alt_counts=r.alt_counts.T.tocsr(), ref_counts=r.ref_counts.T.tocsr(),
                       unknown_counts=r.unknown_counts.T.tocsr(), variants=r.variants, barcodes=r.barcodes, metrics={}, shape=(len(r.variants), 12),
                       orient="variants")
    d = on_device(r)
    one, two = api.donor_tally(d, geno), api.doublet_tally(d, geno)
    a = api.assign_doublets(one, two)
    recovered(a, kind)
    host = api.assign_doublets(api.donor_tally(r, geno), api.doublet_tally(r, geno))
    agrees(a, {"kind": host.kind.tolist(), "best": host.best.tolist(), "best_pair": host.best_pair.tolist(), "log_odds": host.log_odds,
               "ll2": host.log_lik_pairs})
    agrees(a, scalar_model(api.donor_tally(r, geno), api.doublet_tally(r, geno), 0.01, 0.5))
