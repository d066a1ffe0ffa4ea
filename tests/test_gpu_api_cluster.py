"""``vartrix_amd.api.weighted_sum`` and ``cluster_donors`` on the GPU, on synthetic results: the sum of a torch result, computed on the
device, must be the model in Python integers of tests/csr_dense_util.py in both orientations of the result and of the sum (the
transpose path included); the planted pools of tests/test_api_cluster.py must come back from the device, with tables that reproduce the
scores exactly; and the int32 tables the device builds from given weighted reads may differ from numpy's by one unit at most."""
import numpy as np
import pytest
import torch

from tests.test_api_cluster import N_VAR, is_the_plant, model_of, planted_pool, random_tables
from tests.test_api_select import build
from tests.test_gpu_api_doublets import DEV, on_device
from vartrix_amd import api

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("orient", ["variants", "cells"])
@pytest.mark.parametrize("over", ["cells", "variants"])
def test_the_device_sum_is_the_host_sum_and_the_model(orient, over):
    rng = np.random.default_rng(19)
    on_host = build(orient, n_var=90, n_cell=31, seed=9)
    on_dev = on_device(on_host)
    n_rows, n_table = (31, 90) if over == "cells" else (90, 31)
    w_alt, w_ref = random_tables(rng, n_table, 70)         # a pass of 64 and one of 6
    for wa, wf in ((w_alt, w_ref), (w_alt, None), (None, w_ref)):
        want = model_of(on_host, wa, wf, over)
        got = api.weighted_sum(on_dev, wa, wf, over=over)
        assert isinstance(got, torch.Tensor) and got.device.type == "cuda" and got.dtype == torch.int64 and tuple(got.shape) == (n_rows, 70)
        assert np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(api.weighted_sum(on_host, wa, wf, over=over), want)
    tensors = [torch.from_numpy(w).to(DEV) for w in (w_alt, w_ref)]          # tables that are on the device already; the copy to the host
    got = api.weighted_sum(on_dev, *tensors, over=over, to="scipy")
    assert isinstance(got, np.ndarray) and np.array_equal(got, model_of(on_host, w_alt, w_ref, over))
    empty = api.weighted_sum(on_dev, w_alt[:, :0], over=over)                # no columns: no library call
    assert isinstance(empty, torch.Tensor) and tuple(empty.shape) == (n_rows, 0) and empty.dtype == torch.int64
    with pytest.raises(ValueError):
        api.weighted_sum(on_dev, np.zeros((n_table, 1025), np.int32), over=over)


def test_the_guard_holds_on_the_device():
    import scipy.sparse as sp
    alt = sp.csr_matrix((np.array([0xFFFFFFFF, 1, 5], np.uint32), np.array([0, 2, 1], np.int32), np.array([0, 2, 3], np.int32)), shape=(2, 3))
    ref = sp.csr_matrix((np.zeros(3, np.uint32), alt.indices.copy(), alt.indptr.copy()), shape=(2, 3))
    r = api.Result(matrix=alt.astype(np.float64), ref_matrix=None, alt_counts=alt, ref_counts=ref,
                   unknown_counts=ref.copy(), variants=["a", "b", "c"], barcodes=["x", "y"], metrics={}, shape=(2, 3), orient="cells")
    d = on_device(r)
    w = np.full((3, 2), -(1 << 31), np.int32)
    with pytest.raises(ValueError, match="2\\^63"):
        api.weighted_sum(d, w_alt=w)
    w[:] = -(1 << 31) + 1
    assert api.weighted_sum(d, w_alt=w).cpu().tolist() == [[-(1 << 63) + (1 << 32)] * 2, [-5 * ((1 << 31) - 1)] * 2]


@pytest.mark.parametrize("k,seed,orient", [(3, 0, "cells"), (5, 1, "variants")])
def test_the_planted_donors_come_back_from_the_device(k, seed, orient):
    on_host, plant = planted_pool(k, seed, orient)
    on_dev = on_device(on_host)
    c = api.cluster_donors(on_dev, k)
    print("k", k, "restart", c.restart, "rounds", c.n_iter, "log_lik", c.log_lik)
    for f, kind in (("labels", torch.int64), ("score", torch.int64), ("w_alt", torch.int32), ("w_ref", torch.int32), ("theta", torch.float64), ("resp", torch.float64)):
        t = getattr(c, f)
        assert isinstance(t, torch.Tensor) and t.device.type == "cuda" and t.dtype == kind, f
    labels, score, w_alt, w_ref = (getattr(c, f).cpu().numpy() for f in ("labels", "score", "w_alt", "w_ref"))
    assert is_the_plant(labels, plant) and labels[7] == -1 and labels[-1] == -1 and c.converged is True
    assert tuple(c.theta.shape) == (N_VAR, k) and tuple(c.resp.shape) == (len(plant), k) and not c.resp[[7, -1]].any()
    want = model_of(on_host, w_alt, w_ref, "cells")        # the fixed point, in integers, from the returned tables
    assert np.array_equal(score, want) and np.array_equal(labels, np.where(plant >= 0, np.argmax(want, axis=1), -1))
    again = api.cluster_donors(on_dev, k, to="scipy")      # the same call twice, and its copy to the host
    for f in ("labels", "resp", "score", "theta", "w_alt", "w_ref"):
        a = getattr(again, f)
        assert isinstance(a, np.ndarray) and a.tobytes() == getattr(c, f).cpu().numpy().tobytes(), f
    assert (again.log_lik, again.n_iter, again.converged, again.restart) == (c.log_lik, c.n_iter, c.converged, c.restart)
    host = api.cluster_donors(on_host, k)                  # the trajectories may differ by units of the tables; the partition may not
    assert is_the_plant(host.labels, plant)
    assert len(set(zip(host.labels.tolist(), labels.tolist()))) == k + 1
    g = api.pseudobulk(on_dev, c.labels)                   # a tensor of labels is taken as it is
    assert [int(x) for x in g.groups] == [-1] + list(range(k)) and g.group_sizes.tolist() == [2] + [200] * k


def test_the_device_tables_are_numpys_within_one_unit():
    """From one (A, R): S log(theta) carries a relative error near 2^-52 in either library, so the two can round differently only where
    the value lies next to a half: one unit at most, in any element.  How many elements differ is printed, not bounded."""
    rng = np.random.default_rng(23)
    q = api.RESP_SCALE
    A = rng.integers(0, 40 * q, (20_000, 8))
    R = rng.integers(0, 40 * q, (20_000, 8))
    A[:50], R[50:100] = 0, 0                               # theta at its smallest and at its largest
    A[100:110], R[100:110] = 1 << 40, 3                    # deep rows
    theta, w_alt, w_ref = api._m_step_tables(A, R, (1.0, 1.0))
    t_theta, t_alt, t_ref = api._m_step_tables(torch.from_numpy(A).to(DEV), torch.from_numpy(R).to(DEV), (1.0, 1.0))
    assert t_alt.dtype == t_ref.dtype == torch.int32 and t_theta.dtype == torch.float64 and w_alt.dtype == w_ref.dtype == np.int32
    for name, a, b in (("w_alt", w_alt, t_alt), ("w_ref", w_ref, t_ref)):
        diff = np.abs(a.astype(np.int64) - b.cpu().numpy().astype(np.int64))
        print(name, "elements that differ:", int((diff != 0).sum()), "of", diff.size, "largest difference", int(diff.max()))
        assert diff.max() <= 1
    assert np.all(w_alt <= 0) and np.all(w_ref < 0) and (w_alt == 0).any() and min(w_alt.min(), w_ref.min()) > -(1 << 30)
