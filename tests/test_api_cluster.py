"""``vartrix_amd.api.weighted_sum`` and ``cluster_donors`` on the CPU: hand-built scipy ``Result``s of both orientations summed against
the model in Python integers of tests/csr_dense_util.py, the guard against a wrapped sum at its boundary, and genotype-free clustering
on planted pools — the labels must be the plant up to a renaming of the clusters, the returned tables must reproduce the returned
scores exactly, and the same call twice must give the same arrays.  (The torch path runs on the device: tests/test_gpu_api_cluster.py.)"""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.csr_dense_util import INT32_MAX, INT32_MIN, model_dense_sum
from tests.test_api_donors import cell_major
from tests.test_api_select import build
from vartrix_amd import api

N_VAR = 400
P_ALT = (0.01, 0.5, 0.99)                                  # the chance of an alt read by genotype


def planted_pool(k, seed, orient="cells", cells_per_donor=200):
    """k donors with genotypes uniform in {0, 1, 2} over 400 variants; cells_per_donor cells each, donor by donor in turn; a cell covers
    20 variants at depth 1 - 3, alt reads binomial by genotype; and two cells without reads: one without entries, one whose five entries
    hold no read.  -> (a scipy Result, the donor of every cell, -1 for the two)

    200 cells per donor: with 100 the host path recovered nine of these ten plants and put ONE cell of the tenth (k = 5, seed 1) into
    another cluster — the fault of a cell's 20 draws, which no number of restarts mends; with 150 again one cell of one plant; with 200
    all ten come back, the closest cell by 0.6 nats (k = 5) and 6 nats (k = 3).  The assertion stays every cell."""
    rng = np.random.default_rng([k, seed])
    geno = rng.integers(0, 3, (N_VAR, k))
    n_cell = k * cells_per_donor + 2
    plant = np.full(n_cell, -1, np.int64)
    empty = (7, n_cell - 1)
    plant[[c for c in range(n_cell) if c not in empty]] = np.arange(k * cells_per_donor) % k
    indptr, indices, alt, ref = [0], [], [], []
    for c in range(n_cell):
        if c == empty[0]:
            cols, depth = rng.choice(N_VAR, 5, replace=False), np.zeros(5, np.int64)
        elif c == empty[1]:
            cols, depth = np.zeros(0, np.int64), np.zeros(0, np.int64)
        else:
            cols, depth = rng.choice(N_VAR, 20, replace=False), rng.integers(1, 4, 20)
        cols = np.sort(cols)
        a = rng.binomial(depth, np.asarray(P_ALT)[geno[cols, max(plant[c], 0)]]) if len(cols) else depth
        indices.extend(cols)
        alt.extend(a)
        ref.extend(depth - a)
        indptr.append(len(indices))

    def mat(data):
        m = sp.csr_matrix((np.asarray(data, np.uint32), np.asarray(indices, np.int32), np.asarray(indptr, np.int32)), shape=(n_cell, N_VAR))
        if orient == "variants":
            m = m.T.tocsr()
            m.sort_indices()
        return m
    shape = (n_cell, N_VAR) if orient == "cells" else (N_VAR, n_cell)
    r = api.Result(matrix=mat(alt).astype(np.float64), ref_matrix=None, alt_counts=mat(alt), ref_counts=mat(ref), unknown_counts=mat(np.zeros(len(alt))),
                   variants=["chr1_%d" % i for i in range(N_VAR)], barcodes=["BC%d-1" % i for i in range(n_cell)], metrics={}, shape=shape, orient=orient)
    return r, plant


def is_the_plant(labels, plant):
    """The labels are the plant up to a renaming of the clusters, and -1 exactly where the plant is."""
    labels = np.asarray(labels)
    live = plant >= 0
    pairs = set(zip(plant[live].tolist(), labels[live].tolist()))
    k = len(set(plant[live].tolist()))
    return (np.array_equal(labels < 0, ~live) and len(pairs) == k and len({a for a, _ in pairs}) == k and len({b for _, b in pairs}) == k)


def model_of(r, w_alt, w_ref, over):
    alt, ref = cell_major(r)
    if over == "variants":
        alt, ref = alt.T.tocsr(), ref.T.tocsr()
    n_cols = (w_alt if w_alt is not None else w_ref).shape[1]
    return model_dense_sum(alt.indptr, alt.indices, alt.data, ref.data, w_alt, w_ref, n_cols)


def random_tables(rng, n_rows, n_cols, limit=1 << 24):
    return [rng.integers(-limit, limit, (n_rows, n_cols)).astype(np.int32) for _ in range(2)]


@pytest.mark.parametrize("orient", ["variants", "cells"])
@pytest.mark.parametrize("over", ["cells", "variants"])
def test_weighted_sum_of_a_scipy_result_is_the_model(orient, over):
    rng = np.random.default_rng(11)
    r = build(orient, n_var=23, n_cell=9, seed=3)
    n_rows, n_table = (9, 23) if over == "cells" else (23, 9)
    w_alt, w_ref = random_tables(rng, n_table, 7)
    for wa, wf in ((w_alt, w_ref), (w_alt, None), (None, w_ref)):
        got = api.weighted_sum(r, wa, wf, over=over)
        assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.shape == (n_rows, 7)
        assert np.array_equal(got, model_of(r, wa, wf, over))
    assert np.array_equal(api.weighted_sum(r, w_alt=w_alt, over=over, to="scipy"), model_of(r, w_alt, None, over))
    empty = api.weighted_sum(r, w_alt[:, :0], w_ref[:, :0], over=over)
    assert empty.shape == (n_rows, 0) and empty.dtype == np.int64


def test_weighted_sum_argument_errors():
    rng = np.random.default_rng(12)
    r = build("cells", n_var=23, n_cell=9, seed=3)
    w_alt, w_ref = random_tables(rng, 23, 4)
    for bad in (dict(), dict(w_alt=w_alt[:-1]), dict(w_alt=w_alt, w_ref=w_ref[:, :3]), dict(w_alt=w_alt.astype(np.int64)), dict(w_alt=w_alt.astype(np.float64)),
                dict(w_alt=w_alt, over="rows"), dict(w_alt=w_alt, to="numpy"), dict(w_alt=w_alt, to="torch"), dict(w_alt=w_alt, over="variants"),
                dict(w_alt=w_alt.reshape(-1))):
        with pytest.raises(ValueError):
            api.weighted_sum(r, **bad)


def test_the_guard_raises_at_the_boundary_and_not_one_below():
    """One cell with two entries of 2^32 - 1 and 1 alt reads: 2^32 reads in the largest row.  |w| = 2^31 reaches 2^63 exactly and is
    refused; |w| = 2^31 - 1 stays below and is summed, exactly."""
    alt = sp.csr_matrix((np.array([0xFFFFFFFF, 1, 5], np.uint32), np.array([0, 2, 1], np.int32), np.array([0, 2, 3], np.int32)), shape=(2, 3))
    ref = sp.csr_matrix((np.zeros(3, np.uint32), alt.indices.copy(), alt.indptr.copy()), shape=(2, 3))
    r = api.Result(matrix=alt.astype(np.float64), ref_matrix=None, alt_counts=alt, ref_counts=ref, unknown_counts=ref.copy(), variants=["a", "b", "c"],
                   barcodes=["x", "y"], metrics={}, shape=(2, 3), orient="cells")
    w = np.full((3, 2), INT32_MIN, np.int32)
    with pytest.raises(ValueError, match="2\\^63"):
        api.weighted_sum(r, w_alt=w)
    with pytest.raises(ValueError, match="2\\^63"):
        api.weighted_sum(r, w_ref=w)                       # the guard is computed from the row sums of alt + ref, whichever table is given
    w[:] = INT32_MIN + 1
    got = api.weighted_sum(r, w_alt=w)
    assert got.tolist() == [[-(1 << 32) * INT32_MAX] * 2, [-5 * INT32_MAX] * 2] and -(1 << 32) * INT32_MAX == -(1 << 63) + (1 << 32)
    w[:] = INT32_MAX
    assert api.weighted_sum(r, w_alt=w)[0, 0] == (1 << 63) - (1 << 32)
    over = np.full((2, 1), INT32_MIN, np.int32)            # by variant the largest row holds 2^32 - 1 reads: below the boundary
    assert api.weighted_sum(r, w_alt=over, over="variants")[:, 0].tolist() == [0xFFFFFFFF * INT32_MIN, 5 * INT32_MIN, INT32_MIN]


POOLS = {}


def pool(k, seed, orient="cells"):
    if (k, seed, orient) not in POOLS:
        POOLS[k, seed, orient] = planted_pool(k, seed, orient)
    return POOLS[k, seed, orient]


@pytest.mark.parametrize("seed", range(5))
@pytest.mark.parametrize("k", [3, 5])
def test_the_planted_donors_come_back(k, seed):
    r, plant = pool(k, seed)
    c = api.cluster_donors(r, k)
    print("k", k, "seed", seed, "restart", c.restart, "rounds", c.n_iter, "log_lik", c.log_lik)
    assert is_the_plant(c.labels, plant)
    assert c.labels[7] == -1 and c.labels[-1] == -1 and c.converged is True
    assert c.labels.dtype == np.int64 and c.score.dtype == np.int64 and c.w_alt.dtype == c.w_ref.dtype == np.int32 and c.theta.dtype == np.float64
    assert c.score.shape == c.resp.shape == (len(plant), k) and c.theta.shape == c.w_alt.shape == c.w_ref.shape == (N_VAR, k)
    assert c.barcodes == r.barcodes and c.variants == r.variants and 0 <= c.restart < 8 and 1 <= c.n_iter <= 100
    assert not c.resp[[7, -1]].any() and np.all(np.abs(c.resp[plant >= 0].sum(axis=1) - 1.0) <= k * 2.0 ** -16)      # each of k roundings moves a sum by half a unit at most


def test_the_returned_tables_give_the_returned_scores_exactly():
    """The fixed point, in integers: the model's sum of the result's CSR with w_alt / w_ref is ``score``, and its argmax ``labels``."""
    for orient in ("cells", "variants"):
        r, plant = pool(3, 0, orient)
        c = api.cluster_donors(r, 3)
        want = model_of(r, c.w_alt, c.w_ref, "cells")
        assert np.array_equal(c.score, want)
        assert np.array_equal(c.labels, np.where(plant >= 0, np.argmax(want, axis=1), -1))
        assert is_the_plant(c.labels, plant)
        assert np.array_equal(c.w_alt, np.rint(api.SCORE_SCALE * np.log(c.theta)).astype(np.int32))
        assert np.array_equal(c.w_ref, np.rint(api.SCORE_SCALE * np.log1p(-c.theta)).astype(np.int32))
        assert np.all(c.theta > 0) and np.all(c.theta < 1)


def test_the_same_call_twice_gives_identical_arrays():
    r, _ = pool(5, 1)
    a, b = api.cluster_donors(r, 5, n_init=3), api.cluster_donors(r, 5, n_init=3)
    for f in ("labels", "resp", "score", "theta", "w_alt", "w_ref"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    assert (a.log_lik, a.n_iter, a.converged, a.restart) == (b.log_lik, b.n_iter, b.converged, b.restart)
    other = api.cluster_donors(r, 5, n_init=3, seed=1)
    assert other.score.tobytes() != a.score.tobytes()      # the seed is what the restarts are drawn from


def test_the_labels_go_through_pseudobulk():
    r, plant = pool(3, 2)
    c = api.cluster_donors(r, 3)
    g = api.pseudobulk(r, c.labels)
    assert [int(x) for x in g.groups] == [-1, 0, 1, 2] and g.group_sizes.tolist() == [2, 200, 200, 200]
    alt = np.asarray(g.alt_counts.todense())
    A = api.weighted_sum(r, w_alt=(c.labels[:, None] == np.arange(3)).astype(np.int32), over="variants")
    assert alt.shape == (4, N_VAR) and np.array_equal(alt[1:].T, A)      # the fold of the alt counts is the M-step's sum with hard responsibilities


def test_one_cluster_and_the_limits_of_k():
    r, plant = pool(3, 3)
    c = api.cluster_donors(r, 1, n_init=2)
    assert c.labels.tolist() == np.where(plant >= 0, 0, -1).tolist() and c.converged and c.n_iter <= 2 and c.restart == 0
    assert np.array_equal(c.resp[:, 0], (plant >= 0).astype(np.float64)) and c.score.shape == (len(plant), 1)
    assert api.SCORE_SCALE == 2 ** 20 and api.RESP_SCALE == 2 ** 15
    for bad in (0, -1, 65, 1.5):
        with pytest.raises(ValueError):
            api.cluster_donors(r, bad)
    for bad in (dict(n_init=0), dict(max_iter=0), dict(prior=(0.0, 1.0)), dict(to="torch"), dict(to="numpy")):
        with pytest.raises(ValueError):
            api.cluster_donors(r, 2, **bad)
    few = api.cluster_donors(r, 3, n_init=1, max_iter=1)   # one round from a random start: not converged, and said so
    assert few.n_iter == 1 and few.converged is False
    assert api.cluster_donors(r, 64, n_init=1, max_iter=2).score.shape == (len(plant), 64)
