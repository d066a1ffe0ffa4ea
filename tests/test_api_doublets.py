"""``vartrix_amd.api.doublet_tally`` and ``assign_doublets`` on the CPU: hand-built scipy ``Result``s of both orientations tallied against
the numpy model of tests/csr_geno_pair_util.py, the default list of pairs, a pair of a donor with itself against ``donor_tally``, the
likelihood and the decision bit for bit against a scalar-loop model written here, ties, cells without reads, argument errors, and an
authored pool of singlets and doublets (no random draws) whose every label must come back.  (The torch path runs on the device:
tests/test_gpu_api_doublets.py.)"""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.csr_geno_pair_util import model_pair_tally
from tests.csr_geno_util import BYTES, NONE
from tests.test_api_donors import cell_major
from tests.test_api_select import build
from vartrix_amd import abi, api, lib

FIELDS = (("alt", "sum_alt"), ("ref", "sum_ref"), ("n_obs", "n_obs"))


def model_of(r, geno, pairs):
    alt, ref = cell_major(r)
    return model_pair_tally(alt.indptr, alt.indices, alt.data, ref.data, geno, geno.shape[1], pairs)


def check(got, want, r, donors, pairs):
    assert isinstance(got, api.DoubletTally) and got.donors == donors and got.barcodes == r.barcodes
    assert isinstance(got.pairs, np.ndarray) and got.pairs.dtype == np.int64 and got.pairs.tolist() == np.asarray(pairs).reshape(-1, 2).tolist()
    for f, k in FIELDS:
        a = getattr(got, f)
        assert isinstance(a, np.ndarray) and a.dtype == np.int64 and a.shape == (len(r.barcodes), len(got.pairs), 6), f
        assert np.array_equal(a, want[k].astype(np.int64)), f


@pytest.mark.parametrize("orient", ["variants", "cells"])
def test_doublet_tally_of_a_scipy_result_is_the_model(orient):
    rng = np.random.default_rng(7)
    r = build(orient, n_var=23, n_cell=9, seed=3)
    geno = BYTES[rng.choice(4, (23, 6), p=[0.3, 0.3, 0.2, 0.2])]
    pairs = [[0, 1], [1, 0], [5, 5], [2, 4], [2, 4], [3, 0], [4, 5]]
    want = model_of(r, geno, pairs)
    assert all(want["sum_alt"][..., c].sum() + want["sum_ref"][..., c].sum() > 0 for c in range(6))
    check(api.doublet_tally(r, geno, pairs), want, r, list(range(6)), pairs)
    check(api.doublet_tally(r, geno.tolist(), np.asarray(pairs, np.uint32), donors=list("uvwxyz")), want, r, list("uvwxyz"), pairs)
    every = np.stack(np.triu_indices(6, 1), axis=1)        # the default: every a < b, in this order
    assert len(every) == 15 and every[:6].tolist() == [[0, 1], [0, 2], [0, 3], [0, 4], [0, 5], [1, 2]]
    check(api.doublet_tally(r, geno), model_of(r, geno, every), r, list(range(6)), every)
    assert abi.GENO_PAIR_CLASSES == 6 and abi.VTX_GENO_NONE == NONE


def test_argument_errors_and_empty_lists():
    rng = np.random.default_rng(9)
    r = build("cells", n_var=23, n_cell=9, seed=3)
    geno = BYTES[rng.choice(4, (23, 6))]
    for bad in ([[0, 6]], [[-1, 0]], [[0, 1, 2]], [0, 1], [[0.0, 1.0]]):
        with pytest.raises(ValueError):
            api.doublet_tally(r, geno, bad)
    with pytest.raises(ValueError, match=r"pair 2 is \(1, 6\)"):
        api.doublet_tally(r, geno, [[0, 1], [5, 5], [1, 6], [7, 0]])
    with pytest.raises(ValueError):
        api.doublet_tally(r, geno[:-1])                                # one row per variant
    with pytest.raises(ValueError):
        api.doublet_tally(r, geno, to="torch")                         # a scipy result stays on the host
    with pytest.raises(ValueError):
        api.doublet_tally(r, geno, to="numpy")
    wrong = geno.copy()
    wrong[4, 2] = 3
    with pytest.raises(ValueError, match="variant 4, donor 2"):
        api.doublet_tally(r, wrong)
    most = lib.load().vtx_csr_geno_pair_max()
    with pytest.raises(ValueError):
        api.doublet_tally(r, geno, np.zeros((most + 1, 2), np.int64))
    wide = np.zeros((23, 92), np.uint8)                                # 92 donors: 4 186 pairs
    assert 91 * 90 // 2 <= most < 92 * 91 // 2
    with pytest.raises(ValueError, match="pass `pairs`"):
        api.doublet_tally(r, wide)
    assert api.doublet_tally(r, wide, [[0, 91]]).alt.shape == (9, 1, 6)
    for t in (api.doublet_tally(r, geno, []), api.doublet_tally(r, geno, np.zeros((0, 2), np.int64)), api.doublet_tally(r, geno[:, :1]),
              api.doublet_tally(r, geno[:, :0])):
        assert t.alt.shape == t.ref.shape == t.n_obs.shape == (9, 0, 6) and t.alt.dtype == np.int64 and t.pairs.shape == (0, 2)


@pytest.mark.parametrize("orient", ["variants", "cells"])
def test_a_donor_paired_with_itself_carries_its_donor_tally(orient):
    rng = np.random.default_rng(13)
    r = build(orient, n_var=40, n_cell=12, seed=5)
    geno = BYTES[rng.choice(4, (40, 4), p=[0.3, 0.3, 0.2, 0.2])]
    one = api.donor_tally(r, geno)
    two = api.doublet_tally(r, geno, [[d, d] for d in range(4)])
    assert one.alt.sum() > 0
    for f, _ in FIELDS:
        assert np.array_equal(getattr(two, f)[..., [0, 2, 4, 5]], getattr(one, f)) and not getattr(two, f)[..., [1, 3]].any(), f


def scalar_model(singlets, doublets, error, prior):
    """``assign_doublets`` as the documentation states it, cell by cell and hypothesis by hypothesis in scalar loops."""
    p, q = (error, 0.5, 1.0 - error), (error, 0.25, 0.5, 0.75, 1.0 - error)
    n_cell, n_donors, n_pairs = singlets.alt.shape[0], singlets.alt.shape[1], doublets.alt.shape[1]
    out = {"kind": [], "best": [], "best_pair": [], "log_odds": [], "ll2": np.zeros((n_cell, n_pairs))}
    for i in range(n_cell):
        top1, best, informative = None, -1, 0
        for d in range(n_donors):
            ll = None
            for g in range(3):
                for term in (np.float64(singlets.alt[i, d, g]) * np.log(p[g]), np.float64(singlets.ref[i, d, g]) * np.log1p(-p[g])):
                    ll = term if ll is None else ll + term             # one sum, left to right
                informative += int(singlets.n_obs[i, d, g])
            if top1 is None or ll > top1:
                top1, best = ll, d
        top2, best_pair = None, -1
        for k in range(n_pairs):
            ll = None
            for c in range(5):
                for term in (np.float64(doublets.alt[i, k, c]) * np.log(q[c]), np.float64(doublets.ref[i, k, c]) * np.log1p(-q[c])):
                    ll = term if ll is None else ll + term
            out["ll2"][i, k] = ll
            if top2 is None or ll > top2:
                top2, best_pair = ll, k
        odds = (top2 + np.log(prior) - np.log(float(n_pairs))) - (top1 + np.log1p(-prior) - np.log(float(n_donors)))
        out["log_odds"].append(odds)
        out["best"].append(best if informative else -1)
        out["best_pair"].append(best_pair)
        out["kind"].append(-1 if not informative else int(odds > 0))
    return out


def agrees(a, m):
    assert a.kind.dtype == np.int8 and a.kind.tolist() == m["kind"]
    assert a.best.dtype == np.int64 and a.best.tolist() == m["best"]
    assert a.best_pair.dtype == np.int64 and a.best_pair.tolist() == m["best_pair"]
    assert a.log_odds.dtype == np.float64 and a.log_odds.tobytes() == np.asarray(m["log_odds"], np.float64).tobytes()
    assert a.log_lik_pairs.dtype == np.float64 and a.log_lik_pairs.tobytes() == m["ll2"].tobytes()


def test_assign_doublets_is_the_scalar_model_bit_for_bit():
    rng = np.random.default_rng(11)
    r = build("cells", n_var=60, n_cell=14, seed=5)
    geno = BYTES[rng.choice(4, (60, 5), p=[0.3, 0.3, 0.3, 0.1])]
    one, two = api.donor_tally(r, geno), api.doublet_tally(r, geno)
    assert two.pairs.shape == (10, 2)
    for error, prior in ((0.01, 0.5), (0.1, 0.1), (0.3, 0.9)):
        a = api.assign_doublets(one, two, error=error, doublet_prior=prior)
        agrees(a, scalar_model(one, two, error, prior))
        assert a.donors == one.donors and a.barcodes == one.barcodes and np.array_equal(a.pairs, two.pairs)
        assert np.array_equal(a.best, api.assign_donors(one, error=error).best)
    agrees(api.assign_doublets(one, two), scalar_model(one, two, 0.01, 0.5))      # the defaults
    for error in (0.0, 0.5, -0.1, 0.7):
        with pytest.raises(ValueError):
            api.assign_doublets(one, two, error=error)
    for prior in (0.0, 1.0, -0.2, 1.5):
        with pytest.raises(ValueError):
            api.assign_doublets(one, two, doublet_prior=prior)
    other = api.doublet_tally(build("cells", n_var=60, n_cell=13, seed=5), geno)
    with pytest.raises(ValueError):
        api.assign_doublets(one, other)                                # not the same cells


def tallies(alt1, ref1, alt2, ref2, pairs):
    a1, r1, a2, r2 = (np.asarray(a, np.int64) for a in (alt1, ref1, alt2, ref2))
    cells = ["c%d" % i for i in range(a1.shape[0])]
    donors = list(range(a1.shape[1]))
    return (api.DonorTally(alt=a1, ref=r1, n_obs=((a1 + r1) > 0).astype(np.int64), donors=donors, barcodes=cells),
            api.DoubletTally(alt=a2, ref=r2, n_obs=((a2 + r2) > 0).astype(np.int64), pairs=np.asarray(pairs, np.int64).reshape(-1, 2), donors=donors,
                             barcodes=cells))


def test_ties_go_to_the_lowest_index_and_cells_without_an_informative_read_are_minus_one():
    z4, z6 = [0, 0, 0, 0], [0, 0, 0, 0, 0, 0]
    # cell 0: the pairs 1 and 2 tie above pair 0, the donors 1 and 2 tie above donor 0; cell 1: reads at missing genotypes only; cell 2: no read
    alt1 = [[z4, [0, 0, 3, 0], [0, 0, 3, 0]], [[0, 0, 0, 5]] * 3, [z4] * 3]
    ref1 = [[[0, 0, 2, 0], z4, z4], [z4] * 3, [z4] * 3]
    alt2 = [[[3, 0, 0, 0, 0, 0], [0, 0, 0, 3, 0, 0], [0, 0, 0, 3, 0, 0]], [[0, 0, 0, 0, 0, 5]] * 3, [z6] * 3]
    ref2 = [[[1, 0, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0], [0, 0, 0, 1, 0, 0]], [z6] * 3, [z6] * 3]
    one, two = tallies(alt1, ref1, alt2, ref2, [[0, 1], [0, 2], [1, 2]])
    a = api.assign_doublets(one, two)
    agrees(a, scalar_model(one, two, 0.01, 0.5))
    assert a.best.tolist() == [1, -1, -1] and a.best_pair.tolist() == [1, 0, 0] and a.kind.tolist()[1:] == [-1, -1]
    assert not a.log_lik_pairs[1:].any()                               # class 5 contributes nothing
    assert a.log_odds[1] == a.log_odds[2] == (np.log(0.5) - np.log(3.0)) - (np.log1p(-0.5) - np.log(3.0))
    none = api.assign_doublets(one, tallies(alt1, ref1, np.zeros((3, 0, 6)), np.zeros((3, 0, 6)), [])[1])      # no pairs: no doublet
    assert none.best_pair.tolist() == [-1, -1, -1] and none.kind.tolist() == [0, -1, -1] and np.all(np.isneginf(none.log_odds))
    assert none.log_lik_pairs.shape == (3, 0)


N_VAR = 200
PAIRS = np.stack(np.triu_indices(4, 1), axis=1)


def authored_pool():
    """4 donors whose genotypes at variant v are the four base-3 digits of v (pairwise distinct columns), and 12 cells: each donor
    alone, each of the 6 pairs, two empty.  Every cell with reads has depth 4 at every variant: alt = 2 g for a singlet, the dosage for
    a doublet — the expectation of the model at error -> 0.  -> (Result cell-major, geno, planted kind, donor, pair)."""
    v = np.arange(N_VAR)
    geno = np.stack([(v // 3 ** d) % 3 for d in range(4)], axis=1).astype(np.uint8)
    assert all((geno[:, a] != geno[:, b]).sum() >= 100 for a, b in PAIRS)
    alt = np.zeros((12, N_VAR), np.int64)
    for d in range(4):
        alt[d] = 2 * geno[:, d]
    for k, (a, b) in enumerate(PAIRS):
        alt[4 + k] = geno[:, a].astype(np.int64) + geno[:, b]
    depth = np.zeros((12, N_VAR), np.int64)
    depth[:10] = 4
    covered = depth > 0
    pattern = sp.csr_matrix(covered.astype(np.int64))

    def mat(d):
        return sp.csr_matrix((d[covered].astype(np.uint32), pattern.indices.copy(), pattern.indptr.copy()), shape=(12, N_VAR))
    r = api.Result(matrix=mat(alt).astype(np.float64), ref_matrix=None, alt_counts=mat(alt), ref_counts=mat(depth - alt), unknown_counts=mat(depth * 0),
                   variants=["chr1_%d" % i for i in range(N_VAR)], barcodes=["BC%d-1" % i for i in range(12)], metrics={}, shape=(12, N_VAR),
                   orient="cells")
    kind = [0] * 4 + [1] * 6 + [-1] * 2
    return r, geno, kind, [0, 1, 2, 3], list(range(6))


def recovered(a, kind):
    assert a.kind.tolist() == kind
    assert a.best[:4].tolist() == [0, 1, 2, 3] and a.best[10:].tolist() == [-1, -1]
    assert a.best_pair[4:10].tolist() == list(range(6)) and np.array_equal(a.pairs, PAIRS)
    assert np.all(a.log_odds[:4] < 0) and np.all(a.log_odds[4:10] > 0)


def test_the_authored_pool_every_planted_label_comes_back():
    r, geno, kind, donors, pairs = authored_pool()
    one, two = api.donor_tally(r, geno), api.doublet_tally(r, geno)
    # first, with the scalar model: the planted hypothesis is the STRICT maximum of its kind, and the decision between the kinds is not a tie
    m = scalar_model(one, two, 0.01, 0.5)
    ll1 = api.assign_donors(one).log_lik
    for i in range(4):
        assert np.all(np.delete(ll1[i], i) < ll1[i, i]) and m["log_odds"][i] < 0
    for k in range(6):
        assert np.all(np.delete(m["ll2"][4 + k], k) < m["ll2"][4 + k, k]) and m["log_odds"][4 + k] > 0
    a = api.assign_doublets(one, two)
    agrees(a, m)
    recovered(a, kind)
