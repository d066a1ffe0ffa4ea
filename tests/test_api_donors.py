"""``vartrix_amd.api.read_genotypes``, ``donor_tally`` and ``assign_donors`` on the CPU: genotype tables from VCFs authored here, hand-built
scipy ``Result``s of both orientations tallied against the numpy model of tests/csr_geno_util.py, the likelihood bit for bit from the
expression the documentation states, and a small authored pool whose cells must all come back to their donors.  (The torch path runs on
the device: tests/test_gpu_api_donors.py.)"""
import gzip

import numpy as np
import pytest

from tests.csr_geno_util import BYTES, NONE, model_geno_tally
from tests.test_api_select import build
from vartrix_amd import abi, api

HEAD = "##fileformat=VCFv4.2\n##contig=<ID=chr1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tdonor_a\tdonor_b\tdonor_c\n"


def record(chrom, pos, fmt, *samples):
    fields = [chrom, str(pos), ".", "A", "C", ".", "PASS", "."] + ([fmt, *samples] if fmt is not None else [])
    return "\t".join(fields) + "\n"


VCF = HEAD + "".join([
    record("chr1", 11, "GT", "0/0", "0|1", "1/1"),                     # chr1_10: unphased, phased
    record("chr1", 21, "GT:DP", "1|0:7", "./.:0", "1|1:3"),            # chr1_20: a second field; a call without alleles
    record("chr1", 31, "DP:GT", "4:./1", "9:1", "2:0/2"),              # chr1_30: GT is not the first key; half a call, a haploid call, allele 2
    record("chr1", 41, None),                                          # chr1_40: a record without FORMAT
    record("chr1", 51, "DP", "4", "9", "2"),                           # chr1_50: a FORMAT without GT
    record("chr1", 61, "GT", "0/1", "0/1", "0/1"),                     # chr1_60: twice in the file
    record("chr1", 61, "GT", "1/1", "1/1", "1/1"),
    record("chr1", 71, "GT", "1/1", "0/0", "0/1"),                     # chr1_70: twice among the variants
    record("chr2", 11, "GT", "0/0", "0/0", "."),                       # chr2_10: another contig, the same position
    record("chr9", 5, "GT", "1/1", "1/1", "1/1"),                      # no variant of the run
])
VARIANTS = ["chr1_10", "chr1_20", "chr1_30", "chr1_40", "chr1_50", "chr1_60", "chr1_70", "chr1_70", "chr2_10", "chr3_99"]
N = NONE
WANT = [[0, 1, 2], [1, N, 2], [N, N, N], [N, N, N], [N, N, N], [N, N, N], [N, N, N], [N, N, N], [0, 0, N], [N, N, N]]


@pytest.mark.parametrize("gz", [False, True])
def test_read_genotypes(tmp_path, gz):
    path = tmp_path / ("donors.vcf.gz" if gz else "donors.vcf")
    if gz:
        with gzip.open(path, "wt") as f:
            f.write(VCF)
    else:
        path.write_text(VCF)
    geno, donors = api.read_genotypes(str(path), VARIANTS)
    assert donors == ["donor_a", "donor_b", "donor_c"] and geno.dtype == np.uint8 and geno.shape == (len(VARIANTS), 3)
    assert geno.tolist() == WANT
    one, _ = api.read_genotypes(path, ["chr1_70", "chr1_10"])          # the order is the variants', a name that is there once is read
    assert one.tolist() == [[2, 0, 1], [0, 1, 2]]
    none, donors = api.read_genotypes(path, [])
    assert none.shape == (0, 3) and donors == ["donor_a", "donor_b", "donor_c"]


def cell_major(r):
    alt, ref = r.alt_counts.tocsr(), r.ref_counts.tocsr()
    if r.orient == "variants":
        alt, ref = alt.T.tocsr(), ref.T.tocsr()
    assert np.array_equal(alt.indptr, ref.indptr) and np.array_equal(alt.indices, ref.indices)
    return alt, ref


def model_of(r, geno):
    alt, ref = cell_major(r)
    return model_geno_tally(alt.indptr, alt.indices, alt.data, ref.data, geno, geno.shape[1])


def check(got, want, r, donors):
    assert isinstance(got, api.DonorTally) and got.donors == donors and got.barcodes == r.barcodes
    for f, k in (("alt", "sum_alt"), ("ref", "sum_ref"), ("n_obs", "n_obs")):
        a = getattr(got, f)
        assert isinstance(a, np.ndarray) and a.dtype == np.int64 and a.shape == (len(r.barcodes), len(donors), 4), f
        assert np.array_equal(a, want[k].astype(np.int64)), f


@pytest.mark.parametrize("orient", ["variants", "cells"])
def test_donor_tally_of_a_scipy_result_is_the_model(orient):
    rng = np.random.default_rng(7)
    r = build(orient, n_var=23, n_cell=9, seed=3)
    geno = BYTES[rng.choice(4, (23, 6), p=[0.3, 0.3, 0.2, 0.2])]
    want = model_of(r, geno)
    assert want["sum_alt"][..., :3].sum() > 0 and want["n_obs"][..., 3].sum() > 0
    check(api.donor_tally(r, geno), want, r, list(range(6)))
    check(api.donor_tally(r, geno.tolist(), donors=list("uvwxyz")), want, r, list("uvwxyz"))
    with pytest.raises(ValueError):
        api.donor_tally(r, geno[:-1])                                  # one row per variant
    with pytest.raises(ValueError):
        api.donor_tally(r, geno, donors=["a"])
    with pytest.raises(ValueError):
        api.donor_tally(r, geno, to="torch")                           # a scipy result stays on the host
    bad = geno.copy()
    bad[4, 2] = 3
    with pytest.raises(ValueError, match="variant 4, donor 2"):
        api.donor_tally(r, bad)


def test_donor_tally_reads_a_vcf(tmp_path):
    r = build(n_var=7)
    path = tmp_path / "donors.vcf"
    path.write_text(HEAD + "".join(record("chr1", i + 1, "GT", *gts) for i, gts in
                                   enumerate([("0/0", "0/1", "1/1"), ("1/1", "0/0", "./."), ("0/1", "0/1", "0/0"), ("1|1", "0|0", "1|0")])))
    geno, donors = api.read_genotypes(path, r.variants)
    assert geno[:4].tolist() == [[0, 1, 2], [2, 0, N], [1, 1, 0], [2, 0, 1]] and np.all(geno[4:] == N)
    check(api.donor_tally(r, str(path)), model_of(r, geno), r, donors)


def expression(alt, ref, error):
    """What the documentation of assign_donors states, written here on its own."""
    alt, ref = alt.astype(np.float64), ref.astype(np.float64)
    p = (error, 0.5, 1.0 - error)
    return (alt[..., 0] * np.log(p[0]) + ref[..., 0] * np.log1p(-p[0]) + alt[..., 1] * np.log(p[1]) + ref[..., 1] * np.log1p(-p[1])
            + alt[..., 2] * np.log(p[2]) + ref[..., 2] * np.log1p(-p[2]))


def test_assign_donors_is_the_stated_expression_bit_for_bit():
    rng = np.random.default_rng(11)
    r = build("cells", n_var=40, n_cell=12, seed=5)
    geno = BYTES[rng.choice(4, (40, 4), p=[0.3, 0.3, 0.3, 0.1])]
    t = api.donor_tally(r, geno)
    for error in (0.01, 0.1, 0.3):
        a = api.assign_donors(t, error=error)
        ll = expression(t.alt, t.ref, error)
        assert a.log_lik.dtype == np.float64 and a.log_lik.tobytes() == ll.tobytes()
        assert a.best.dtype == np.int64 and np.array_equal(a.best, np.argmax(ll, axis=1))
        top = np.sort(ll, axis=1)
        assert a.margin.tobytes() == (top[:, -1] - top[:, -2]).tobytes() and a.donors == t.donors and a.barcodes == t.barcodes
    b = api.assign_donors(r, geno, error=0.1)                          # a Result and its genotypes: the same
    assert b.log_lik.tobytes() == expression(t.alt, t.ref, 0.1).tobytes()
    for error in (0.0, 0.5, -0.1, 0.7):
        with pytest.raises(ValueError):
            api.assign_donors(t, error=error)
    with pytest.raises(ValueError):
        api.assign_donors(r)


def tally_of(alt, ref, n_obs=None):
    alt, ref = np.asarray(alt, np.int64), np.asarray(ref, np.int64)
    n_obs = ((alt + ref) > 0).astype(np.int64) if n_obs is None else np.asarray(n_obs, np.int64)
    return api.DonorTally(alt=alt, ref=ref, n_obs=n_obs, donors=list(range(alt.shape[1])), barcodes=["c%d" % i for i in range(alt.shape[0])])


def test_ties_cells_without_reads_and_one_donor():
    z = [0, 0, 0, 0]
    # cell 0: donors 1 and 2 tie above donor 0 -> 1; cell 1: no read at a genotyped variant, only at missing ones -> -1; cell 2: donor 2
    alt = [[z, [0, 0, 3, 0], [0, 0, 3, 0]], [[0, 0, 0, 5], [0, 0, 0, 5], [0, 0, 0, 5]], [[4, 0, 0, 0], [0, 4, 0, 0], [0, 0, 4, 0]]]
    ref = [[[0, 0, 2, 0], z, z], [z, z, z], [z, z, z]]
    a = api.assign_donors(tally_of(alt, ref))
    assert a.best.tolist() == [1, -1, 2] and a.margin[0] == 0.0 and a.margin[1] == 0.0 and a.margin[2] > 0
    assert not a.log_lik[1].any()                                      # missing genotypes contribute nothing
    one = api.assign_donors(tally_of([[[1, 0, 0, 0]], [z]], [[z], [z]]))
    assert one.best.tolist() == [0, -1] and np.all(np.isposinf(one.margin)) and one.log_lik.shape == (2, 1)


def test_a_small_pool_every_cell_goes_back_to_its_donor():
    """3 donors x 40 variants with distinct genotypes, 30 cells whose reads are drawn from one donor each."""
    import scipy.sparse as sp
    rng = np.random.default_rng(2026)
    n_var, n_cell, error = 40, 30, 0.01
    geno = np.stack([np.arange(n_var) % 3, (np.arange(n_var) // 3) % 3, (np.arange(n_var) // 9 + 1) % 3], axis=1).astype(np.uint8)
    assert all((geno[:, a] != geno[:, b]).sum() >= 20 for a, b in ((0, 1), (0, 2), (1, 2)))
    truth = np.arange(n_cell) % 3
    p_alt = np.array([error, 0.5, 1 - error])
    covered = rng.random((n_cell, n_var)) < 0.6
    depth = rng.integers(1, 5, (n_cell, n_var)) * covered
    alt = rng.binomial(depth, p_alt[geno[:, truth].T])
    ref = depth - alt
    pattern = sp.csr_matrix(covered.astype(np.int64))

    def mat(d):
        return sp.csr_matrix((d[covered].astype(np.uint32), pattern.indices.copy(), pattern.indptr.copy()), shape=(n_cell, n_var))
    r = api.Result(matrix=mat(alt).astype(np.float64), ref_matrix=None, alt_counts=mat(alt), ref_counts=mat(ref), unknown_counts=mat(depth * 0),
                   variants=["chr1_%d" % i for i in range(n_var)], barcodes=["BC%d-1" % i for i in range(n_cell)], metrics={}, shape=(n_cell, n_var),
                   orient="cells")
    a = api.assign_donors(r, geno, error=error)
    assert a.best.tolist() == truth.tolist() and np.all(a.margin > 0)
    assert abi.VTX_GENO_NONE == NONE
