"""vtx_csr_geno_tally on the GPU, driven directly with synthetic CSRs and genotype tables in torch device tensors: the twelve numbers of
every (row, donor) pair against the numpy model of tests/csr_geno_util.py on the smallest shapes at which the kernel can go wrong, bit
for bit; a cross-check against vtx_csr_row_stats on every case and every donor; every subset of NULL outputs; then what the library must
DECLINE — bad genotype bytes, bad arrays, donor counts out of range are refused before a byte is written.  Every refused input is refused
by the check kernels or on the host, which read within the given lengths only: nothing here provokes a fault."""
import itertools

import numpy as np
import pytest
import torch

from tests.csr_geno_util import NAMES, NONE, cases, model_geno_tally, random_counts, random_table
from tests.test_gpu_csr_ops import dev, filled, row_stats, untouched, words
from tests.test_gpu_csr_transpose import random_csr
from vartrix_amd import abi, lib
from vartrix_amd.abi import default_config

pytestmark = pytest.mark.gpu

WIDE = ("sum_alt", "sum_ref")


@pytest.fixture(scope="module")
def ctx():
    with lib.Context(default_config(n_barcodes=4)) as c:      # no batch, no run: the context gives the device, the stream, the work space
        yield c


@pytest.fixture(scope="module")
def CASES():
    """Every case with the model's answer, computed once and shared."""
    return [(c, model_geno_tally(c[1], c[2], *c[4], c[5], c[6])) for c in cases()]


def tally(ctx, indptr, indices, n_minor, counts, geno, n_donors, names=NAMES, nnz=None, n_alloc=None, expect=None, no_geno=False):
    """-> dict of outputs as unsigned words, n_major x n_donors x 4.  ``n_alloc``: donors the outputs are made for (a refused call:
    any size does).  ``expect``: the status the call must fail with; the message comes back."""
    n_major = len(indptr) - 1
    nnz = len(indices) if nnz is None else nnz
    d = [dev(np.asarray(indptr, np.uint64))] + [dev(np.asarray(a, np.uint32)) for a in (indices, *counts)]
    d_geno = dev(np.asarray(geno, np.uint8).reshape(-1))
    n = n_major * (n_donors if n_alloc is None else n_alloc) * 4
    out = {k: filled(n, k in WIDE) for k in NAMES}
    torch.cuda.synchronize()
    args = (n_major, n_minor, nnz, *[t.data_ptr() for t in d], 0 if no_geno else d_geno.data_ptr(), n_donors,
            {k: out[k].data_ptr() for k in names})
    if expect is not None:
        with pytest.raises(lib.VtxError) as e:
            ctx.csr_geno_tally(*args)
        assert e.value.status == expect, str(e.value)
        untouched(out.values())
        return str(e.value)
    ctx.csr_geno_tally(*args)
    untouched([out[k] for k in NAMES if k not in names])
    return {k: words(out[k], n, k in WIDE).reshape(n_major, n_donors, 4) for k in names}


def same(got, want, names=NAMES):
    for k in names:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def test_every_case_against_the_model_and_against_row_stats(ctx, CASES):
    assert len(CASES) >= 20
    for (name, indptr, indices, n_minor, counts, geno, n_donors), want in CASES:
        got = tally(ctx, indptr, indices, n_minor, counts, geno, n_donors)
        same(got, want)
        if len(indptr) > 1:                                # over the classes, every donor sees every entry of the row once
            stats = row_stats(ctx, indptr, indices, n_minor, *counts, np.zeros(len(indices), np.uint32))
            for d in range(n_donors):
                assert np.array_equal(got["sum_alt"][:, d].sum(axis=1, dtype=np.uint64), stats["sum_alt"]), (name, d)
                assert np.array_equal(got["sum_ref"][:, d].sum(axis=1, dtype=np.uint64), stats["sum_ref"]), (name, d)
                assert np.array_equal(got["n_obs"][:, d].sum(axis=1, dtype=np.uint32), stats["n_alt"] + stats["n_ref"] - stats["n_both"]), (name, d)
        if name.startswith("sums_past_2_32"):
            assert got["sum_alt"].max() > 1 << 32 and got["sum_ref"].max() > 1 << 32
        if name == "one_donor_all_missing":
            assert not got["sum_alt"][:, 2, :3].any() and got["sum_alt"][:, 2, 3].any()


def test_more_rows_than_one_block_two_passes_and_the_same_bytes_twice(ctx):
    """300 rows: 75 blocks of four wavefronts; 70 donors: a pass of 64 and one of 6."""
    rng = np.random.default_rng(41)
    indptr, indices = random_csr(rng, 300, 600, 9000)
    counts = random_counts(rng, 9000)
    geno = random_table(rng, 600, 70)
    want = model_geno_tally(indptr, indices, *counts, geno, 70)
    a, b = (tally(ctx, indptr, indices, 600, counts, geno, 70) for _ in range(2))
    same(a, want)
    assert all(a[k].tobytes() == b[k].tobytes() for k in NAMES)


def test_every_subset_of_null_outputs_leaves_those_buffers_untouched(ctx, CASES):
    (name, indptr, indices, n_minor, counts, geno, n_donors), want = CASES[5]
    for n in range(len(NAMES) + 1):
        for names in itertools.combinations(NAMES, n):
            got = tally(ctx, indptr, indices, n_minor, counts, geno, n_donors, names)      # (tally checks the buffers that were not passed)
            same(got, want, names)


def test_refusals_write_nothing_and_leave_the_context_usable(ctx, CASES):
    (name, indptr, indices, n_minor, counts, geno, n_donors), want = CASES[3]
    assert n_donors == 5 and len(indices) > 100
    top = lib.load().vtx_csr_geno_max()

    def after():
        same(tally(ctx, indptr, indices, n_minor, counts, geno, n_donors), want)
    INVAL, UNSUP = abi.VTX_E_INVAL, abi.VTX_E_UNSUPPORTED
    two = geno.copy()
    two[30, 1], two[7, 3] = 3, 254                         # two offenders: the lower flat position is named
    order, index = indptr.copy(), indices.copy()
    order[3] = order[4] + np.uint64(1)
    index[100] = n_minor
    table = [(indptr, indices, two, n_donors, INVAL, "variant 7, donor 3"), (indptr, indices, geno, 0, INVAL, "no donors"),
             (indptr, indices, geno, top + 1, UNSUP, "at most"), (order, indices, geno, n_donors, INVAL, "indptr decreases"),
             (indptr, index, geno, n_donors, INVAL, "an index >= n_minor")]
    for ptr, idx, gen, nd, status, reason in table:
        msg = tally(ctx, ptr, idx, n_minor, counts, gen, nd, n_alloc=n_donors, expect=status)
        assert reason in msg, msg
        after()
    assert "32-bit" in tally(ctx, indptr, indices, n_minor, counts, geno, n_donors, nnz=1 << 32, expect=UNSUP)      # refused on the host, nothing is read
    after()
    assert "null" in tally(ctx, indptr, indices, n_minor, counts, geno, n_donors, expect=INVAL, no_geno=True)      # no table
    after()
    d = [dev(np.asarray(indptr, np.uint64))] + [dev(np.asarray(a, np.uint32)) for a in (indices, *counts)] + [dev(geno.reshape(-1))]
    torch.cuda.synchronize()
    rc = ctx._L.vtx_csr_geno_tally(ctx._h, len(indptr) - 1, n_minor, len(indices), *[t.data_ptr() for t in d], n_donors, None)      # no outputs
    assert rc == INVAL
    after()


def test_phase_times_are_reported(ctx):
    rng = np.random.default_rng(43)
    indptr, indices = random_csr(rng, 300, 600, 40_000)
    tally(ctx, indptr, indices, 600, random_counts(rng, 40_000), random_table(rng, 600, 20), 20)
    ms = ctx.csr_ms()
    assert ms["check"] > 0 and ms["place"] > 0 and ms["sort"] == 0 and ms["offsets"] == 0 and sum(ms.values()) < 100
