"""vtx_csr_group_plan and vtx_csr_group_sum on the GPU, driven directly with synthetic CSRs in torch device tensors: the folded matrix
against the numpy model of tests/csr_group_util.py on the smallest shapes at which the kernels can go wrong, two cross-checks against
vtx_csr_row_stats and vtx_csr_select on every case, every subset of NULL outputs; then what the library must DECLINE — bad labels, bad
arrays, group counts out of range, and allocations made for another fold are refused before a byte is written.  Every refused input is
refused by the check kernels or on the host, which read within the given lengths only: nothing here provokes a fault."""
import itertools

import numpy as np
import pytest
import torch

from tests.csr_group_util import NAMES, NONE, cases, model_group_sum
from tests.csr_ops_util import COUNTS, SUMS, random_counts
from tests.test_gpu_csr_ops import dev, filled, row_stats, select, untouched, words
from tests.test_gpu_csr_transpose import random_csr
from vartrix_amd import abi, lib
from vartrix_amd.abi import default_config

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with lib.Context(default_config(n_barcodes=4)) as c:      # no batch, no run: the context gives the device, the stream, the work space
        yield c


@pytest.fixture(scope="module")
def W(ctx):
    return lib.load().vtx_csr_group_window()


@pytest.fixture(scope="module")
def CASES(W):
    """Every case with the model's answer, computed once and shared."""
    return [(c, model_group_sum(c[1], c[2], *c[4], c[5], c[6])) for c in cases(W)]


def fold(ctx, indptr, indices, n_minor, counts, group, n_groups, names=NAMES, nnz=None, nnz_out=None, n_alloc=None, expect=None,
         plan_expect=None):
    """plan + sum -> (nnz_out, dict of outputs as unsigned words).  ``nnz_out``: passed to the sum INSTEAD of the plan's (the outputs
    keep the plan's size, or ``n_alloc`` when the plan is refused too).  ``expect`` / ``plan_expect``: the status the sum / the plan
    must fail with; the message comes back."""
    n_major = len(indptr) - 1
    nnz = len(indices) if nnz is None else nnz
    d = [dev(np.asarray(indptr, np.uint64))] + [dev(np.asarray(a, np.uint32)) for a in (indices, *counts, group)]
    torch.cuda.synchronize()
    head = (n_major, n_minor, nnz, d[0].data_ptr(), d[1].data_ptr())
    if plan_expect is not None:
        with pytest.raises(lib.VtxError) as e:
            ctx.csr_group_plan(*head, d[5].data_ptr(), n_groups)
        assert e.value.status == plan_expect, str(e.value)
        planned = n_alloc or 0
    else:
        planned = ctx.csr_group_plan(*head, d[5].data_ptr(), n_groups)
    out = {"indptr": filled(n_major + 1, True), "indices": filled(planned, False)}
    out.update({k: filled(planned, k in SUMS) for k in NAMES})
    torch.cuda.synchronize()
    args = (*head, *[t.data_ptr() for t in d[2:5]], d[5].data_ptr(), n_groups, planned if nnz_out is None else nnz_out,
            out["indptr"].data_ptr(), out["indices"].data_ptr(), {k: out[k].data_ptr() for k in names})
    if expect is not None:
        with pytest.raises(lib.VtxError) as e:
            ctx.csr_group_sum(*args)
        assert e.value.status == expect, str(e.value)
        untouched(out.values())
        return str(e.value)
    ctx.csr_group_sum(*args)
    untouched([out[k] for k in NAMES if k not in names])
    got = {"indptr": words(out["indptr"], n_major + 1, True), "indices": words(out["indices"], planned, False)}
    got.update({k: words(out[k], planned, k in SUMS) for k in names})
    return planned, got


def same(got, want, names=("indptr", "indices") + NAMES):
    for k in names:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def test_every_case_against_the_model_and_against_row_stats_and_select(ctx, CASES):
    assert len(CASES) >= 20
    for (name, indptr, indices, n_minor, counts, group, n_groups), want in CASES:
        n_out, got = fold(ctx, indptr, indices, n_minor, counts, group, n_groups)
        assert n_out == len(want["indices"]), name
        same(got, want)
        lens = np.diff(indptr.astype(np.int64))
        # all labels 0, one group: vtx_csr_row_stats' numbers for the rows that have entries
        n_one, one = fold(ctx, indptr, indices, n_minor, counts, np.zeros(n_minor, np.uint32), 1)
        stats = row_stats(ctx, indptr, indices, n_minor, *counts)
        assert n_one == int((lens > 0).sum()) and not one["indices"].any(), name
        for k in NAMES:
            assert np.array_equal(one[k], stats[k][lens > 0]), (name, k)
        # the payloads summed over each output row: vtx_csr_row_stats of the matrix without the columns that are left out
        _, sel = select(ctx, indptr, indices, n_minor, None, group != NONE, list(counts), ids=False)
        kept = row_stats(ctx, sel["indptr"], sel["indices"], max(int((group != NONE).sum()), 1), *sel["payloads"])
        rows = np.repeat(np.arange(len(lens)), np.diff(got["indptr"].astype(np.int64)))
        for k in NAMES:
            total = np.zeros(len(lens), np.uint64)
            np.add.at(total, rows, got[k].astype(np.uint64))
            assert np.array_equal(total, kept[k].astype(np.uint64)), (name, k)
        if name == "every_cell_left_out":
            assert n_out == 0 and not got["indptr"].any()
        if name == "identity":                             # one group per column on a canonical CSR: the matrix itself
            assert np.array_equal(got["indptr"], indptr) and np.array_equal(got["indices"], indices)
            assert all(np.array_equal(got[k], c) for k, c in zip(SUMS, counts)) and np.all(got["n_entries"] == 1)
        if name == "a_group_without_cells":
            assert not np.isin(got["indices"], [1, 4]).any()
        if name == "sums_past_2_32":
            assert got["sum_alt"].max() > 1 << 32 and got["sum_unk"].max() > 1 << 32
        if name.startswith("groups_") and n_groups > 64:   # one row has both sides of every 64-bin step and of every window edge
            full = int(np.argmax(lens == n_minor))
            row = got["indices"][int(got["indptr"][full]):int(got["indptr"][full + 1])]
            assert all(e - 1 in row and e in row for e in range(64, n_groups, 64)), name


def test_more_rows_than_one_block_and_the_same_bytes_twice(ctx, W):
    """300 rows: 75 blocks of four wavefronts and one more for the last offset; labels over two windows."""
    rng = np.random.default_rng(31)
    indptr, indices = random_csr(rng, 300, 600, 9000)
    counts = random_counts(rng, 9000)
    group = rng.integers(0, W + 40, 600, dtype=np.uint64).astype(np.uint32)
    group[rng.random(600) < 0.1] = NONE
    want = model_group_sum(indptr, indices, *counts, group, W + 40)
    a, b = (fold(ctx, indptr, indices, 600, counts, group, W + 40) for _ in range(2))
    same(a[1], want)
    assert a[0] == b[0] and all(a[1][k].tobytes() == b[1][k].tobytes() for k in a[1])


def test_every_subset_of_null_outputs_leaves_those_buffers_untouched(ctx, CASES):
    (name, indptr, indices, n_minor, counts, group, n_groups), want = CASES[4]
    for n in range(len(NAMES) + 1):
        for names in itertools.combinations(NAMES, n):
            _, got = fold(ctx, indptr, indices, n_minor, counts, group, n_groups, names)      # (fold checks the buffers that were not passed)
            same(got, want, ("indptr", "indices") + names)


def test_refusals_write_nothing_and_leave_the_context_usable(ctx, CASES):
    (name, indptr, indices, n_minor, counts, group, n_groups), want = CASES[5]
    n_out = len(want["indices"])
    assert n_out > 1
    top = lib.load().vtx_csr_group_max()

    def after():
        same(fold(ctx, indptr, indices, n_minor, counts, group, n_groups)[1], want)
    INVAL, UNSUP = abi.VTX_E_INVAL, abi.VTX_E_UNSUPPORTED
    equal, other = group.copy(), group.copy()
    equal[[250, 40]] = n_groups                            # two offenders: the lowest column is named
    other[7] = 0xFFFFFFFE
    order, index = indptr.copy(), indices.copy()
    order[3] = order[4] + np.uint64(1)
    index[100] = n_minor
    table = [(indptr, indices, equal, n_groups, INVAL, "column 40"), (indptr, indices, other, n_groups, INVAL, "column 7"),
             (indptr, indices, group, 0, INVAL, "no groups"), (indptr, indices, group, top + 1, UNSUP, "at most"),
             (order, indices, group, n_groups, INVAL, "indptr decreases"), (indptr, index, group, n_groups, INVAL, "an index >= n_minor")]
    for ptr, idx, grp, ng, status, reason in table:
        msg = fold(ctx, ptr, idx, n_minor, counts, grp, ng, n_alloc=n_out, nnz_out=n_out, plan_expect=status, expect=status)
        assert reason in msg, msg
        after()
    for wrong in (n_out + 1, n_out - 1):                   # arrays made for another fold
        assert "vtx_csr_group_plan" in fold(ctx, indptr, indices, n_minor, counts, group, n_groups, nnz_out=wrong, expect=INVAL)
        after()
    d_ptr, d_idx = dev(indptr), dev(indices)
    torch.cuda.synchronize()
    with pytest.raises(lib.VtxError) as e:                 # positions are 32-bit; refused on the host, nothing is read
        ctx.csr_group_plan(len(indptr) - 1, n_minor, 1 << 32, d_ptr.data_ptr(), d_idx.data_ptr(), d_idx.data_ptr(), 3)
    assert e.value.status == UNSUP
    with pytest.raises(lib.VtxError) as e:                 # no labels
        ctx.csr_group_plan(len(indptr) - 1, n_minor, len(indices), d_ptr.data_ptr(), d_idx.data_ptr(), 0, 3)
    assert e.value.status == INVAL
    after()


def test_phase_times_are_reported(ctx, W):
    rng = np.random.default_rng(33)
    indptr, indices = random_csr(rng, 300, 600, 40_000)
    counts = random_counts(rng, 40_000)
    fold(ctx, indptr, indices, 600, counts, rng.integers(0, 20, 600), 20)
    ms = ctx.csr_ms()
    assert ms["check"] > 0 and ms["sort"] > 0 and ms["place"] > 0 and ms["offsets"] == 0 and sum(ms.values()) < 100
