"""vtx_csr_geno_pair_tally on the GPU, driven directly with synthetic CSRs, genotype tables and lists of pairs in torch device tensors: the
eighteen numbers of every (row, pair) against the numpy model of tests/csr_geno_pair_util.py on the smallest shapes at which the kernel
can go wrong, bit for bit; cross-checks against vtx_csr_row_stats and vtx_csr_geno_tally on every case; every subset of NULL outputs;
then what the library must DECLINE — pairs of donors that do not exist, bad genotype bytes, bad arrays, counts out of range are refused
before a byte is written.  Every refused input is refused by the check kernels or on the host, which read within the given lengths only:
nothing here provokes a fault."""
import itertools

import numpy as np
import pytest
import torch

from tests.csr_geno_pair_util import CLASSES, NAMES, cases, model_pair_tally, random_pairs
from tests.csr_geno_util import model_geno_tally, random_counts, random_table
from tests.csr_group_util import model_group_sum
from tests.csr_ops_util import model_stats
from tests.test_gpu_csr_geno import tally as donor_tally
from tests.test_gpu_csr_group import fold
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
    return [(c, model_pair_tally(c[1], c[2], *c[4], c[5], c[6], c[7])) for c in cases()]


def tally(ctx, indptr, indices, n_minor, counts, geno, n_donors, pairs, names=NAMES, nnz=None, n_pairs=None, expect=None, no_geno=False,
          no_pairs=False):
    """-> dict of outputs as unsigned words, n_major x n_pairs x 6.  ``n_pairs``: the count the call is told (a call the host refuses:
    the outputs are made for the list's own length).  ``expect``: the status the call must fail with; the message comes back."""
    n_major = len(indptr) - 1
    nnz = len(indices) if nnz is None else nnz
    d = [dev(np.asarray(indptr, np.uint64))] + [dev(np.asarray(a, np.uint32)) for a in (indices, *counts)]
    d_geno = dev(np.asarray(geno, np.uint8).reshape(-1))
    d_pairs = dev(np.asarray(pairs, np.uint32).reshape(-1))
    n = n_major * len(pairs) * CLASSES
    out = {k: filled(n, k in WIDE) for k in NAMES}
    torch.cuda.synchronize()
    args = (n_major, n_minor, nnz, *[t.data_ptr() for t in d], 0 if no_geno else d_geno.data_ptr(), n_donors,
            0 if no_pairs else d_pairs.data_ptr(), len(pairs) if n_pairs is None else n_pairs, {k: out[k].data_ptr() for k in names})
    if expect is not None:
        with pytest.raises(lib.VtxError) as e:
            ctx.csr_geno_pair_tally(*args)
        assert e.value.status == expect, str(e.value)
        untouched(out.values())
        return str(e.value)
    ctx.csr_geno_pair_tally(*args)
    untouched([out[k] for k in NAMES if k not in names])
    return {k: words(out[k], n, k in WIDE).reshape(n_major, len(pairs), CLASSES) for k in names}


def same(got, want, names=NAMES):
    for k in names:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def test_every_case_against_the_model_row_stats_and_the_donor_tally(ctx, CASES):
    assert len(CASES) >= 20
    with_itself = both_orders = 0
    for (name, indptr, indices, n_minor, counts, geno, n_donors, pairs), want in CASES:
        got = tally(ctx, indptr, indices, n_minor, counts, geno, n_donors, pairs)
        same(got, want)
        if len(indptr) > 1:                                # over the classes, every pair sees every entry of the row once
            stats = row_stats(ctx, indptr, indices, n_minor, *counts, np.zeros(len(indices), np.uint32))
            for p in range(len(pairs)):
                assert np.array_equal(got["sum_alt"][:, p].sum(axis=1, dtype=np.uint64), stats["sum_alt"]), (name, p)
                assert np.array_equal(got["sum_ref"][:, p].sum(axis=1, dtype=np.uint64), stats["sum_ref"]), (name, p)
                assert np.array_equal(got["n_obs"][:, p].sum(axis=1, dtype=np.uint32), stats["n_alt"] + stats["n_ref"] - stats["n_both"]), (name, p)
        one = None
        for p, (a, b) in enumerate(pairs):
            if a == b:                                     # donor a's one-donor tally on 0, 2, 4, its missing class on 5, nothing on 1 and 3
                one = one or donor_tally(ctx, indptr, indices, n_minor, counts, geno, n_donors)
                for k in NAMES:
                    assert np.array_equal(got[k][:, p, [0, 2, 4, 5]], one[k][:, a, :]) and not got[k][:, p, [1, 3]].any(), (name, p, k)
                with_itself += 1
            for q in range(p):
                if (pairs[q][0], pairs[q][1]) == (b, a):   # (a, b) equals (b, a)
                    assert all(np.array_equal(got[k][:, p], got[k][:, q]) for k in NAMES), (name, p, q)
                    both_orders += a != b
        if name.startswith("sums_past_2_32"):
            assert got["sum_alt"].max() > 1 << 32 and got["sum_ref"].max() > 1 << 32
        if name == "one_donor_all_missing":
            assert not got["sum_alt"][:, :3, :5].any() and got["sum_alt"][:, :3, 5].any()
    assert with_itself >= 5 and both_orders >= 5


def test_more_rows_than_one_block_two_passes_and_the_same_bytes_twice(ctx):
    """300 rows: 75 blocks of four wavefronts; 70 pairs of 12 donors: a pass of 64 and one of 6."""
    rng = np.random.default_rng(47)
    indptr, indices = random_csr(rng, 300, 600, 9000)
    counts = random_counts(rng, 9000)
    geno = random_table(rng, 600, 12)
    pairs = random_pairs(rng, 70, 12)
    want = model_pair_tally(indptr, indices, *counts, geno, 12, pairs)
    a, b = (tally(ctx, indptr, indices, 600, counts, geno, 12, pairs) for _ in range(2))
    same(a, want)
    assert all(a[k].tobytes() == b[k].tobytes() for k in NAMES)


def by_name(CASES, name):
    return next(c for c in CASES if c[0][0] == name)


def test_every_subset_of_null_outputs_leaves_those_buffers_untouched(ctx, CASES):
    (name, indptr, indices, n_minor, counts, geno, n_donors, pairs), want = by_name(CASES, "pairs_5")
    for n in range(len(NAMES) + 1):
        for names in itertools.combinations(NAMES, n):
            got = tally(ctx, indptr, indices, n_minor, counts, geno, n_donors, pairs, names)      # (tally checks the buffers that were not passed)
            same(got, want, names)


def test_refusals_write_nothing_and_leave_the_context_usable(ctx, CASES):
    (name, indptr, indices, n_minor, counts, geno, n_donors, pairs), want = by_name(CASES, "same_donor_both_orders_and_repeats")
    assert n_donors == 5 and len(pairs) == 6 and len(indices) > 100
    top, top_donors = lib.load().vtx_csr_geno_pair_max(), lib.load().vtx_csr_geno_max()

    def after():
        same(tally(ctx, indptr, indices, n_minor, counts, geno, n_donors, pairs), want)
    INVAL, UNSUP = abi.VTX_E_INVAL, abi.VTX_E_UNSUPPORTED
    off = pairs.copy()
    off[4] = (5, 0)
    off[2] = (1, 0xFFFFFFFF)                               # two offenders, in either slot: the lower pair is named, with its donors
    two = geno.copy()
    two[30, 1], two[7, 3] = 3, 254
    order, index = indptr.copy(), indices.copy()
    order[3] = order[4] + np.uint64(1)
    index[100] = n_minor
    table = [(indptr, indices, geno, n_donors, off, None, INVAL, "pair 2 is (1, 4294967295)"),
             (indptr, indices, geno, 4, pairs, None, INVAL, "pair 5 is (4, 2)"),      # one donor fewer (the check reads no genotype): the last pair
             (indptr, indices, two, n_donors, pairs, None, INVAL, "variant 7, donor 3"),
             (indptr, indices, geno, n_donors, pairs, 0, INVAL, "no pairs"), (indptr, indices, geno, n_donors, pairs, top + 1, UNSUP, "at most"),
             (indptr, indices, geno, 0, pairs, None, INVAL, "no donors"), (indptr, indices, geno, top_donors + 1, pairs, None, UNSUP, "at most"),
             (order, indices, geno, n_donors, pairs, None, INVAL, "indptr decreases"), (indptr, index, geno, n_donors, pairs, None, INVAL, "an index >= n_minor")]
    for ptr, idx, gen, nd, prs, np_told, status, reason in table:
        msg = tally(ctx, ptr, idx, n_minor, counts, gen, nd, prs, n_pairs=np_told, expect=status)
        assert reason in msg, msg
        after()
    assert "32-bit" in tally(ctx, indptr, indices, n_minor, counts, geno, n_donors, pairs, nnz=1 << 32, expect=UNSUP)      # refused on the host, nothing is read
    after()
    assert "null" in tally(ctx, indptr, indices, n_minor, counts, geno, n_donors, pairs, expect=INVAL, no_geno=True)       # no table
    after()
    assert "null" in tally(ctx, indptr, indices, n_minor, counts, geno, n_donors, pairs, expect=INVAL, no_pairs=True)      # no list
    after()
    d = [dev(np.asarray(indptr, np.uint64))] + [dev(np.asarray(a, np.uint32)) for a in (indices, *counts)] + [dev(geno.reshape(-1))]
    d_pairs = dev(pairs.reshape(-1))
    torch.cuda.synchronize()
    rc = ctx._L.vtx_csr_geno_pair_tally(ctx._h, len(indptr) - 1, n_minor, len(indices), *[t.data_ptr() for t in d], n_donors, d_pairs.data_ptr(),
                                        len(pairs), None)      # no outputs
    assert rc == INVAL
    after()


def test_the_csr_is_judged_first_then_the_table_then_the_pairs(ctx, CASES):
    """One call with all three inputs bad names the CSR; with the CSR repaired, the genotype byte; with the table repaired, the pair.
    Nothing is written each time (tally checks the outputs).  The pseudobulk calls judge the CSR before the labels in the same way."""
    (name, indptr, indices, n_minor, counts, geno, n_donors, pairs), want = by_name(CASES, "same_donor_both_orders_and_repeats")
    INVAL = abi.VTX_E_INVAL
    order = indptr.copy()
    order[3] = order[4] + np.uint64(1)
    byte = geno.copy()
    byte[7, 3] = 254
    off = pairs.copy()
    off[4] = (5, 0)
    said = [tally(ctx, ptr, indices, n_minor, counts, gen, n_donors, off, expect=INVAL) for ptr, gen in ((order, byte), (indptr, byte), (indptr, geno))]
    for msg, reason in zip(said, ("indptr decreases", "variant 7, donor 3", "pair 4 is (5, 0)")):
        assert reason in msg and sum(r in msg for r in ("indptr", "variant", "pair 4")) == 1, msg
    same(tally(ctx, indptr, indices, n_minor, counts, geno, n_donors, pairs), want)
    three = (*counts, np.zeros(len(indices), np.uint32))
    label = np.zeros(n_minor, np.uint32)
    label[9] = 2                                           # two groups: neither a group nor VTX_GROUP_NONE
    msg = fold(ctx, order, indices, n_minor, three, label, 2, n_alloc=8, expect=INVAL, plan_expect=INVAL)      # plan and sum
    assert "indptr decreases" in msg and "label" not in msg, msg
    assert "the label of column 9" in fold(ctx, indptr, indices, n_minor, three, label, 2, n_alloc=8, expect=INVAL, plan_expect=INVAL)


def test_no_verdict_of_a_check_survives_its_call():
    """Refused and accepted calls of the three kinds of check (pairs, genotype bytes, labels) interleaved on one context: a call that
    follows a refusal is judged by its own input alone."""
    name, indptr, indices, n_minor, counts, geno, n_donors, pairs = next(c for c in cases() if c[0] == "same_donor_both_orders_and_repeats")
    INVAL = abi.VTX_E_INVAL
    off = pairs.copy()
    off[2] = (1, 0xFFFFFFFF)
    byte = geno.copy()
    byte[7, 3] = 254
    three = (*counts, np.zeros(len(indices), np.uint32))
    label = np.arange(n_minor, dtype=np.uint32) % 3
    bad_label = label.copy()
    bad_label[9] = 3
    with lib.Context(default_config(n_barcodes=4)) as c:
        assert "pair 2 is (1, 4294967295)" in tally(c, indptr, indices, n_minor, counts, geno, n_donors, off, expect=INVAL)
        same(donor_tally(c, indptr, indices, n_minor, counts, geno, n_donors), model_geno_tally(indptr, indices, *counts, geno, n_donors))
        assert "the label of column 9" in fold(c, indptr, indices, n_minor, three, bad_label, 3, n_alloc=8, expect=INVAL, plan_expect=INVAL)
        same(tally(c, indptr, indices, n_minor, counts, geno, n_donors, pairs), model_pair_tally(indptr, indices, *counts, geno, n_donors, pairs))
        assert "variant 7, donor 3" in donor_tally(c, indptr, indices, n_minor, counts, byte, n_donors, expect=INVAL)
        want = model_group_sum(indptr, indices, *three, label, 3)
        n_out, got = fold(c, indptr, indices, n_minor, three, label, 3)
        assert n_out == len(want["indices"])
        same(got, want, tuple(want))
        same(row_stats(c, indptr, indices, n_minor, *three), model_stats(indptr, *three), tuple(model_stats(indptr, *three)))


def test_phase_times_are_reported(ctx):
    rng = np.random.default_rng(53)
    indptr, indices = random_csr(rng, 300, 600, 40_000)
    tally(ctx, indptr, indices, 600, random_counts(rng, 40_000), random_table(rng, 600, 8), 8, random_pairs(rng, 20, 8))
    ms = ctx.csr_ms()
    print("phase times", ms)
    assert ms["check"] > 0 and ms["place"] > 0 and ms["sort"] == 0 and ms["offsets"] == 0 and sum(ms.values()) < 100
