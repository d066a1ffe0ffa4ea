"""vtx_csr_dense_sum on the GPU, driven directly with synthetic CSRs and tables in torch device tensors: every (row, column) sum against
the model in Python integers of tests/csr_dense_util.py on the smallest shapes at which the kernel can go wrong, bit for bit, with both
tables and with either one absent; a tie to vtx_csr_geno_tally on the same device (class-constant tables turn the dense sum into a
linear function of the tally, exact in integers); then what the library must DECLINE — bad arrays, counts out of range, no tables are
refused before a byte is written.  Every refused input is refused by the check kernel or on the host, which read within the given
lengths only: nothing here provokes a fault."""
import numpy as np
import pytest
import torch

from tests.csr_dense_util import INT32_MAX, INT32_MIN, model_dense_sum, modelled, random_weights, variants
from tests.csr_geno_util import NONE, cases as geno_cases, model_geno_tally, random_counts, random_table
from tests.test_gpu_csr_geno import tally as donor_tally
from tests.test_gpu_csr_ops import dev, filled, untouched, words
from tests.test_gpu_csr_transpose import random_csr
from vartrix_amd import abi, lib
from vartrix_amd.abi import default_config

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with lib.Context(default_config(n_barcodes=4)) as c:      # no batch, no run: the context gives the device, the stream, the work space
        yield c


@pytest.fixture(scope="module")
def CASES():
    """Every case with the model's answer to its three calls, computed once and shared."""
    return modelled()


def dense_sum(ctx, indptr, indices, n_minor, counts, w_alt, w_ref, n_cols, nnz=None, n_told=None, expect=None, no_out=False):
    """-> int64, n_major x n_cols.  ``w_alt`` / ``w_ref``: None is an absent table.  ``n_told``: the column count the call is told (a
    call the host refuses: the output is made for the tables' own).  ``expect``: the status the call must fail with; the message comes
    back."""
    n_major = len(indptr) - 1
    nnz = len(indices) if nnz is None else nnz
    d = [dev(np.asarray(indptr, np.uint64))] + [dev(np.asarray(a, np.uint32)) for a in (indices, *counts)]
    tables = [None if w is None else dev(np.asarray(w, np.int32).reshape(-1)) for w in (w_alt, w_ref)]
    n = n_major * n_cols
    out = filled(n, True)
    torch.cuda.synchronize()
    args = (n_major, n_minor, nnz, *[t.data_ptr() for t in d], *[0 if t is None else t.data_ptr() for t in tables], n_cols if n_told is None else n_told,
            0 if no_out else out.data_ptr())
    if expect is not None:
        with pytest.raises(lib.VtxError) as e:
            ctx.csr_dense_sum(*args)
        assert e.value.status == expect, str(e.value)
        untouched([out])
        return str(e.value)
    ctx.csr_dense_sum(*args)
    return words(out, n, True).view(np.int64).reshape(n_major, n_cols)


def test_every_case_and_its_null_table_variants_against_the_model(ctx, CASES):
    assert len(CASES) >= 20
    for case, want in CASES:
        name, indptr, indices, n_minor, counts, w_alt, w_ref, n_cols = case
        for tag, wa, wf in variants(case):
            if n_minor == 0 and tag != "both":
                continue                                   # no table has an element: one call
            got = dense_sum(ctx, indptr, indices, n_minor, counts, wa, wf, n_cols)
            assert np.array_equal(got, want[tag]), (name, tag)
        if name == "the_true_sum_leaves_int64":            # the wrap is the contract's: 3 (2^32 - 1) INT32_MIN modulo 2^64
            assert int(want["no_w_ref"][1, 0]) == -(1 << 63) + 3 * (1 << 31) and int(want["both"][1, 0]) == 3 * (1 << 32)
    assert abi.CSR_DENSE_MAX == 1024


def test_more_rows_than_one_block_two_passes_and_the_same_bytes_twice(ctx):
    """300 rows: 75 blocks of four wavefronts; 70 columns: a pass of 64 and one of 6."""
    rng = np.random.default_rng(47)
    indptr, indices = random_csr(rng, 300, 600, 9000)
    counts = random_counts(rng, 9000)
    w_alt, w_ref = random_weights(rng, 600, 70)
    want = model_dense_sum(indptr, indices, *counts, w_alt, w_ref, 70)
    a, b = (dense_sum(ctx, indptr, indices, 600, counts, w_alt, w_ref, 70) for _ in range(2))
    assert np.array_equal(a, want) and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["donors_5", "donors_65", "sums_past_2_32_two_passes"])
def test_class_constant_tables_tie_the_sum_to_the_donor_tally(ctx, name):
    """w_alt[v, d] = c_alt[class(geno[v, d])] (missing: 0) and w_ref likewise: the dense sum is then the sum over the classes of
    sum_alt[..., c] * c_alt[c] + sum_ref[..., c] * c_ref[c] of vtx_csr_geno_tally on the same device, exactly (modulo 2^64)."""
    _, indptr, indices, n_minor, counts, geno, n_donors = next(c for c in geno_cases() if c[0] == name)
    c_alt = np.array([-4829531, 726817, INT32_MAX, 0], np.int64)
    c_ref = np.array([-10076, -726817, INT32_MIN, 0], np.int64)
    cls = np.where(geno == NONE, 3, geno).astype(np.int64)
    w_alt, w_ref = c_alt[cls].astype(np.int32), c_ref[cls].astype(np.int32)
    got = dense_sum(ctx, indptr, indices, n_minor, counts, w_alt, w_ref, n_donors)
    t = donor_tally(ctx, indptr, indices, n_minor, counts, geno, n_donors)
    assert all(np.array_equal(t[k], v) for k, v in model_geno_tally(indptr, indices, *counts, geno, n_donors).items())
    with np.errstate(over="ignore"):
        want = ((t["sum_alt"] * c_alt.astype(np.uint64)).sum(axis=2, dtype=np.uint64) + (t["sum_ref"] * c_ref.astype(np.uint64)).sum(axis=2, dtype=np.uint64))
    assert np.array_equal(got.view(np.uint64), want) and got.any()


def by_name(CASES, name):
    return next(c for c in CASES if c[0][0] == name)


def test_refusals_write_nothing_and_leave_the_context_usable(ctx, CASES):
    (name, indptr, indices, n_minor, counts, w_alt, w_ref, n_cols), want = by_name(CASES, "cols_5")
    assert len(indices) > 100
    top = lib.load().vtx_csr_dense_max()

    def after():
        assert np.array_equal(dense_sum(ctx, indptr, indices, n_minor, counts, w_alt, w_ref, n_cols), want["both"])
    INVAL, UNSUP = abi.VTX_E_INVAL, abi.VTX_E_UNSUPPORTED
    order, index = indptr.copy(), indices.copy()
    order[3] = order[4] + np.uint64(1)
    index[100] = n_minor
    table = [(order, indices, w_alt, w_ref, None, INVAL, "indptr decreases"), (indptr, index, w_alt, w_ref, None, INVAL, "an index >= n_minor"),
             (indptr, indices, w_alt, w_ref, 0, INVAL, "no columns"), (indptr, indices, w_alt, w_ref, top + 1, UNSUP, "at most"),
             (indptr, indices, None, None, None, INVAL, "null tables")]
    for ptr, idx, wa, wf, told, status, reason in table:
        msg = dense_sum(ctx, ptr, idx, n_minor, counts, wa, wf, n_cols, n_told=told, expect=status)
        assert reason in msg, msg
        after()
    assert "32-bit" in dense_sum(ctx, indptr, indices, n_minor, counts, w_alt, w_ref, n_cols, nnz=1 << 32, expect=UNSUP)      # refused on the host, nothing is read
    after()
    assert "null" in dense_sum(ctx, indptr, indices, n_minor, counts, w_alt, w_ref, n_cols, expect=INVAL, no_out=True)          # no output
    after()
    d = [dev(np.asarray(indptr, np.uint64))] + [dev(np.asarray(a, np.uint32)) for a in (indices, *counts)] + [dev(w_alt.reshape(-1)), dev(w_ref.reshape(-1))]
    out = filled(len(indptr) - 1, True)
    torch.cuda.synchronize()
    rc = ctx._L.vtx_csr_dense_sum(None, len(indptr) - 1, n_minor, len(indices), *[t.data_ptr() for t in d], n_cols, out.data_ptr())      # no context
    assert rc == INVAL
    untouched([out])
    after()


def test_a_bad_csr_is_judged_before_anything_else(ctx, CASES):
    """One call with a bad CSR and tables of every int32 names the CSR and writes nothing; the same tables with the CSR repaired are
    summed: no weight is ever refused."""
    (name, indptr, indices, n_minor, counts, w_alt, w_ref, n_cols), want = by_name(CASES, "cols_5")
    order = indptr.copy()
    order[3] = order[4] + np.uint64(1)
    msg = dense_sum(ctx, order, indices, n_minor, counts, w_alt, w_ref, n_cols, expect=abi.VTX_E_INVAL)
    assert "indptr decreases" in msg
    assert {INT32_MIN, INT32_MAX} <= set(w_alt.reshape(-1).tolist())
    assert np.array_equal(dense_sum(ctx, indptr, indices, n_minor, counts, w_alt, w_ref, n_cols), want["both"])


def test_no_verdict_of_a_check_survives_its_call(CASES):
    """Refused and accepted calls interleaved with the donor tally's on one context: a call that follows a refusal is judged by its own
    input alone."""
    (name, indptr, indices, n_minor, counts, w_alt, w_ref, n_cols), want = by_name(CASES, "cols_5")
    rng = np.random.default_rng(5)
    geno = random_table(rng, n_minor, 4)
    byte = geno.copy()
    byte[7, 3] = 254
    index = indices.copy()
    index[100] = n_minor
    INVAL = abi.VTX_E_INVAL
    with lib.Context(default_config(n_barcodes=4)) as c:
        assert "an index >= n_minor" in dense_sum(c, indptr, index, n_minor, counts, w_alt, w_ref, n_cols, expect=INVAL)
        assert np.array_equal(dense_sum(c, indptr, indices, n_minor, counts, w_alt, None, n_cols), want["no_w_ref"])
        assert "variant 7, donor 3" in donor_tally(c, indptr, indices, n_minor, counts, byte, 4, expect=INVAL)
        assert np.array_equal(dense_sum(c, indptr, indices, n_minor, counts, None, w_ref, n_cols), want["no_w_alt"])
        assert "an index >= n_minor" in dense_sum(c, indptr, index, n_minor, counts, w_alt, w_ref, n_cols, expect=INVAL)
        got = donor_tally(c, indptr, indices, n_minor, counts, geno, 4)
        assert all(np.array_equal(got[k], v) for k, v in model_geno_tally(indptr, indices, *counts, geno, 4).items())
        assert np.array_equal(dense_sum(c, indptr, indices, n_minor, counts, w_alt, w_ref, n_cols), want["both"])


def test_phase_times_are_reported(ctx):
    rng = np.random.default_rng(53)
    indptr, indices = random_csr(rng, 300, 600, 40_000)
    w_alt, w_ref = random_weights(rng, 600, 8)
    dense_sum(ctx, indptr, indices, 600, random_counts(rng, 40_000), w_alt, w_ref, 8)
    ms = ctx.csr_ms()
    print("phase times", ms)
    assert ms["check"] > 0 and ms["place"] > 0 and ms["sort"] == 0 and ms["offsets"] == 0 and sum(ms.values()) < 100
