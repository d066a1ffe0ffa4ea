"""vtx_csr_row_stats, vtx_csr_select_plan and vtx_csr_select on the GPU, driven directly with synthetic CSRs in torch device tensors:
the seven statistics and the selected matrix against the numpy models of tests/csr_ops_util.py (and scipy's own ``A[rows][:, cols]`` on
canonical inputs), the payload arrays bit for bit; then what the library must DECLINE — a caller's bad arrays, and allocations made for
another selection, are refused with VTX_E_INVAL before a byte is written.  Every refused input is refused by the check kernel or on the
host, which read within the given lengths only: nothing here provokes a fault."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests.csr_ops_util import COUNTS, SUMS, csr_with_row_lengths, model_select, model_stats, random_counts
from tests.test_gpu_csr_transpose import make_payloads, random_csr
from vartrix_amd import abi, lib
from vartrix_amd.abi import default_config

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PATTERN = 0x5A5A5A5A
GUARD = 4                      # sentinel elements behind every output array: a store past the end would show there


@pytest.fixture(scope="module")
def ctx():
    with lib.Context(default_config(n_barcodes=4)) as c:      # no batch, no run: the context gives the device, the stream, the work space
        yield c


def dev(a):
    """A numpy array of 1-, 4- or 8-byte elements as a device tensor of the same bytes (one spare element when empty: a real address)."""
    a = np.ascontiguousarray(a)
    view = {1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    if not a.size:
        return torch.zeros(1, dtype={1: torch.uint8, 4: torch.int32, 8: torch.int64}[a.dtype.itemsize], device=DEV)
    return torch.from_numpy(a.view(view).copy()).to(DEV)


def mask(m):
    """A byte per row / column: a boolean mask as 0 / 1, a byte mask as it is."""
    return None if m is None else dev(np.asarray(m).astype(np.uint8))


def filled(n, wide):
    """n + GUARD elements of 4 (8 if ``wide``) bytes whose every 32-bit word is PATTERN."""
    return torch.full(((n + GUARD) * (2 if wide else 1),), PATTERN, dtype=torch.int32, device=DEV)


def words(t, n, wide):
    """The first n elements as unsigned words; everything behind them must still hold the pattern."""
    a = t.cpu().numpy()
    k = n * (2 if wide else 1)
    assert np.all(a[k:] == PATTERN), "a store behind the end of an output array"
    return a[:k].view(np.uint64) if wide else a[:k].view(np.uint32)


def untouched(tensors):
    for t in tensors:
        assert bool((t == PATTERN).all()), "an output buffer was written before the input was refused"


def row_stats(ctx, indptr, indices, n_minor, alt, ref, unk, names=COUNTS + SUMS, nnz=None, expect=None):
    n_major = len(indptr) - 1
    nnz = len(indices) if nnz is None else nnz
    d = [dev(np.asarray(indptr, np.uint64))] + [dev(np.asarray(a, np.uint32)) for a in (indices, alt, ref, unk)]
    out = {k: filled(n_major, k in SUMS) for k in names}
    torch.cuda.synchronize()
    args = (n_major, n_minor, nnz, *[t.data_ptr() for t in d], {k: v.data_ptr() for k, v in out.items()})
    if expect is not None:
        with pytest.raises(lib.VtxError) as e:
            ctx.csr_row_stats(*args)
        assert e.value.status == expect, str(e.value)
        untouched(out.values())
        return str(e.value)
    ctx.csr_row_stats(*args)
    return {k: words(v, n_major, k in SUMS) for k, v in out.items()}


def select(ctx, indptr, indices, n_minor, km, kn, payloads=(), ids=True, nnz=None, sizes=None, expect=None, plan_expect=None):
    """plan + select -> (sizes, dict of outputs as unsigned words).  ``sizes``: passed to the select INSTEAD of the plan's (the outputs
    keep the plan's sizes).  ``expect`` / ``plan_expect``: the status the select / the plan must fail with."""
    n_major = len(indptr) - 1
    nnz = len(indices) if nnz is None else nnz
    d_ptr, d_idx = dev(np.asarray(indptr, np.uint64)), dev(np.asarray(indices, np.uint32))
    d_km, d_kn = mask(km), mask(kn)
    d_in = [dev(p) for p in payloads]
    torch.cuda.synchronize()
    head = (n_major, n_minor, nnz, d_ptr.data_ptr(), d_idx.data_ptr(), d_km.data_ptr() if d_km is not None else 0, d_kn.data_ptr() if d_kn is not None else 0)
    if plan_expect is not None:
        with pytest.raises(lib.VtxError) as e:
            ctx.csr_select_plan(*head)
        assert e.value.status == plan_expect, str(e.value)
        planned, (a, b, n) = None, (n_major, n_minor, len(indices))      # the select below is refused as well: any sizes do
    else:
        a, b, n = planned = ctx.csr_select_plan(*head)
    out = {"indptr": filled(a + 1, True), "indices": filled(n, False), "major_ids": filled(a, False), "minor_ids": filled(b, False)}
    o_pay = [filled(n, p.dtype.itemsize == 8) for p in payloads]
    torch.cuda.synchronize()
    args = (*head, sizes or (a, b, n), out["indptr"].data_ptr(), out["indices"].data_ptr(), out["major_ids"].data_ptr() if ids else 0,
            out["minor_ids"].data_ptr() if ids else 0, [(i.data_ptr(), o.data_ptr(), p.dtype.itemsize) for i, o, p in zip(d_in, o_pay, payloads)])
    if expect is not None:
        with pytest.raises(lib.VtxError) as e:
            ctx.csr_select(*args)
        assert e.value.status == expect, str(e.value)
        untouched(list(out.values()) + o_pay)
        return str(e.value)
    ctx.csr_select(*args)
    if not ids:
        untouched([out["major_ids"], out["minor_ids"]])
    got = {"indptr": words(out["indptr"], a + 1, True), "indices": words(out["indices"], n, False),
           "major_ids": words(out["major_ids"], a if ids else 0, False), "minor_ids": words(out["minor_ids"], b if ids else 0, False),
           "payloads": [words(o, n, p.dtype.itemsize == 8) for o, p in zip(o_pay, payloads)]}
    return planned, got


def unsigned(p):
    return p.view(np.uint64 if p.dtype.itemsize == 8 else np.uint32)


def check_case(ctx, indptr, indices, n_minor, km=None, kn=None, seed=0, canonical=True, big=False):
    """Statistics and selection of one matrix against the models; on canonical inputs also against scipy's indexing."""
    rng = np.random.default_rng(seed)
    n_major, nnz = len(indptr) - 1, len(indices)
    alt, ref, unk = random_counts(rng, nnz, big)
    got, want = row_stats(ctx, indptr, indices, n_minor, alt, ref, unk), model_stats(indptr, alt, ref, unk)
    for k in COUNTS + SUMS:
        assert np.array_equal(got[k], want[k]), k
    pay = make_payloads(rng, nnz)                              # u32 words; f64 with NaN payloads, -0.0, explicit zeros; f64 positions + 1
    sizes, sel = select(ctx, indptr, indices, n_minor, km, kn, pay)
    model = model_select(indptr, indices, n_minor, km, kn, [unsigned(p) for p in pay])
    assert sizes == (len(model["major_ids"]), len(model["minor_ids"]), len(model["indices"]))
    for k in ("indptr", "indices", "major_ids", "minor_ids"):
        assert np.array_equal(sel[k], model[k]), k
    for g, w in zip(sel["payloads"], model["payloads"]):        # bit patterns, not values: NaN == NaN here, -0.0 != 0.0
        assert np.array_equal(g, w)
    if canonical:
        a = sp.csr_matrix((pay[2], indices.astype(np.int64), indptr.astype(np.int64)), shape=(n_major, n_minor))
        rm = np.ones(n_major, bool) if km is None else np.asarray(km) != 0
        cm = np.ones(n_minor, bool) if kn is None else np.asarray(kn) != 0
        b = a[rm][:, cm]
        assert b.shape == sizes[:2] and b.nnz == sizes[2]
        assert np.array_equal(sel["indptr"], b.indptr.astype(np.uint64)) and np.array_equal(sel["indices"], b.indices.astype(np.uint32))
        assert np.array_equal(sel["payloads"][2], b.data.view(np.uint64))
    return sizes, sel, got


def masks(rng, n_major, n_minor, p=0.6):
    return rng.random(n_major) < p, rng.random(n_minor) < p


def test_empty_matrix_one_row_one_column(ctx):
    none = np.zeros(0, np.uint32)
    assert check_case(ctx, np.zeros(1, np.uint64), none, 5, None, np.array([1, 0, 1, 1, 0], bool))[0] == (0, 3, 0)     # no rows
    assert check_case(ctx, np.zeros(8, np.uint64), none, 3, np.array([1, 0, 1, 0, 0, 1, 1], bool), None)[0] == (4, 3, 0)   # rows, no entries
    rng = np.random.default_rng(1)
    indptr, indices = csr_with_row_lengths(rng, [40], 100)                                           # one row
    check_case(ctx, indptr, indices, 100, None, rng.random(100) < 0.5)
    assert check_case(ctx, indptr, indices, 100, np.array([0], bool), None)[0] == (0, 100, 0)
    indptr = np.concatenate([[0], np.cumsum(rng.random(300) < 0.5)]).astype(np.uint64)              # one column
    indices = np.zeros(int(indptr[-1]), np.uint32)
    check_case(ctx, indptr, indices, 1, rng.random(300) < 0.5, None, seed=2)
    assert check_case(ctx, indptr, indices, 1, None, np.array([0], bool))[0] == (300, 0, 0)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_block_edges(ctx, n):
    """n rows and n entries: the last lane of a block, the first lane of the next one."""
    rng = np.random.default_rng(n)
    indptr, indices = random_csr(rng, n, 40, n)
    km, kn = masks(rng, n, 40)
    check_case(ctx, indptr, indices, 40, km, kn, seed=n)
    check_case(ctx, indptr, indices, 40, None, None, seed=n + 1)


def test_row_lengths_around_the_wavefront(ctx):
    rng = np.random.default_rng(4)
    lens = [0, 1, 63, 64, 65, 129, 0, 0, 64, 1]
    indptr, indices = csr_with_row_lengths(rng, lens, 130)
    km, kn = masks(rng, len(lens), 130)
    _, _, st = check_case(ctx, indptr, indices, 130, km, kn, seed=5)
    assert st["n_entries"].tolist() == lens
    check_case(ctx, indptr, indices, 130, None, kn, seed=6, big=True)      # sums past 2^32


STEPS = [(8 * G * 97 + extra, 97) for G in (1, 2, 4, 8, 16, 32) for extra in (0, 1)] + [(48, 97), (97, 97), (3 * 97, 97), (300 * 97, 97)]


@pytest.mark.parametrize("nnz,n_major", STEPS)
def test_both_sides_of_every_step_of_the_group_size_rule(ctx, nnz, n_major):
    """nnz = 8 G n_major runs G lanes per row, one entry more 2 G (vtxr::group_lanes): mean row lengths from 0.5 to 300, every
    instance of the kernel, each over more than one block's worth of entries and with rows of unlike lengths in a wavefront."""
    rng = np.random.default_rng(nnz)
    lens = rng.multinomial(nnz, np.ones(n_major) / n_major)
    n_minor = int(lens.max()) + 3
    indptr, indices = csr_with_row_lengths(rng, lens, n_minor)
    km, kn = masks(rng, n_major, n_minor)
    check_case(ctx, indptr, indices, n_minor, km, kn, seed=nnz + 1, big=nnz % 2 == 0)


def test_a_million_entries(ctx):
    rng = np.random.default_rng(8)
    indptr, indices = random_csr(rng, 1500, 1000, 1_000_003)
    km, kn = masks(rng, 1500, 1000, 0.5)
    sizes, _, _ = check_case(ctx, indptr, indices, 1000, km, kn, seed=9)
    assert 200_000 < sizes[2] < 300_000


def test_unsorted_and_duplicate_indices(ctx):
    """Entries keep their source order inside a row, sorted or not; duplicates stay duplicates, and a row longer than n_minor is
    walked and counted like any other."""
    rng = np.random.default_rng(10)
    lens = [4, 0, 900, 7, 1, 70]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    indices = rng.integers(0, 40, int(indptr[-1]), dtype=np.uint64).astype(np.uint32)
    km, kn = np.array([1, 1, 1, 0, 1, 1], bool), rng.random(40) < 0.5
    _, _, st = check_case(ctx, indptr, indices, 40, km, kn, canonical=False)
    assert st["n_entries"][2] == 900


def test_same_input_twice_gives_identical_bytes(ctx):
    rng = np.random.default_rng(12)
    indptr, indices = random_csr(rng, 700, 300, 50_000)
    km, kn = masks(rng, 700, 300)
    a, b = (check_case(ctx, indptr, indices, 300, km, kn, seed=13) for _ in range(2))
    assert a[0] == b[0]
    for k in ("indptr", "indices", "major_ids", "minor_ids"):
        assert a[1][k].tobytes() == b[1][k].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1]["payloads"], b[1]["payloads"]))
    assert all(a[2][k].tobytes() == b[2][k].tobytes() for k in COUNTS + SUMS)


def test_null_arguments(ctx):
    """NULL masks keep everything, NULL id arrays and NULL statistics arrays are not written, no payloads at all is fine."""
    rng = np.random.default_rng(14)
    indptr, indices = random_csr(rng, 90, 50, 1200)
    alt, ref, unk = random_counts(rng, 1200)
    want = model_stats(indptr, alt, ref, unk)
    for names in (("n_alt", "n_ref"), ("sum_unk",), ("n_entries", "sum_alt"), ()):
        got = row_stats(ctx, indptr, indices, 50, alt, ref, unk, names)
        assert set(got) == set(names) and all(np.array_equal(got[k], want[k]) for k in names)
    km, kn = masks(rng, 90, 50)
    for m, n in ((None, None), (km, None), (None, kn)):
        sizes, sel = select(ctx, indptr, indices, 50, m, n, (), ids=False)
        model = model_select(indptr, indices, 50, m, n)
        assert np.array_equal(sel["indptr"], model["indptr"]) and np.array_equal(sel["indices"], model["indices"])
    sizes, sel = select(ctx, indptr, indices, 50, None, None, [alt])
    assert sizes == (90, 50, 1200) and np.array_equal(sel["indptr"], indptr) and np.array_equal(sel["indices"], indices)
    assert np.array_equal(sel["payloads"][0], alt) and np.array_equal(sel["major_ids"], np.arange(90)) and np.array_equal(sel["minor_ids"], np.arange(50))
    # a torch.bool tensor is a mask as it is
    t = torch.from_numpy(km).to(DEV)
    assert t.dtype == torch.bool
    torch.cuda.synchronize()
    d_ptr, d_idx = dev(indptr), dev(indices)
    torch.cuda.synchronize()
    assert ctx.csr_select_plan(90, 50, 1200, d_ptr.data_ptr(), d_idx.data_ptr(), t.data_ptr(), 0)[0] == int(km.sum())


def test_bad_arrays_are_refused_with_nothing_written(ctx):
    """Each of the four reasons, by each of the three calls: VTX_E_INVAL, the reason in the message, every output buffer still the
    pattern — and the next valid call on the same context succeeds."""
    rng = np.random.default_rng(15)
    indptr, indices = random_csr(rng, 30, 40, 500)
    alt, ref, unk = random_counts(rng, 500)
    km, kn = masks(rng, 30, 40)
    first, order, index = indptr.copy(), indptr.copy(), indices.copy()
    first[0] = 1
    order[10] = order[11] + np.uint64(1)
    index[123] = 40
    bad = [(first, indices, None, "indptr[0] != 0"), (order, indices, None, "indptr decreases"),
           (indptr, indices, 499, "indptr[n_major] != nnz"),        # fewer entries than the offsets say: nothing past the arrays is read
           (indptr, index, None, "an index >= n_minor")]
    for ptr, idx, nnz, reason in bad:
        assert reason in row_stats(ctx, ptr, idx, 40, alt, ref, unk, nnz=nnz, expect=abi.VTX_E_INVAL)
        assert reason in select(ctx, ptr, idx, 40, km, kn, [alt], nnz=nnz, plan_expect=abi.VTX_E_INVAL, expect=abi.VTX_E_INVAL)
        check_case(ctx, indptr, indices, 40, km, kn, seed=16)   # the context is as usable as before


def test_sizes_of_another_selection_are_refused_with_nothing_written(ctx):
    rng = np.random.default_rng(17)
    indptr, indices = random_csr(rng, 60, 70, 900)
    km, kn = masks(rng, 60, 70)
    pay = make_payloads(rng, 900)
    (a, b, n), _ = select(ctx, indptr, indices, 70, km, kn, pay)
    for wrong in ((a + 1, b, n), (a - 1, b, n), (a, b + 1, n), (a, b, n + 1), (a, b, n - 1), (60, 70, 900)):
        msg = select(ctx, indptr, indices, 70, km, kn, pay, sizes=wrong, expect=abi.VTX_E_INVAL)
        assert "vtx_csr_select_plan" in msg
    # ... and the sizes of the full matrix are the wrong ones for these masks, the right ones without masks
    assert select(ctx, indptr, indices, 70, None, None, pay, sizes=(60, 70, 900))[0] == (60, 70, 900)
    check_case(ctx, indptr, indices, 70, km, kn, seed=18)


def test_bad_payload_sizes_and_null_arrays(ctx):
    rng = np.random.default_rng(19)
    indptr, indices = random_csr(rng, 10, 10, 30)
    d_ptr, d_idx, o_ptr, o_idx = dev(indptr), dev(indices), filled(11, True), filled(30, False)
    torch.cuda.synchronize()
    head = (10, 10, 30, d_ptr.data_ptr(), d_idx.data_ptr(), 0, 0, (10, 10, 30))
    for args in ((o_ptr.data_ptr(), o_idx.data_ptr(), 0, 0, [(d_idx.data_ptr(), o_idx.data_ptr(), 2)]),       # 2-byte elements
                 (0, o_idx.data_ptr(), 0, 0, []), (o_ptr.data_ptr(), 0, 0, 0, []),                               # no output offsets / indices
                 (o_ptr.data_ptr(), o_idx.data_ptr(), 0, 0, [(0, o_idx.data_ptr(), 4)])):                         # a null payload
        with pytest.raises(lib.VtxError) as e:
            ctx.csr_select(*head, *args)
        assert e.value.status == abi.VTX_E_INVAL
    untouched([o_ptr, o_idx])
    with pytest.raises(lib.VtxError) as e:
        ctx.csr_row_stats(10, 10, 30, d_ptr.data_ptr(), d_idx.data_ptr(), 0, d_idx.data_ptr(), d_idx.data_ptr(), {})
    assert e.value.status == abi.VTX_E_INVAL
    with pytest.raises(lib.VtxError) as e:                       # positions are 32-bit; refused on the host, nothing is read
        ctx.csr_select_plan(10, 10, 1 << 32, d_ptr.data_ptr(), d_idx.data_ptr(), 0, 0)
    assert e.value.status == abi.VTX_E_UNSUPPORTED


def test_phase_times_are_reported(ctx):
    rng = np.random.default_rng(20)
    indptr, indices = random_csr(rng, 400, 300, 60_000)
    alt, ref, unk = random_counts(rng, 60_000)
    row_stats(ctx, indptr, indices, 300, alt, ref, unk)
    ms = ctx.csr_ms()
    assert ms["check"] > 0 and ms["place"] > 0 and ms["sort"] == 0 and ms["offsets"] == 0
    select(ctx, indptr, indices, 300, *masks(rng, 400, 300), [alt])
    ms = ctx.csr_ms()
    assert all(ms[k] > 0 for k in ("check", "sort", "offsets", "place")) and sum(ms.values()) < 100
