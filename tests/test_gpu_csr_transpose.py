"""vtx_csr_transpose on the GPU, driven directly with synthetic CSRs in torch device tensors: the offsets and indices against
``scipy ... .T.tocsr()``, the permutation against ``np.argsort(indices, kind="stable")``, the payload arrays bit for bit; then what the
library must DECLINE — a caller's bad arrays are refused with VTX_E_INVAL before a byte is written through them."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from vartrix_amd import abi, lib
from vartrix_amd.abi import default_config

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PATTERN = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ctx():
    with lib.Context(default_config(n_barcodes=4)) as c:      # no batch, no run: the context gives the device, the stream, the work space
        yield c


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(DEV)


def dev_i64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to(DEV)


def filled(n, dtype):
    """n elements of ``dtype`` whose every 32-bit word is PATTERN."""
    words = n * (2 if dtype == torch.int64 else 1)
    return torch.full((max(words, 1),), PATTERN, dtype=torch.int32, device=DEV)


def words(t, n, dtype):
    a = t.cpu().numpy()
    return a[: n * 2].view(np.uint64) if dtype == torch.int64 else a[:n].view(np.uint32)


def transpose(ctx, n_major, n_minor, indptr, indices, payloads=(), with_perm=True, nnz=None, expect=None):
    """-> (indptr_t, indices_t, perm or None, [payload out as unsigned words]); ``expect``: the status the call must fail with — then
    every output buffer must still hold the pattern."""
    nnz = len(indices) if nnz is None else nnz
    n_idx = len(indices)
    d_ptr, d_idx = dev_i64(np.asarray(indptr, np.uint64)), dev_i32(np.asarray(indices, np.uint32)) if n_idx else filled(0, torch.int32)
    d_in = [dev_i64(p) if p.dtype.itemsize == 8 else dev_i32(p) for p in payloads] if n_idx else [filled(0, torch.int32) for _ in payloads]
    o_ptr, o_idx, o_perm = filled(n_minor + 1, torch.int64), filled(n_idx, torch.int32), filled(n_idx, torch.int32)
    o_pay = [filled(n_idx, torch.int64 if p.dtype.itemsize == 8 else torch.int32) for p in payloads]
    torch.cuda.synchronize()
    args = (n_major, n_minor, nnz, d_ptr.data_ptr(), d_idx.data_ptr(), o_ptr.data_ptr(), o_idx.data_ptr(), o_perm.data_ptr() if with_perm else 0,
            [(i.data_ptr(), o.data_ptr(), p.dtype.itemsize) for i, o, p in zip(d_in, o_pay, payloads)])
    if expect is not None:
        with pytest.raises(lib.VtxError) as e:
            ctx.csr_transpose(*args)
        assert e.value.status == expect, str(e.value)
        for t in [o_ptr, o_idx, o_perm] + o_pay:
            assert bool((t == PATTERN).all()), "an output buffer was written before the input was refused"
        return str(e.value)
    ctx.csr_transpose(*args)
    if not with_perm:
        assert bool((o_perm == PATTERN).all())
    return (words(o_ptr, n_minor + 1, torch.int64), words(o_idx, n_idx, torch.int32), words(o_perm, n_idx, torch.int32) if with_perm else None,
            [words(o, n_idx, torch.int64 if p.dtype.itemsize == 8 else torch.int32) for o, p in zip(o_pay, payloads)])


def random_csr(rng, n_major, n_minor, nnz):
    """nnz distinct cells of an n_major x n_minor matrix, in CSR order (indices ascending inside a row)."""
    flat = np.sort(rng.permutation(n_major * n_minor)[:nnz])
    row, col = flat // n_minor, flat % n_minor
    indptr = np.searchsorted(row, np.arange(n_major + 1), side="left").astype(np.uint64)
    return indptr, col.astype(np.uint32)


def make_payloads(rng, n):
    """One uint32 array and two float64 arrays: the first with NaNs of distinct payload bits (quiet and signalling, both signs), -0.0
    and explicit 0.0 among ordinary values; the second the source position + 1 (what scipy's transpose carries as data)."""
    u = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    f = rng.random(n)
    bits = f.view(np.uint64)
    k = np.arange(n, dtype=np.uint64)
    bits[k % 7 == 1] = 0x7FF8000000000000 | (k[k % 7 == 1] + 1)
    bits[k % 7 == 2] = 0xFFF0000000000001 + k[k % 7 == 2]
    bits[k % 7 == 3] = 0x8000000000000000          # -0.0
    bits[k % 7 == 4] = 0                           # an explicit 0.0: nothing is dropped for being zero
    return [u, f, np.arange(1, n + 1, dtype=np.float64)]


def check_case(ctx, n_major, n_minor, indptr, indices, seed=0, sorted_rows=True):
    rng = np.random.default_rng(seed)
    n = len(indices)
    pay = make_payloads(rng, n)
    got_ptr, got_idx, got_perm, got_pay = transpose(ctx, n_major, n_minor, indptr, indices, pay)
    perm = np.argsort(indices, kind="stable").astype(np.uint32)
    assert np.array_equal(got_perm, perm)
    row_of = np.repeat(np.arange(n_major, dtype=np.uint32), np.diff(indptr.astype(np.int64)))
    assert np.array_equal(got_idx, row_of[perm])
    assert np.array_equal(got_ptr, np.searchsorted(indices[perm], np.arange(n_minor + 1), side="left").astype(np.uint64))
    if sorted_rows:      # scipy's own transpose: structure, and the source positions it carries as data
        t = sp.csr_matrix((pay[2], indices.astype(np.int64), indptr.astype(np.int64)), shape=(n_major, n_minor)).T.tocsr()
        assert t.nnz == n                                      # scipy kept every entry
        assert np.array_equal(got_ptr, t.indptr.astype(np.uint64)) and np.array_equal(got_idx, t.indices.astype(np.uint32))
        assert np.array_equal(got_pay[2], t.data.view(np.uint64))
    for g, p in zip(got_pay, pay):                              # bit patterns, not values: NaN == NaN here, -0.0 != 0.0
        assert np.array_equal(g, p.view(np.uint64 if p.dtype.itemsize == 8 else np.uint32)[perm])
    return got_ptr, got_idx, got_perm, got_pay


def test_empty_and_minimal(ctx):
    ptr, idx, perm, _ = check_case(ctx, 3, 5, np.zeros(4, np.uint64), np.zeros(0, np.uint32))
    assert np.array_equal(ptr, np.zeros(6, np.uint64)) and idx.size == 0
    ptr, idx, perm, _ = check_case(ctx, 1, 1, np.array([0, 1], np.uint64), np.zeros(1, np.uint32))
    assert ptr.tolist() == [0, 1] and idx.tolist() == [0] and perm.tolist() == [0]


def test_one_row_and_one_column(ctx):
    check_case(ctx, 1, 300, np.array([0, 300], np.uint64), np.arange(300, dtype=np.uint32))
    ptr, idx, _, _ = check_case(ctx, 300, 1, np.arange(301, dtype=np.uint64), np.zeros(300, np.uint32))      # every entry in one output row
    assert ptr.tolist() == [0, 300] and np.array_equal(idx, np.arange(300))


def test_sparse_random_with_empty_border(ctx):
    rng = np.random.default_rng(1)
    mask = rng.random((70, 50)) < 0.3
    mask[0] = mask[-1] = False
    mask[:, 0] = mask[:, -1] = False
    row, col = np.nonzero(mask)
    indptr = np.searchsorted(row, np.arange(71), side="left").astype(np.uint64)
    ptr, _, _, _ = check_case(ctx, 70, 50, indptr, col.astype(np.uint32), seed=1)
    assert ptr[0] == ptr[1] == 0 and ptr[49] == ptr[50] == len(col)


def test_wide_and_mostly_empty(ctx):
    indptr, indices = random_csr(np.random.default_rng(2), 50, 100003, 1000)
    check_case(ctx, 50, 100003, indptr, indices, seed=2)


@pytest.mark.parametrize("n_minor,cols", [(257, [256]), (258, [0, 257]), (1000003, [5, 6, 700000]), (4000, [])])
def test_long_stretches_of_empty_output_rows(ctx, n_minor, cols):
    """Stretches of more than 256 empty output rows are written by one lane per row (csr_fill_kernel), at the threshold and far
    beyond it; the device reports its time by phase."""
    indices = np.array(cols, np.uint32)
    indptr = np.array([0, len(cols)], np.uint64)
    check_case(ctx, 1, n_minor, indptr, indices, seed=n_minor)
    ms = ctx.csr_ms()
    assert set(ms) == {"check", "sort", "offsets", "place"} and all(0.0 <= v < 1000.0 for v in ms.values()) and ms["offsets"] > 0.0


@pytest.mark.parametrize("nnz", [255, 256, 257])
def test_block_boundaries(ctx, nnz):
    indptr, indices = random_csr(np.random.default_rng(nnz), 20, 30, nnz)
    check_case(ctx, 20, 30, indptr, indices, seed=nnz)


@pytest.mark.parametrize("nnz,shape", [(65535, (300, 400)), (65536, (300, 400)), (65537, (300, 400)), (1000003, (1500, 1000))])
def test_tile_boundaries(ctx, nnz, shape):
    indptr, indices = random_csr(np.random.default_rng(nnz), shape[0], shape[1], nnz)
    check_case(ctx, shape[0], shape[1], indptr, indices, seed=nnz)


@pytest.mark.parametrize("n_minor", [2, 64, 65])
def test_column_counts(ctx, n_minor):
    indptr, indices = random_csr(np.random.default_rng(n_minor), 40, n_minor, 20 * n_minor)
    check_case(ctx, 40, n_minor, indptr, indices, seed=n_minor)


def test_unsorted_and_duplicate_indices_keep_source_order(ctx):
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 40, 60)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    indices = rng.integers(0, 11, int(lens.sum())).astype(np.uint32)      # 11 columns: many duplicates inside a row, no order
    check_case(ctx, 60, 11, indptr, indices, seed=9, sorted_rows=False)


def test_same_input_twice_gives_identical_bytes_and_perm_is_optional(ctx):
    indptr, indices = random_csr(np.random.default_rng(4), 200, 300, 30000)
    pay = make_payloads(np.random.default_rng(4), len(indices))
    a = transpose(ctx, 200, 300, indptr, indices, pay)
    b = transpose(ctx, 200, 300, indptr, indices, pay)
    c = transpose(ctx, 200, 300, indptr, indices, pay, with_perm=False)
    assert c[2] is None
    for x, y, z in zip(a[:2] + tuple(a[3]), b[:2] + tuple(b[3]), c[:2] + tuple(c[3])):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert a[2].tobytes() == b[2].tobytes()


def test_bad_arrays_are_declined_before_anything_is_written(ctx):
    """Arguments the library must decline: VTX_E_INVAL with the reason, every output buffer untouched, the context usable."""
    indptr, indices = random_csr(np.random.default_rng(5), 30, 40, 500)
    pay = make_payloads(np.random.default_rng(5), 500)
    bad = indptr.copy()
    bad[10], bad[11] = indptr[11] + 3, indptr[10]
    assert "indptr decreases" in transpose(ctx, 30, 40, bad, indices, pay, expect=abi.VTX_E_INVAL)
    bad = indptr.copy()
    bad[-1] = 499
    assert "indptr[n_major] != nnz" in transpose(ctx, 30, 40, bad, indices, pay, expect=abi.VTX_E_INVAL)
    bad = indptr.copy()
    bad[0] = 1
    assert "indptr[0] != 0" in transpose(ctx, 30, 40, bad, indices, pay, expect=abi.VTX_E_INVAL)
    bad = indices.copy()
    bad[321] = 40                                                        # == n_minor
    assert "index >= n_minor" in transpose(ctx, 30, 40, indptr, bad, pay, expect=abi.VTX_E_INVAL)
    assert "32-bit" in transpose(ctx, 30, 40, indptr, indices, pay, nnz=1 << 32, expect=abi.VTX_E_UNSUPPORTED)      # refused by its size alone
    d_ptr, d_idx, o_ptr, o_idx = dev_i64(indptr), dev_i32(indices), filled(41, torch.int64), filled(500, torch.int32)
    torch.cuda.synchronize()
    with pytest.raises(lib.VtxError) as e:                               # an element size other than 4 / 8
        ctx.csr_transpose(30, 40, 500, d_ptr.data_ptr(), d_idx.data_ptr(), o_ptr.data_ptr(), o_idx.data_ptr(), 0,
                          [(d_idx.data_ptr(), o_idx.data_ptr(), 2)])
    assert e.value.status == abi.VTX_E_INVAL and bool((o_ptr == PATTERN).all()) and bool((o_idx == PATTERN).all())
    check_case(ctx, 30, 40, indptr, indices, seed=5)                     # the context works afterwards
