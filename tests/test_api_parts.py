"""The parts of the CSR interface that need no GPU: ``api.stack_parts`` against ``scipy.sparse.vstack``, the two new entry points
without a context, and the size of ``vtx_csr`` in ``vtx_abi_sizes``."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

from vartrix_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return lib.load()


def part_of(m):
    m = sp.csr_matrix(m)
    rng = np.random.default_rng(m.nnz)
    return {"indptr": m.indptr.astype(np.int64), "indices": m.indices.astype(np.int32), "value": m.data.astype(np.float64),
            "alt": rng.integers(0, 9, m.nnz).astype(np.int32)}


def random_rows(rng, n_rows, n_cols, density):
    m = sp.random(n_rows, n_cols, density=density, random_state=np.random.RandomState(int(rng.integers(1 << 30))), format="csr")
    m.data[:] = rng.integers(1, 4, m.nnz)
    return m


def check_stack(mats):
    from vartrix_amd import api
    parts = [part_of(m) for m in mats]
    before = [{k: v.copy() for k, v in p.items()} for p in parts]
    got = api.stack_parts(parts)
    want = sp.vstack(mats, format="csr")
    assert np.array_equal(got["indptr"], want.indptr) and got["indptr"].size == want.shape[0] + 1
    assert np.array_equal(got["indices"], want.indices)
    assert np.array_equal(got["value"], want.data)
    assert np.array_equal(got["alt"], np.concatenate([p["alt"] for p in parts]))
    for p, b in zip(parts, before):                      # pure: the parts are as they were
        assert all(np.array_equal(p[k], b[k]) for k in b)
    return got


def test_stack_parts_equals_scipy_vstack():
    rng = np.random.default_rng(5)
    n_cols = 13
    a, b, c = random_rows(rng, 7, n_cols, 0.3), random_rows(rng, 1, n_cols, 0.9), random_rows(rng, 20, n_cols, 0.1)
    check_stack([a, b, c])
    check_stack([a])                                                             # a single part
    empty = sp.csr_matrix((5, n_cols))
    check_stack([empty, a, empty, empty, c, empty])                              # parts without entries, also first and last
    check_stack([sp.csr_matrix((0, n_cols)), a, sp.csr_matrix((0, n_cols))])     # parts without rows
    tail = sp.vstack([random_rows(rng, 4, n_cols, 0.5), sp.csr_matrix((3, n_cols))], format="csr")
    got = check_stack([tail, b])                                                 # a part whose last rows are empty
    assert np.all(np.diff(got["indptr"])[4:7] == 0)


def test_stack_parts_on_torch_tensors_and_on_nothing():
    import torch
    from vartrix_amd import api
    rng = np.random.default_rng(6)
    mats = [random_rows(rng, 6, 9, 0.4), sp.csr_matrix((2, 9)), random_rows(rng, 3, 9, 0.4)]
    parts = [{k: torch.from_numpy(v) for k, v in part_of(m).items()} for m in mats]
    got = api.stack_parts(parts)
    want = sp.vstack(mats, format="csr")
    assert isinstance(got["indptr"], torch.Tensor) and got["indptr"].dtype == torch.int64
    assert np.array_equal(got["indptr"].numpy(), want.indptr) and np.array_equal(got["indices"].numpy(), want.indices)
    assert np.array_equal(got["value"].numpy(), want.data)
    none = api.stack_parts([])
    assert none["indptr"].tolist() == [0] and none["indices"].size == 0


def test_new_entry_points_without_a_context(L):
    """Like every other entry point: no context, VTX_E_INVAL — and nothing is dereferenced."""
    st = abi.VtxCsr()
    assert L.vtx_device_csr(None, 0, 1, C.byref(st)) == abi.VTX_E_INVAL
    assert L.vtx_csr_transpose(None, 1, 1, 0, None, None, None, None, None, None, None, None, 0) == abi.VTX_E_INVAL


def test_abi_sizes_report_vtx_csr(L):
    """sizeof(vtx_csr) is the 17th entry of vtx_abi_sizes; the 16 in front of it (the structs up to vtx_mtx_part) are as before, and a
    caller that asks for fewer gets fewer: the change is additive, VTX_ABI_VERSION stays."""
    out = (C.c_uint32 * 18)(*([0xDEAD] * 18))
    assert L.vtx_abi_sizes(out, 18) == abi.VTX_ABI_VERSION == 6
    assert out[16] == C.sizeof(abi.VtxCsr) == 80 and out[17] == 0xDEAD
    assert list(out)[:16] == [C.sizeof(abi.VtxConfig), abi.LOCUS_DTYPE.itemsize, abi.RECORD_DTYPE.itemsize, C.sizeof(abi.VtxBatch),
                              C.sizeof(abi.VtxCoo), C.sizeof(abi.VtxTiming), abi.RAW_RECORD_DTYPE.itemsize, C.sizeof(abi.VtxRawBatch),
                              C.sizeof(abi.VtxRawStats), abi.BGZF_BLOCK_DTYPE.itemsize, abi.BAM_INTERVAL_DTYPE.itemsize,
                              C.sizeof(abi.VtxBamIngest), C.sizeof(abi.VtxIngestStats), abi.BAM_SEGMENT_DTYPE.itemsize,
                              C.sizeof(abi.VtxBamSegments), C.sizeof(abi.VtxMtxPart)]
    few = (C.c_uint32 * 17)(*([0xDEAD] * 17))
    L.vtx_abi_sizes(few, 16)
    assert few[15] == C.sizeof(abi.VtxMtxPart) and few[16] == 0xDEAD


def test_header_and_binding_name_the_same_struct():
    """vtx_csr in include/vtx.h field by field against abi.VtxCsr (names and order)."""
    import re
    header = open(os.path.join(ROOT, "include", "vtx.h")).read()
    body = re.search(r"typedef struct vtx_csr \{(.*?)\} vtx_csr;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*([a-z_]+)\s*(?:,|$)", decl.strip())]
    assert names == [f for f, _ in abi.VtxCsr._fields_]
