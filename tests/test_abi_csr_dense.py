"""The C-ABI surface of the CSR x integer-table sum without a GPU: the largest column count as the library, the binding and the header
state it, the header's declaration against the ctypes signature, the version and the table of sizes unchanged (the call takes no
struct), and the entry point without a context in both builds of the library."""
import ctypes as C
import os
import re

import pytest

from vartrix_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE = {"vtx_ctx*": C.c_void_p, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "const uint64_t*": C.c_void_p, "const uint32_t*": C.c_void_p,
         "const int32_t*": C.c_void_p, "int64_t*": C.c_void_p}


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return lib.load()


def test_largest_column_count(L):
    header = open(os.path.join(ROOT, "include", "vtx.h")).read()
    said = int(re.search(r"uint32_t vtx_csr_dense_max\(void\);\s*/\* the largest n_cols accepted: (\d+) \((\d+) passes of a wavefront\)", header).group(1))
    assert L.vtx_csr_dense_max() == abi.CSR_DENSE_MAX == said == 64 * 16      # 16 passes of a wavefront over a row
    assert lib.load("dev").vtx_csr_dense_max() == L.vtx_csr_dense_max()


def test_signature_matches_the_header(L):
    header = open(os.path.join(ROOT, "include", "vtx.h")).read()
    args = re.search(r"\nint vtx_csr_dense_sum\((.*?)\);", header, re.S).group(1)
    types, names = [], []
    for a in (" ".join(a.split()) for a in args.split(",")):
        kind, name = a.rsplit(" ", 1)
        types.append(CTYPE[kind])
        names.append(name)
    assert names == ["ctx", "n_major", "n_minor", "nnz", "d_indptr", "d_indices", "d_alt", "d_ref", "d_w_alt", "d_w_ref", "n_cols", "d_out"]
    assert L.vtx_csr_dense_sum.argtypes == types and L.vtx_csr_dense_sum.restype == C.c_int
    assert {"vtx_csr_dense_max", "vtx_csr_dense_sum"} <= set(lib.SYMBOLS)


def test_version_and_table_of_sizes_are_unchanged(L):
    out = (C.c_uint32 * 20)(*([0xDEAD] * 20))
    assert L.vtx_abi_sizes(out, 20) == abi.VTX_ABI_VERSION == 6
    assert out[16] == C.sizeof(abi.VtxCsr) and list(out)[17:] == [0xDEAD] * 3


@pytest.mark.parametrize("variant", ["", "dev"])
def test_entry_point_without_a_context(variant):
    """Like every other entry point: no context, VTX_E_INVAL — and nothing is dereferenced."""
    D = lib.load(variant)
    assert D.vtx_csr_dense_sum(None, 1, 1, 0, None, None, None, None, None, None, 1, None) == abi.VTX_E_INVAL
    assert D.vtx_csr_dense_sum(None, 0, 0, 0, None, None, None, None, None, None, 0, None) == abi.VTX_E_INVAL
