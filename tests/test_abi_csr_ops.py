"""The C-ABI surface of the CSR summaries and selections without a GPU: ``vtx_csr_stats`` in include/vtx.h field by field against
``abi.VtxCsrStats``, its size as the library reports it, the table of ``vtx_abi_sizes`` unchanged, and the three entry points without a
context."""
import ctypes as C
import os
import re

import pytest

from vartrix_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return lib.load()


def test_header_and_binding_name_the_same_struct(L):
    header = open(os.path.join(ROOT, "include", "vtx.h")).read()
    body = re.search(r"typedef struct vtx_csr_stats \{(.*?)\} vtx_csr_stats;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*\s*([a-z_]+)\s*(?:,|$)", decl.strip())]
    assert names == [f for f, _ in abi.VtxCsrStats._fields_] == list(abi.CSR_STAT_NAMES)
    assert [t._type_ for _, t in abi.VtxCsrStats._fields_] == [C.c_uint32] * 4 + [C.c_uint64] * 3
    assert L.vtx_sizeof_csr_stats() == C.sizeof(abi.VtxCsrStats) == 56


def test_the_table_of_sizes_keeps_its_17_entries(L):
    out = (C.c_uint32 * 20)(*([0xDEAD] * 20))
    assert L.vtx_abi_sizes(out, 20) == abi.VTX_ABI_VERSION == 6
    assert out[16] == C.sizeof(abi.VtxCsr) and list(out)[17:] == [0xDEAD] * 3


@pytest.mark.parametrize("variant", ["", "dev"])
def test_entry_points_without_a_context(variant):
    """Like every other entry point: no context, VTX_E_INVAL — and nothing is dereferenced."""
    D = lib.load(variant)
    st = abi.VtxCsrStats()
    a, b, n = C.c_uint32(), C.c_uint32(), C.c_uint64()
    assert D.vtx_csr_row_stats(None, 1, 1, 0, None, None, None, None, None, C.byref(st)) == abi.VTX_E_INVAL
    assert D.vtx_csr_select_plan(None, 1, 1, 0, None, None, None, None, C.byref(a), C.byref(b), C.byref(n)) == abi.VTX_E_INVAL
    assert D.vtx_csr_select(None, 1, 1, 0, None, None, None, None, 1, 1, 0, None, None, None, None, None, None, None, 0) == abi.VTX_E_INVAL
