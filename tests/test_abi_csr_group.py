"""The C-ABI surface of the pseudobulk calls without a GPU: the two constants, the entry points without a context in both builds of the
library, the header's and the binding's VTX_GROUP_NONE, and the table of ``vtx_abi_sizes`` unchanged (no new struct: ``vtx_csr_stats`` is
the output)."""
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


def test_window_and_largest_group_count(L):
    w = L.vtx_csr_group_window()
    assert w >= 64 and 1 <= L.vtx_csr_group_max() <= 256 * w          # at most 256 passes over a row
    assert L.vtx_csr_group_max() < abi.VTX_GROUP_NONE
    D = lib.load("dev")
    assert (D.vtx_csr_group_window(), D.vtx_csr_group_max()) == (w, L.vtx_csr_group_max())


def test_header_and_binding_agree_on_the_label_of_no_group():
    header = open(os.path.join(ROOT, "include", "vtx.h")).read()
    assert int(re.search(r"#define VTX_GROUP_NONE (0x[0-9A-Fa-f]+)u", header).group(1), 16) == abi.VTX_GROUP_NONE == 0xFFFFFFFF


def test_the_table_of_sizes_keeps_its_17_entries(L):
    out = (C.c_uint32 * 20)(*([0xDEAD] * 20))
    assert L.vtx_abi_sizes(out, 20) == abi.VTX_ABI_VERSION == 6
    assert out[16] == C.sizeof(abi.VtxCsr) and list(out)[17:] == [0xDEAD] * 3
    assert L.vtx_sizeof_csr_stats() == C.sizeof(abi.VtxCsrStats) == 56


@pytest.mark.parametrize("variant", ["", "dev"])
def test_entry_points_without_a_context(variant):
    """Like every other entry point: no context, VTX_E_INVAL — and nothing is dereferenced."""
    D = lib.load(variant)
    st = abi.VtxCsrStats()
    n = C.c_uint64(77)
    assert D.vtx_csr_group_plan(None, 1, 1, 0, None, None, None, 1, C.byref(n)) == abi.VTX_E_INVAL
    assert D.vtx_csr_group_sum(None, 1, 1, 0, None, None, None, None, None, None, 1, 0, None, None, C.byref(st)) == abi.VTX_E_INVAL
    assert n.value == 77
