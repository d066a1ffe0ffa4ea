"""The C-ABI surface of the doublet tally without a GPU: the largest pair count, the header's and the binding's VTX_GENO_PAIR_CLASSES, the
size of ``vtx_geno_pair_tally`` as the library reports it (a call of its own: the table of ``vtx_abi_sizes`` is unchanged), and the entry
point without a context in both builds of the library."""
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


def test_largest_pair_count(L):
    assert 64 <= L.vtx_csr_geno_pair_max() <= 4096          # at most 64 passes of a wavefront over a row
    assert lib.load("dev").vtx_csr_geno_pair_max() == L.vtx_csr_geno_pair_max()


def test_header_and_binding_agree_on_the_classes():
    header = open(os.path.join(ROOT, "include", "vtx.h")).read()
    assert int(re.search(r"#define VTX_GENO_PAIR_CLASSES (\d+)u", header).group(1)) == abi.GENO_PAIR_CLASSES == 6


def test_struct_matches_the_header_and_the_library(L):
    header = open(os.path.join(ROOT, "include", "vtx.h")).read()
    body = re.search(r"typedef struct vtx_geno_pair_tally \{(.*?)\} vtx_geno_pair_tally;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\*\s*([a-z_]+)", body)
    assert tuple(names) == abi.GENO_TALLY_NAMES == tuple(k for k, _ in abi.VtxGenoPairTally._fields_)
    assert L.vtx_sizeof_geno_pair_tally() == lib.load("dev").vtx_sizeof_geno_pair_tally() == C.sizeof(abi.VtxGenoPairTally) == 24
    # ... by a call of its own: the table of sizes keeps its 17 entries and the version stays
    out = (C.c_uint32 * 20)(*([0xDEAD] * 20))
    assert L.vtx_abi_sizes(out, 20) == abi.VTX_ABI_VERSION == 6
    assert out[16] == C.sizeof(abi.VtxCsr) and list(out)[17:] == [0xDEAD] * 3


def test_the_symbols_are_bound():
    assert {"vtx_csr_geno_pair_max", "vtx_sizeof_geno_pair_tally", "vtx_csr_geno_pair_tally"} <= set(lib.SYMBOLS)


@pytest.mark.parametrize("variant", ["", "dev"])
def test_entry_point_without_a_context(variant):
    """Like every other entry point: no context, VTX_E_INVAL — and nothing is dereferenced."""
    D = lib.load(variant)
    st = abi.VtxGenoPairTally()
    assert D.vtx_csr_geno_pair_tally(None, 1, 1, 0, None, None, None, None, None, 1, None, 1, C.byref(st)) == abi.VTX_E_INVAL
    assert D.vtx_csr_geno_pair_tally(None, 1, 1, 0, None, None, None, None, None, 1, None, 1, None) == abi.VTX_E_INVAL
