"""vtx_write_mtx_f64 in the C-ABI: declared in include/vtx.h, listed in the binding, exported by the production library, the developer
library and the band-semantics variants (they link the same vtx_api.o / vtx_ingest.o).  tests/test_abi.py's scan of the header reads
names of [a-z_] only, so the names with a digit (lib.SYMBOLS_ALNUM) get the same comparison here.  The slab hook VTX_MTX_SLAB is a
developer hook: libvtx_dev.so only (tests/test_abi.py checks that for every VTX_DEV_ENV of vtx_api.hip, this one included)."""
import ctypes as C
import inspect
import os
import re

from vartrix_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_every_library_agree_on_the_names_with_digits():
    header = open(os.path.join(ROOT, "include", "vtx.h")).read()
    declared = set(re.findall(r"\b(vtx_[a-z0-9_]+)\s*\(", header)) - {"vtx_ctx"}
    assert declared == set(lib.SYMBOLS) | set(lib.SYMBOLS_ALNUM)
    assert "vtx_write_mtx_f64" in lib.SYMBOLS_ALNUM and not set(lib.SYMBOLS) & set(lib.SYMBOLS_ALNUM)
    for variant in ("", "dev", "lazy0", "lazy40", "anchor5", "noseed0"):
        L = lib.load(variant)
        for name in lib.SYMBOLS_ALNUM:
            assert hasattr(L, name), (variant, name)
    f = lib.load("").vtx_write_mtx_f64
    assert f.restype is C.c_int and len(f.argtypes) == 6 and list(f.argtypes) == list(lib.load("").vtx_write_mtx.argtypes)


def test_write_mtx_has_the_real_keyword_and_declines_without_a_run():
    sig = inspect.signature(lib.Context.write_mtx)
    assert sig.parameters["real"].default is False
    # no context: the entry point answers VTX_E_INVAL before it touches a device (like every other one)
    assert lib.load("").vtx_write_mtx_f64(None, b"/nonexistent/x.mtx", 1, 1, 0, None) != 0


def test_slab_hook_is_a_developer_hook():
    here = os.path.dirname(lib.lib_path(""))
    assert b"VTX_MTX_SLAB" not in open(os.path.join(here, "libvtx.so"), "rb").read()
    assert b"VTX_MTX_SLAB" in open(os.path.join(here, "libvtx_dev.so"), "rb").read()
    src = open(os.path.join(ROOT, "vartrix_amd", "csrc", "vtx_api.hip")).read()
    assert 'VTX_DEV_ENV("VTX_MTX_SLAB")' in src
