"""A matrix written in PARTS, the host side (no GPU): vtxh_mtx_part formats the triplets of one run as a finished piece of the
Matrix-Market file — the lines alone, or their BGZF members — and vtx_mtx_join writes the pieces behind a header.  Whatever the cuts,
the joined plain file must be vtxh_write_mtx's of all the triplets byte for byte (sprs::io::write_matrix_market, src/main.rs:381-389),
the joined gzip file must decompress to it and be valid BGZF member by member; the error cases leave nothing behind; and the same
calls run clean as a stand-alone program under AddressSanitizer and UBSan (tests/mtxparts/).  The device-made parts are
tests/test_gpu_mtx_parts.py's."""
import ctypes as C
import gzip
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import deflate_util as DU
from vartrix_amd import abi, hostlib, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS, N_COLS = 500, 300


@pytest.fixture(scope="module", autouse=True)
def built():
    if not (os.path.exists(hostlib.LIB_PATH) and os.path.exists(lib.LIB_PATH)):
        import __graft_entry__
        __graft_entry__.build()


def header(nnz, n_rows=N_ROWS, n_cols=N_COLS):
    return b"%%%%MatrixMarket matrix coordinate real general\n%% written by sprs\n%d %d %d\n" % (n_rows, n_cols, nnz)


@pytest.fixture(scope="module")
def triplets():
    """About 9 000 triplets in row order (then column order): alt_frac's values — NaN, thirds, 0, 1 — and counts."""
    rng = np.random.default_rng(11)
    cells = np.sort(rng.choice(N_ROWS * N_COLS, 9000, replace=False))
    row, col = (cells // N_COLS).astype(np.uint32), (cells % N_COLS).astype(np.uint32)
    pool = np.array([float("nan"), 1 / 3, 2 / 3, 0.0, 1.0, 0.5, 2.0, 3.0, 17.0, 1 / 7, 0.000033333333333333335, 4096.0])
    value = pool[rng.integers(0, len(pool), len(cells))]
    assert np.isnan(value).any() and (value == 0).any()
    return row, col, value


def cuts_for(n_parts, nnz, seed):
    """n_parts + 1 ascending cut points; seven parts: an empty one in front, one in the middle and one at the end."""
    rng = np.random.default_rng(seed)
    if n_parts == 7:
        x, y, z = np.sort(rng.choice(np.arange(1, nnz), 3, replace=False))
        return [0, 0, int(x), int(y), int(y), int(z), nnz, nnz]
    return [0] + sorted(int(c) for c in rng.choice(np.arange(1, nnz), n_parts - 1, replace=False)) + [nnz]


def whole_text(tmp_path, row, col, value):
    p = str(tmp_path / "whole.mtx")
    hostlib.write_mtx(p, N_ROWS, N_COLS, row, col, value)
    return open(p, "rb").read()


def make_parts(row, col, value, cuts, gz):
    return [hostlib.mtx_part(row[a:b], col[a:b], value[a:b], gz=gz) for a, b in zip(cuts, cuts[1:])]


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def seq_sum(v):
    """`sum += v` in order, as the host formatter adds (NaN once a value is NaN)."""
    s = 0.0
    for x in v:
        s += float(x)
    return s


@pytest.mark.parametrize("n_parts", [1, 2, 7])
def test_plain_parts_joined_equal_the_whole_file(tmp_path, triplets, n_parts):
    row, col, value = triplets
    want = whole_text(tmp_path, row, col, value)
    cuts = cuts_for(n_parts, len(row), seed=n_parts)
    parts = make_parts(row, col, value, cuts, gz=False)
    for p, a, b in zip(parts, cuts, cuts[1:]):
        assert p.nnz == b - a and not p.gz and p.text_bytes == len(p.bytes) and p.bytes.count(b"\n") == b - a
        assert same(p.sum, seq_sum(value[a:b]))
        assert (b > a) == bool(p.bytes)
    out = str(tmp_path / "joined.mtx")
    nbytes = lib.mtx_join(out, N_ROWS, N_COLS, parts)
    got = open(out, "rb").read()
    assert got == want and nbytes == len(want)
    assert got.startswith(header(len(row))) and b"".join(p.bytes for p in parts) == want[len(header(len(row))):]


@pytest.mark.parametrize("n_parts", [1, 2, 7])
def test_gz_parts_joined_decompress_to_the_whole_file(tmp_path, triplets, n_parts):
    row, col, value = triplets
    want = whole_text(tmp_path, row, col, value)
    cuts = cuts_for(n_parts, len(row), seed=10 + n_parts)
    parts = make_parts(row, col, value, cuts, gz=True)
    texts = make_parts(row, col, value, cuts, gz=False)
    for p, t in zip(parts, texts):
        assert p.gz and p.nnz == t.nnz and p.text_bytes == len(t.bytes) and same(p.sum, t.sum)
        assert bool(p.bytes) == bool(t.bytes)                      # an empty part has no member
    out = str(tmp_path / "joined.mtx.gz")
    nbytes = lib.mtx_join(out, N_ROWS, N_COLS, parts, gz=True)
    z = open(out, "rb").read()
    assert gzip.decompress(z) == want and nbytes == len(want)
    chunks = [header(len(row))]
    for t in texts:
        if t.bytes:
            chunks += DU.cut(t.bytes)
    kinds = DU.check_bgzf(z, chunks)
    assert kinds[0] == 0                                           # the header lines: a member of their own, one stored block
    # the host gzip writer of the whole list decompresses to the same text (one formatter behind both)
    hostlib.write_mtx_gz(str(tmp_path / "whole.mtx.gz"), N_ROWS, N_COLS, row, col, value)
    assert gzip.decompress(open(str(tmp_path / "whole.mtx.gz"), "rb").read()) == want


@pytest.mark.parametrize("gz", [False, True])
def test_no_parts_and_empty_parts_give_the_header_alone(tmp_path, gz):
    e = np.zeros(0, np.uint32)
    for name, parts in (("none", []), ("empty", [hostlib.mtx_part(e, e, np.zeros(0), gz=gz) for _ in range(3)])):
        out = str(tmp_path / name)
        nbytes = lib.mtx_join(out, 12, 34, parts, gz=gz)
        data = open(out, "rb").read()
        text = header(0, 12, 34)
        assert nbytes == len(text) and text.count(b"\n") == 3
        if gz:
            assert gzip.decompress(data) == text
            DU.check_bgzf(data, [text])
        else:
            assert data == text


def test_a_part_of_the_other_kind_is_refused_and_leaves_no_file(tmp_path, triplets):
    row, col, value = triplets
    for gz in (False, True):
        parts = [hostlib.mtx_part(row[:100], col[:100], value[:100], gz=gz), hostlib.mtx_part(row[100:200], col[100:200], value[100:200], gz=not gz)]
        out = str(tmp_path / ("mixed%d" % gz))
        with pytest.raises(lib.VtxError) as e:
            lib.mtx_join(out, N_ROWS, N_COLS, parts, gz=gz)
        assert e.value.status == abi.VTX_E_INVAL and "part 1" in str(e.value) and not os.path.exists(out)


def test_an_unwritable_path_is_an_error_and_leaves_no_file(tmp_path, triplets):
    row, col, value = triplets
    parts = [hostlib.mtx_part(row[:50], col[:50], value[:50])]
    out = str(tmp_path / "no_such_dir" / "m.mtx")
    with pytest.raises(lib.VtxError) as e:
        lib.mtx_join(out, N_ROWS, N_COLS, parts)
    assert e.value.status == abi.VTX_E_INVAL and not os.path.exists(out) and not os.path.exists(os.path.dirname(out))
    lib.mtx_join(str(tmp_path / "after.mtx"), N_ROWS, N_COLS, parts)                  # (no state: the next call works)
    assert open(str(tmp_path / "after.mtx"), "rb").read() == header(50) + parts[0].bytes


def test_a_large_join_written_by_several_threads(tmp_path):
    """Above 16 MiB vtx_mtx_join writes slices of the parts from several threads at their offsets: the file is still the parts in order
    behind the header (three parts of about 8 MiB of text, the middle one longer than a slice)."""
    rng = np.random.default_rng(3)
    n = 1_900_000
    cells = np.sort(rng.choice(40_000 * 5_000, n, replace=False))
    row, col = (cells // 5_000).astype(np.uint32), (cells % 5_000).astype(np.uint32)
    value = rng.integers(1, 4, n).astype(np.float64)
    cuts = [0, 500_000, 1_400_000, n]
    for gz in (False, True):
        parts = make_parts(row, col, value, cuts, gz=gz)
        out = str(tmp_path / ("big%d" % gz))
        nbytes = lib.mtx_join(out, 40_000, 5_000, parts, gz=gz)
        data = open(out, "rb").read()
        if gz:
            assert data.endswith(DU.EOF_BLOCK) and data[-28 - len(parts[2].bytes):-28] == parts[2].bytes
            data = gzip.decompress(data)
        else:
            assert len(data) > (16 << 20) and len(parts[1].bytes) > (8 << 20)
            text = data
        assert data == header(n, 40_000, 5_000) + text[len(header(n, 40_000, 5_000)):] and nbytes == len(data)
    assert text == header(n, 40_000, 5_000) + b"".join(p.bytes for p in make_parts(row, col, value, cuts, gz=False))
    assert data == text


def test_the_bindings_follow_the_headers():
    """sizeof(struct vtx_mtx_part) is the 16th entry of vtx_abi_sizes (the first 15 as before); vtx_host.h's production entry points are
    hostlib.SYMBOLS, all exported; the developer library exports the new calls too."""
    L = lib.load()
    out = (C.c_uint32 * 16)()
    assert L.vtx_abi_sizes(out, 16) == abi.VTX_ABI_VERSION
    assert out[15] == C.sizeof(abi.VtxMtxPart) == 48 and list(out[12:15]) == [C.sizeof(abi.VtxIngestStats), abi.BAM_SEGMENT_DTYPE.itemsize, C.sizeof(abi.VtxBamSegments)]
    for name in ("vtx_mtx_part", "vtx_mtx_part_free", "vtx_mtx_join"):
        assert name in lib.SYMBOLS and hasattr(L, name) and hasattr(lib.load("dev"), name)
    head = open(os.path.join(ROOT, "include", "vtx_host.h")).read()
    head = head[:head.index("#ifdef VTX_DEVTOOLS")]
    declared = set(re.findall(r"\b(vtxh_[a-z0-9_]+)\s*\(", head))
    assert declared == set(hostlib.SYMBOLS)
    H = hostlib.load()
    for name in declared:
        assert hasattr(H, name), name


def test_the_decline_hook_is_a_developer_hook():
    """VTX_MTX_PART_DECLINE (the k-th vtx_mtx_part of a process declines: the only way to reach the command line's host fallback) exists
    in libvtx_dev.so only."""
    here = os.path.dirname(lib.lib_path(""))
    assert b"VTX_MTX_PART_DECLINE" not in open(os.path.join(here, "libvtx.so"), "rb").read()
    assert b"VTX_MTX_PART_DECLINE" in open(os.path.join(here, "libvtx_dev.so"), "rb").read()


def test_parts_and_join_under_the_sanitizers(tmp_path, triplets):
    """The same calls on the same inputs in a stand-alone program built with -fsanitize=address,undefined (host code only): its joined
    files are this process's, byte for byte."""
    row, col, value = triplets
    d = os.path.join(ROOT, "tests", "mtxparts")
    subprocess.check_call(["make", "-C", d, "-s", "mtx_parts_san"])
    for n_parts in (1, 7):
        cuts = cuts_for(n_parts, len(row), seed=20 + n_parts)
        src, outdir = str(tmp_path / ("in%d.bin" % n_parts)), str(tmp_path / ("out%d" % n_parts))
        os.mkdir(outdir)
        with open(src, "wb") as f:
            f.write(struct.pack("<IIQI", N_ROWS, N_COLS, len(row), len(cuts)) + np.asarray(cuts, np.uint64).tobytes())
            f.write(row.tobytes() + col.tobytes() + value.tobytes())
        r = subprocess.run([os.path.join(d, "mtx_parts_san"), src, outdir], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        want = whole_text(tmp_path, row, col, value)
        assert open(os.path.join(outdir, "joined.mtx"), "rb").read() == open(os.path.join(outdir, "whole.mtx"), "rb").read() == want
        z = open(os.path.join(outdir, "joined.mtx.gz"), "rb").read()
        mine = str(tmp_path / ("mine%d.gz" % n_parts))
        lib.mtx_join(mine, N_ROWS, N_COLS, make_parts(row, col, value, cuts, gz=True), gz=True)
        assert z == open(mine, "rb").read() and gzip.decompress(z) == want
        assert gzip.decompress(open(os.path.join(outdir, "whole.mtx.gz"), "rb").read()) == want
    # no triplets at all: one cut point, no part
    src, outdir = str(tmp_path / "in0.bin"), str(tmp_path / "out0")
    os.mkdir(outdir)
    open(src, "wb").write(struct.pack("<IIQI", 12, 34, 0, 1) + np.zeros(1, np.uint64).tobytes())
    r = subprocess.run([os.path.join(d, "mtx_parts_san"), src, outdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert open(os.path.join(outdir, "joined.mtx"), "rb").read() == header(0, 12, 34)
