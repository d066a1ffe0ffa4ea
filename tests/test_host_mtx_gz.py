"""vtxh_write_mtx_gz (libvtxhost.so): the host formatter's Matrix-Market text, gzip-compressed in BGZF framing by zlib on the
formatter's threads — what `vartrix --gzip` writes when the matrix does not come from the device.  Decompressed it must be
vtxh_write_mtx's file byte for byte; its compressed bytes are zlib's, not the device encoder's."""
import glob
import gzip
import os

import numpy as np
import pytest

import deflate_util as DU
from vartrix_amd import hostlib

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def both(tmp_path, n_rows, n_cols, row, col, val):
    p, q = str(tmp_path / "m.mtx"), str(tmp_path / "m.mtx.gz")
    hostlib.write_mtx(p, n_rows, n_cols, row, col, val)
    hostlib.write_mtx_gz(q, n_rows, n_cols, row, col, val)
    return open(p, "rb").read(), open(q, "rb").read()


def read_fixture(path):
    lines = open(path).read().split("\n")
    n_rows, n_cols, nnz = (int(x) for x in lines[2].split())
    body = [l.split() for l in lines[3:] if l]
    assert len(body) == nnz
    return (n_rows, n_cols, np.array([int(b[0]) - 1 for b in body], np.uint32), np.array([int(b[1]) - 1 for b in body], np.uint32),
            np.array([float(b[2]) for b in body], np.float64))


@pytest.mark.parametrize("name", sorted(os.path.basename(p) for p in glob.glob(os.path.join(G, "*.mtx"))))
def test_fixtures_round_trip(tmp_path, name):
    text, z = both(tmp_path, *read_fixture(os.path.join(G, name)))
    assert text == open(os.path.join(G, name), "rb").read()
    assert gzip.decompress(z) == text
    DU.check_bgzf(z, DU.cut(text))


def test_a_50000_line_alt_frac_matrix(tmp_path):
    """Several formatter threads are not reached below 65 536 lines, so a second size above it runs the threaded rounds as well."""
    rng = np.random.default_rng(3)
    for n in (50_000, 150_000):
        row = np.sort(rng.integers(0, 2_000_000, n)).astype(np.uint32)
        col = rng.integers(0, 9000, n).astype(np.uint32)
        val = rng.integers(0, 7, n) / rng.integers(1, 8, n)
        val[::97] = np.nan
        text, z = both(tmp_path, 2_000_000, 9000, row, col, val)
        assert text.count(b"\n") == n + 3 and b" NaN\n" in text
        assert gzip.decompress(z) == text and len(z) < len(text) / 2
        ms = DU.members(z)
        assert all(len(gzip.decompress(m)) <= DU.CHUNK for m in ms)


def test_an_empty_matrix_is_the_header_only(tmp_path):
    e32, e64 = np.zeros(0, np.uint32), np.zeros(0, np.float64)
    text, z = both(tmp_path, 12, 34, e32, e32, e64)
    assert text == b"%%MatrixMarket matrix coordinate real general\n% written by sprs\n12 34 0\n"
    assert gzip.decompress(z) == text
    DU.check_bgzf(z, [text])
