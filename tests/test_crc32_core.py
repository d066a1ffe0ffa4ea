"""CPU unit tests of vartrix_amd/csrc/vtx_crc32_core.h — the lane and wavefront logic bgzf_crc32_kernel is compiled from (the CRC32 of
every inflated BGZF block against its trailer: htslib's check in bgzf_read_block behind src/main.rs:822-830) — built for the host by
tests/crc32core/Makefile, against zlib.crc32: the GF(2) helpers, and the whole 64-lane decomposition (interleaved pieces, head mask,
front padding, butterfly, un-skip, tail) for each slicing width.  The device runs the same grid through the kernel in
tests/test_gpu_crc32.py."""
import ctypes as C
import os
import random
import subprocess
import zlib

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
WIDTHS = (4, 8, 16)


@pytest.fixture(scope="module")
def core():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "crc32core"), "-s"])
    L = C.CDLL(os.path.join(HERE, "crc32core", "libcrc32_host.so"))
    for name in ("vtxt_mulmod", "vtxt_mulx", "vtxt_divx", "vtxt_xpow8", "vtxt_combine"):
        getattr(L, name).restype = C.c_uint32
    L.vtxt_mulmod.argtypes = [C.c_uint32, C.c_uint32]
    L.vtxt_mulx.argtypes = L.vtxt_divx.argtypes = [C.c_uint32]
    L.vtxt_xpow8.argtypes = [C.c_uint64]
    L.vtxt_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
    L.vtxt_block_crc.argtypes = [C.c_int, C.c_char_p, C.c_uint64, C.c_uint32]
    L.vtxt_block_crc.restype = C.c_int64
    L.vtxt_cut.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    L.vtxt_cut.restype = C.c_int
    return L


def corpus(rng, kind, n):
    if kind == "random":
        return rng.randbytes(n)
    if kind == "acgt":
        return bytes(rng.choice(b"ACGT") for _ in range(n)) if n < 2000 else (bytes(rng.choice(b"ACGT") for _ in range(1999)) * (n // 1999 + 1))[:n]
    return (b"\x00" if kind == "zero" else b"\xff") * n


def block_crc(L, w, data, misalign):
    got = L.vtxt_block_crc(w, data, len(data), misalign)
    assert got >= 0
    return got


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("kind", ["random", "acgt", "zero", "ff"])
def test_every_length_to_300_at_every_misalignment(core, w, kind):
    rng = random.Random(w * 100 + len(kind))
    for n in range(301):
        data = corpus(rng, kind, n)
        want = zlib.crc32(data)
        for m in (range(16) if n < 40 or n % 16 == 0 else (rng.randrange(16), rng.randrange(16))):
            assert block_crc(core, w, data, m) == want, (w, kind, n, m)


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("kind", ["random", "acgt", "zero", "ff"])
def test_lengths_up_to_a_full_bgzf_block(core, w, kind):
    """Random lengths up to 65536 with 65280 (htslib's block size) and 65536, around every row boundary of the lane grid (64 W bytes),
    random misalignments 0..15 (and beyond: whole pieces of offset)."""
    rng = random.Random(w * 1000 + len(kind))
    lengths = [65280, 65536, 65535, 64 * w - 1, 64 * w, 64 * w + 1, 128 * w - 1, 128 * w + 1, 63 * w, 65 * w] + \
              [rng.randrange(301, 65537) for _ in range(24)]
    for n in lengths:
        data = corpus(rng, kind, n)
        for m in (rng.randrange(16), rng.randrange(16), 16 * rng.randrange(1, 70) + rng.randrange(16)):
            assert block_crc(core, w, data, m) == zlib.crc32(data), (w, kind, n, m)


@pytest.mark.parametrize("w", WIDTHS)
def test_the_cut_of_a_block(core, w):
    """The lane-chunk rules as numbers: pieces are W-aligned, the padding sits in front and fills the first row only, the tail is
    shorter than W (or the whole of a block that holds no aligned piece), and nothing in front of start & ~(W - 1) is addressed."""
    rng = random.Random(w)
    out = (C.c_uint64 * 6)()
    for _ in range(3000):
        s = rng.randrange(0, 5000)
        n = rng.choice([0, 1, rng.randrange(0, 3 * w), rng.randrange(0, 70000)])
        assert core.vtxt_cut(w, s, s + n, out) == 0
        a0, head, n_pieces, rows, pad, tail_begin = (int(v) for v in out)
        assert a0 % w == 0 and a0 <= s < a0 + w and head == s - a0
        assert rows == (n_pieces + 63) // 64 and pad == rows * 64 - n_pieces and 0 <= pad < 64
        if n_pieces:
            assert tail_begin == a0 + w * n_pieces and tail_begin % w == 0 and s < tail_begin <= s + n and s + n - tail_begin < w
        else:
            assert tail_begin == s and n < 2 * w


def test_mulmod_and_xpow8_against_repeated_multiplication(core):
    rng = random.Random(5)
    one, x = 0x80000000, 0x40000000
    for _ in range(200):
        a, b, c = (rng.getrandbits(32) for _ in range(3))
        assert core.vtxt_mulmod(a, one) == a and core.vtxt_mulmod(one, a) == a
        assert core.vtxt_mulmod(a, b) == core.vtxt_mulmod(b, a)
        assert core.vtxt_mulmod(a, b ^ c) == core.vtxt_mulmod(a, b) ^ core.vtxt_mulmod(a, c)
        assert core.vtxt_mulmod(core.vtxt_mulmod(a, b), c) == core.vtxt_mulmod(a, core.vtxt_mulmod(b, c))
        assert core.vtxt_mulmod(a, x) == core.vtxt_mulx(a) and core.vtxt_divx(core.vtxt_mulx(a)) == a and core.vtxt_mulx(core.vtxt_divx(a)) == a
    x8, p = core.vtxt_xpow8(1), one
    assert x8 == 0x00800000
    for n in range(0, 2100):                      # x^(8 n) = x^8 * x^8 * ...
        assert core.vtxt_xpow8(n) == p, n
        p = core.vtxt_mulmod(p, x8)
    for n in (65536, 65280, 1 << 20, (1 << 32) + 12345):
        assert core.vtxt_xpow8(n) == core.vtxt_mulmod(core.vtxt_xpow8(n - 1000), core.vtxt_xpow8(1000))


def test_combine_against_zlib_on_random_splits(core):
    rng = random.Random(6)
    for _ in range(300):
        n = rng.choice([0, 1, 2, rng.randrange(0, 400), rng.randrange(0, 70000)])
        data = rng.randbytes(n)
        cut = rng.randrange(0, n + 1)
        a, b = data[:cut], data[cut:]
        assert core.vtxt_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(data), (n, cut)
