"""CPU unit tests of vartrix_amd/csrc/vtx_crc32_core.h — the lane and wavefront logic bgzf_crc32_kernel is compiled from (the CRC32 of
every inflated BGZF block against its trailer: htslib's check in bgzf_read_block behind src/main.rs:822-830) — built for the host by
tests/crc32core/Makefile, against zlib.crc32: the GF(2) helpers, and the whole 64-lane decomposition (interleaved pieces, head mask,
front padding, butterfly, un-skip, tail) for each slicing width.  The device runs the same grid through the kernel in
tests/test_gpu_crc32.py.  What the wavefront TOUCHES is checked by a stand-alone program (tests/crc32core/main.cpp) in allocations of
exactly the device's size, plain and under AddressSanitizer and UBSan; nothing sanitized is loaded into Python."""
import ctypes as C
import os
import random
import struct
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


def run_program(cases, tmp, san):
    """cases: [(W, s, data, total, fill)] through tests/crc32core/main.cpp in ONE process -> [crc]."""
    name = "crc32_host_san" if san else "crc32_host"
    subprocess.check_call(["make", "-C", os.path.join(HERE, "crc32core"), "-s", name])
    src, dst = os.path.join(tmp, name + ".in"), os.path.join(tmp, name + ".out")
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for w, s, data, total, fill in cases:
            f.write(struct.pack("<IIIII", w, s, len(data), total, fill) + data)
    r = subprocess.run([os.path.join(HERE, "crc32core", name), src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, "exit %d\n%s" % (r.returncode, r.stderr[-4000:])
    out = open(dst, "rb").read()
    assert len(out) == 4 * len(cases)
    return list(struct.unpack("<%dI" % len(cases), out))


def test_the_wavefront_reads_nothing_outside_the_inflated_buffer(tmp_path):
    """Every length 0..300 and the edge lengths at every misalignment 0..15, each width, the block FIRST in its buffer (its head
    read, down to start & ~(W - 1), starts at the allocation's base; other bytes follow) and LAST (other bytes in front; it ends
    at total, the allocation at total + 64, as d_bam_data's does), the other bytes 00, FF or A5: the stand-alone program gives
    zlib.crc32, and its build under AddressSanitizer and UBSan exits 0 without a report and gives the same."""
    rng = random.Random(12)
    blobs = {n: rng.randbytes(n) for n in list(range(301)) + [65280, 65535, 65536]}
    cases, want = [], []
    for w in WIDTHS:
        edges = [65280, 65536, 65535, 64 * w - 1, 64 * w, 64 * w + 1, 128 * w - 1, 128 * w + 1, 63 * w, 65 * w]
        for n in list(range(301)) + edges:
            data = blobs.setdefault(n, rng.randbytes(n))
            for m in (range(16) if n <= 300 else (0, 1, w - 1, 15)):
                fill = (0x00, 0xFF, 0xA5)[(n + m) % 3]
                cases.append((w, m, data, m + n + 37, fill))               # first
                cases.append((w, 32 + m, data, 32 + m + n, fill))          # last
                if n % 50 == 0:
                    cases.append((w, m, data, m + n, fill))                # alone: first and last
                want += [zlib.crc32(data)] * (len(cases) - len(want))
    assert len(cases) > 28000
    plain = run_program(cases, str(tmp_path), san=False)
    assert plain == want, next((c[:2] + (len(c[2]),) + c[3:]) for c, g, e in zip(cases, plain, want) if g != e)
    assert run_program(cases, str(tmp_path), san=True) == want
