"""Shared by tests/test_deflate_core.py and tests/test_gpu_mtx_gz.py: the stand-alone host build of vartrix_amd/csrc/vtx_deflate_core.h
(tests/deflatecore/) and the checks every BGZF file of this project must pass, with Python's zlib as the judge."""
import gzip
import os
import struct
import subprocess
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
CHUNK = 65280
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")


def harness(san=False):
    name = "deflate_host_san" if san else "deflate_host"
    subprocess.check_call(["make", "-C", os.path.join(HERE, "deflatecore"), "-s", name])
    return os.path.join(HERE, "deflatecore", name)


def encode_many(inputs, tmp, san=False):
    """Every input through the host encoder in ONE process: the BGZF bytes (members + EOF block) per input."""
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        for b in inputs:
            f.write(struct.pack("<I", len(b)) + b)
    r = subprocess.run([harness(san), src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out, p, res = open(dst, "rb").read(), 0, []
    for _ in inputs:
        m, = struct.unpack_from("<I", out, p)
        res.append(out[p + 4:p + 4 + m])
        p += 4 + m
    assert p == len(out)
    return res


def encode_file(text, tmp):
    """One text -> the BGZF file the host encoder makes of it (chunks of 65 280 bytes from its start)."""
    src, dst = os.path.join(tmp, "text.bin"), os.path.join(tmp, "text.gz")
    open(src, "wb").write(text)
    r = subprocess.run([harness(), "--file", src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return open(dst, "rb").read()


def members(z):
    """[(member bytes)] of a BGZF file, the EOF block checked and left out; the fixed header bytes and BSIZE checked by hand."""
    assert z.endswith(EOF_BLOCK)
    p, out = 0, []
    while p < len(z) - len(EOF_BLOCK):
        assert z[p:p + 16] == HEAD, p
        bsize = struct.unpack_from("<H", z, p + 16)[0] + 1
        assert 26 <= bsize and p + bsize <= len(z) - len(EOF_BLOCK)
        out.append(z[p:p + bsize])
        p += bsize
    return out


def check_bgzf(z, chunks, inflate=None):
    """z holds one member per chunk, in order: each member's DEFLATE stream gives its chunk (eof, nothing unused), CRC32 and ISIZE are
    zlib.crc32's and the length, the member is at most n + 31 bytes; gzip reads the whole.  inflate(stream, n) -> bytes or None:
    a second decoder that must agree.  Returns the block type (0 stored, 1 fixed, 2 dynamic) per member."""
    ms = members(z)
    assert len(ms) == len(chunks), (len(ms), len(chunks))
    kinds = []
    for m, c in zip(ms, chunks):
        stream = m[18:-8]
        d = zlib.decompressobj(-15)
        assert d.decompress(stream) == c and d.eof and d.unused_data == b"" and d.unconsumed_tail == b""
        assert struct.unpack("<II", m[-8:]) == (zlib.crc32(c), len(c))
        assert len(m) <= len(c) + 31, (len(m), len(c))
        assert stream[0] & 1 == 1                       # BFINAL: one block per member
        kinds.append((stream[0] >> 1) & 3)
        if inflate is not None:
            assert inflate(stream, len(c)) == c
    assert gzip.decompress(z) == b"".join(chunks)
    return kinds


def cut(b, size=CHUNK):
    """The chunks of one input (an empty input is one empty chunk)."""
    return [b[i:i + size] for i in range(0, len(b), size)] or [b""]


def zlib1_stream_bytes(chunks):
    """Bytes of zlib's raw deflate at level 1 over the same chunks (the yardstick of the compressed size)."""
    total = 0
    for c in chunks:
        z = zlib.compressobj(1, zlib.DEFLATED, -15)
        total += len(z.compress(c)) + len(z.flush())
    return total
