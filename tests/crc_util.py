"""Inputs for the CRC32 tests (tests/test_host_crc.py, tests/test_gpu_crc32.py): BAMs whose BGZF blocks are written STORED (deflate
level 0: a flipped payload bit still inflates, to one wrong byte), the table of a file's blocks, and the two kinds of damage that only
the CRC32 of a block's trailer can notice."""
import contextlib
import struct
import zlib


def stored_bgzf_block(data: bytes) -> bytes:
    co = zlib.compressobj(0, zlib.DEFLATED, -15)
    cdata = co.compress(data) + co.flush()
    hdr = struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(cdata) + 25)
    return hdr + cdata + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


@contextlib.contextmanager
def stored_blocks():
    """oracle.bamwriter writes stored blocks inside this context (its index follows the blocks' real sizes)."""
    from oracle import bamwriter
    keep = bamwriter._bgzf_block
    bamwriter._bgzf_block = stored_bgzf_block
    try:
        yield
    finally:
        bamwriter._bgzf_block = keep


def blocks_of(raw: bytes):
    """Every BGZF block: dict(index, start = file offset of its header, coff / clen = its payload, isize)."""
    o, out = 0, []
    while o + 18 <= len(raw):
        xlen = struct.unpack_from("<H", raw, o + 10)[0]
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        out.append(dict(index=len(out), start=o, coff=o + 12 + xlen, clen=bsize - 12 - xlen - 8,
                        isize=struct.unpack_from("<I", raw, o + bsize - 4)[0]))
        o += bsize
    assert o == len(raw)
    return out


def first_middle_last(blocks):
    d = [b for b in blocks if b["isize"]]
    return {"first": d[0], "middle": d[len(d) // 2], "last": d[-1]}


def flip_trailer(raw: bytearray, b):
    """One bit of the block's CRC32 field."""
    raw[b["coff"] + b["clen"] + 1] ^= 0x10


def flip_stored_payload(raw: bytearray, b, at=None):
    """One bit of a data byte of a STORED block (5 bytes of stored-block header, then the bytes themselves): it still inflates."""
    assert b["clen"] >= b["isize"] + 5 and raw[b["coff"]] & 6 == 0, "not a stored block"
    at = b["isize"] // 2 if at is None else at
    assert 0 <= at < min(b["isize"], 65535)
    raw[b["coff"] + 5 + at] ^= 0x04


def refresh_trailer(raw: bytearray, b):
    """The trailer a writer would have put behind the block's present payload (what a reader that ignores the CRC32 sees)."""
    data = zlib.decompress(bytes(raw[b["coff"]:b["coff"] + b["clen"]]), -15)
    struct.pack_into("<I", raw, b["coff"] + b["clen"], zlib.crc32(data) & 0xFFFFFFFF)
