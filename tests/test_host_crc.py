"""The host packer verifies the CRC32 of every BGZF block it inflates (htslib's check in bgzf_read_block; in the reference a mismatch
is the Err of `let rec = _rec?`, src/main.rs:829-830): an authored BAM packs, the same file with ONE bit flipped — in a trailer's
CRC32 field, or in the payload of a block written stored, which still inflates — fails with the file, the block's offset and the word
CRC32, whichever block carries the damage.  And the damage was silent before: the stored-payload flip behind a trailer that matches
the damaged bytes (what a reader that ignores the trailer sees) packs, to a different batch."""
import os
import struct

import numpy as np
import pytest

from tests import crc_util
from tests.test_host import make_dna_bam
from vartrix_amd import hostlib

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def inputs(bam):
    return dict(vcf=os.path.join(G, "test_dna.vcf"), bam=bam, fasta=os.path.join(G, "test_dna.fa"),
                cell_barcodes=os.path.join(G, "dna_barcodes.tsv"))


@pytest.fixture()
def stored_bam(tmp_path):
    with crc_util.stored_blocks():
        bam = make_dna_bam(tmp_path, seed=4, n_reads=900)
    raw = open(bam, "rb").read()
    blocks = crc_util.blocks_of(raw)
    assert len([b for b in blocks if b["isize"]]) >= 5 and blocks[-1]["isize"] == 0
    return bam, raw, blocks


def raw_pack(bam, **kw):
    batch, metrics, *_ = hostlib.pack_files(raw=True, nibbles=True, threads=3, **inputs(bam), **kw)
    return batch, metrics


def same_raw(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("loci", "records", "hap_arena", "read_arena", "tag_arena"))


def write_copy(tmp_path, name, bam, raw):
    p = str(tmp_path / name)
    open(p, "wb").write(bytes(raw))
    open(p + ".bai", "wb").write(open(bam + ".bai", "rb").read())
    return p


def test_an_authored_bam_packs_whatever_its_blocks_are(tmp_path, stored_bam):
    bam, raw, blocks = stored_bam
    (tmp_path / "deflated").mkdir()
    deflated = make_dna_bam(tmp_path / "deflated", seed=4, n_reads=900)
    a, ma = raw_pack(bam)
    b, mb = raw_pack(deflated)
    assert same_raw(a, b) and ma == mb and a.n_records > 200
    hostlib.pack_files(threads=2, **inputs(bam))                     # the cooked pack and the plan read the same blocks
    with hostlib.plan_ingest(**inputs(bam)) as plan:
        assert plan.reason is None


@pytest.mark.parametrize("which", ["first", "middle", "last"])
@pytest.mark.parametrize("kind", ["trailer", "stored_payload"])
@pytest.mark.parametrize("threads", [1, 3])
def test_one_flipped_bit_fails_the_pack_with_crc32(tmp_path, stored_bam, kind, which, threads):
    bam, raw, blocks = stored_bam
    b = crc_util.first_middle_last(blocks)[which]
    bad = bytearray(raw)
    (crc_util.flip_trailer if kind == "trailer" else crc_util.flip_stored_payload)(bad, b)
    assert sum(bin(x ^ y).count("1") for x, y in zip(bad, raw)) == 1
    p = write_copy(tmp_path, "bad.bam", bam, bad)
    for raw_pack_too in (False, True):
        with pytest.raises(hostlib.HostError) as ei:
            hostlib.pack_files(raw=raw_pack_too, threads=threads, **inputs(p))
        msg = str(ei.value)
        assert "CRC32" in msg and p in msg and ("file offset %d:" % b["start"]) in msg, msg
    if which == "first":                                  # the plan inflates the header's blocks itself
        with pytest.raises(hostlib.HostError, match="CRC32"):
            hostlib.plan_ingest(**inputs(p))


def test_the_eof_block_is_checked_too(tmp_path, stored_bam):
    bam, raw, blocks = stored_bam
    bad = bytearray(raw)
    crc_util.flip_trailer(bad, blocks[-1])                # an empty block's CRC32 is 0
    p = write_copy(tmp_path, "bad_eof.bam", bam, bad)
    with pytest.raises(hostlib.HostError, match="CRC32"):
        hostlib.pack_files(threads=2, **inputs(p))


def seq_byte_positions(raw, blocks, block_size=20000):
    """(block, offset inside its inflated bytes) of the first sequence byte of every BAM record."""
    import zlib
    stream = b"".join(zlib.decompress(raw[b["coff"]:b["coff"] + b["clen"]], -15) for b in blocks)
    l_text = struct.unpack_from("<i", stream, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", stream, p)[0]
    out = []
    while p + 36 <= len(stream):
        bs = struct.unpack_from("<i", stream, p)[0]
        l_rn, n_cig, l_seq = stream[p + 12], struct.unpack_from("<H", stream, p + 16)[0], struct.unpack_from("<i", stream, p + 20)[0]
        u = p + 36 + l_rn + 4 * n_cig
        if l_seq > 4:
            out.append((u // block_size, u % block_size))
        p += 4 + bs
    return out


@pytest.mark.parametrize("which", ["first", "middle", "last"])
def test_the_damage_was_silent_without_the_check(tmp_path, stored_bam, which):
    """A bit of a read's bases, flipped in a stored block: with the block's own trailer the pack fails (CRC32); with a trailer that
    matches the damaged bytes — all a reader that never looks at the CRC32 can tell — the pack succeeds and carries the wrong base."""
    bam, raw, blocks = stored_bam
    b = crc_util.first_middle_last(blocks)[which]
    want, _ = raw_pack(bam)
    silent = 0
    for blk, at in [t for t in seq_byte_positions(raw, blocks) if t[0] == b["index"]][:12]:
        bad = bytearray(raw)
        crc_util.flip_stored_payload(bad, b, at)
        with pytest.raises(hostlib.HostError, match="CRC32"):
            raw_pack(write_copy(tmp_path, "bad.bam", bam, bad))
        crc_util.refresh_trailer(bad, b)
        got, _ = raw_pack(write_copy(tmp_path, "silent.bam", bam, bad))
        silent += not same_raw(got, want)
    assert silent > 0
