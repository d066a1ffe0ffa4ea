"""The device ingest verifies the CRC32 of every BGZF block (bgzf_crc32_kernel, vtx_crc32_core.h; htslib's check in bgzf_read_block,
in the reference the Err of `let rec = _rec?`, src/main.rs:829-830).

The kernel against zlib.crc32 on the size / alignment grid of tests/test_crc32_core.py and on every block of the reference's test.bam;
the ingest of undamaged files unchanged to the byte; ONE flipped bit — in a trailer's CRC32 field, or in the payload of a stored block,
which still inflates — in the first, a middle or the last block of what travels is declined (VTX_E_UNSUPPORTED, "CRC32"), directly,
through vtx_prefetch_file and per segment of a segmented plan; and the command line fails the way it fails for a block that does not
inflate.  Every case here is an error return of the library: nothing faults."""
import ctypes as C
import os
import random
import subprocess
import sys
import zlib

import numpy as np
import pytest

from tests import crc_util
from vartrix_amd import abi, hostlib, lib
from vartrix_amd.abi import default_config

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
import segments_util as su  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def built():
    if not (os.path.exists(hostlib.CLI_PATH) and os.path.exists(hostlib.LIB_PATH) and os.path.exists(lib.LIB_PATH)):
        import __graft_entry__
        __graft_entry__.build()


@pytest.fixture(scope="module")
def ctx():
    with lib.Context(default_config(n_barcodes=4)) as c:
        yield c


def corpus(rng, kind, n):
    if kind == "random":
        return rng.randbytes(n)
    if kind == "acgt":
        return (bytes(rng.choice(b"ACGT") for _ in range(min(n, 1999))) * (n // 1999 + 1))[:n]
    return (b"\x00" if kind == "zero" else b"\xff") * n


@pytest.mark.parametrize("kind", ["random", "acgt", "zero", "ff"])
def test_kernel_equals_zlib_on_the_size_and_alignment_grid(ctx, kind):
    """Every length 0..300, lengths up to 65536 with 65280 and 65536 and the row boundaries of the lane grid, each range at a random
    start misalignment 0..15 (the gap in front of it is a range of its own): ONE launch, every range equals zlib.crc32."""
    rng = random.Random(len(kind))
    lengths = list(range(301)) + [65280, 65536, 65535, 1023, 1024, 1025, 2047, 2049, 1008, 1040] + [rng.randrange(301, 65537) for _ in range(40)]
    rng.shuffle(lengths)
    parts, offsets = [], [0]
    for n in lengths:
        for m in (rng.randrange(16), n):
            parts.append(corpus(rng, kind, m))
            offsets.append(offsets[-1] + m)
    data = b"".join(parts)
    got = ctx.debug_crc32(data, offsets)
    want = np.array([zlib.crc32(p) for p in parts], np.uint32)
    assert got.shape == want.shape and np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert ctx.crc_ms() > 0.0


def test_kernel_on_every_block_of_the_reference_bam(ctx):
    raw = open(os.path.join(G, "test.bam"), "rb").read()
    blocks = crc_util.blocks_of(raw)
    pieces = [zlib.decompress(raw[b["coff"]:b["coff"] + b["clen"]], -15) for b in blocks]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in pieces])])
    got = ctx.debug_crc32(b"".join(pieces), offsets)
    trailers = [int.from_bytes(raw[b["coff"] + b["clen"]:b["coff"] + b["clen"] + 4], "little") for b in blocks]
    assert len(blocks) > 5 and blocks[-1]["isize"] == 0 and trailers[-1] == 0
    assert got.tolist() == trailers == [zlib.crc32(p) for p in pieces]


def test_debug_crc32_refuses_bad_ranges(ctx):
    for offsets in ([0, 65537], [0, 10, 5], [0, 200]):
        with pytest.raises(lib.VtxError) as ei:
            ctx.debug_crc32(b"x" * 100 if offsets[-1] == 200 else b"x" * 70000, offsets)
        assert ei.value.status == abi.VTX_E_INVAL
    assert ctx.debug_crc32(b"", [0]).size == 0


def dna_inputs(bam):
    return dict(vcf=os.path.join(G, "test_dna.vcf"), bam=bam, fasta=os.path.join(G, "test_dna.fa"),
                cell_barcodes=os.path.join(G, "dna_barcodes.tsv"))


def author_stored(tmp_path, **kw):
    from tests.test_host import make_dna_bam
    with crc_util.stored_blocks():
        return make_dna_bam(tmp_path, **kw)


def test_undamaged_files_ingest_as_before(tmp_path):
    """The reference BAM, an authored BAM and the same records in stored blocks: everything the device builds is the host pack's, byte
    for byte (tests/test_gpu_ingest.py's comparison through the vtx_debug_ingest arrays), with the check in the pipeline."""
    from tests.test_gpu_ingest import ingest_and_compare, ref_inputs
    from tests.test_host import make_dna_bam
    st = ingest_and_compare(ref_inputs())
    assert st.bam_records > 500
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    a = ingest_and_compare(dna_inputs(make_dna_bam(tmp_path / "a", seed=3, n_reads=2500)), pack_kw=dict(use_umi=True))
    b = ingest_and_compare(dna_inputs(author_stored(tmp_path / "b", seed=3, n_reads=2500)), pack_kw=dict(use_umi=True))
    assert a.raw_records == b.raw_records > 0 and a.inflated_bytes == b.inflated_bytes


def damaged(raw, b, kind):
    bad = bytearray(raw)
    (crc_util.flip_trailer if kind == "trailer" else crc_util.flip_stored_payload)(bad, b)
    return np.frombuffer(bytes(bad), np.uint8).copy()


def expect_crc_decline(call, block_index):
    with pytest.raises(lib.VtxError) as ei:
        call()
    assert ei.value.status == abi.VTX_E_UNSUPPORTED, ei.value
    assert "CRC32" in str(ei.value) and ("block %d:" % block_index) in str(ei.value), ei.value


@pytest.mark.parametrize("which", ["first", "middle", "last"])
@pytest.mark.parametrize("kind", ["trailer", "stored_payload"])
@pytest.mark.parametrize("prefetch", [False, True])
def test_one_flipped_bit_is_declined(tmp_path, kind, which, prefetch):
    """The plan's blocks are the stretch that travels; the LAST of them has its trailer in the 8 bytes that travel behind the stretch.
    prefetch: the damaged file's bytes come through vtx_prefetch_file (and are used: prefetch_ms says so)."""
    bam = author_stored(tmp_path, seed=7, n_reads=1500)
    raw = open(bam, "rb").read()
    by_coff = {b["coff"]: b for b in crc_util.blocks_of(raw)}
    with hostlib.plan_ingest(**dna_inputs(bam)) as plan:
        assert plan.reason is None and plan.kind == "contiguous"
        pb = plan.arrays()["blocks"]
        data_idx = [i for i in range(len(pb)) if pb["isize"][i]]
        assert len(data_idx) >= 4
        i = {"first": data_idx[0], "middle": data_idx[len(data_idx) // 2], "last": data_idx[-1]}[which]
        bad = damaged(raw, by_coff[int(pb["coff"][i])], kind)
        bad_path = str(tmp_path / "bad.bam")
        bad.tofile(bad_path)
        g = abi.VtxBamIngest.from_buffer_copy(plan.ingest)
        g.file = bad.ctypes.data
        with lib.Context(default_config(n_barcodes=len(plan.barcodes))) as ctx:
            ctx.set_barcodes(plan.barcodes)
            if prefetch:
                ctx.prefetch_file(bad_path)
            expect_crc_decline(lambda: ctx.submit_bam(g, plan.n_loci), i)
            # the context is fine afterwards, and the undamaged bytes are taken
            if prefetch:
                ctx.prefetch_file(bam)
            st = ctx.submit_bam(plan.ingest, plan.n_loci)
            assert st.raw_records > 0 and (st.prefetch_ms > 0) == prefetch
            assert ctx.crc_ms() > 0.0


def test_a_block_without_room_for_its_trailer_is_declined(tmp_path):
    """file_bytes cut inside the last planned block's trailer: not a BGZF block — VTX_E_UNSUPPORTED before anything travels."""
    bam = author_stored(tmp_path, seed=7, n_reads=600)
    with hostlib.plan_ingest(**dna_inputs(bam)) as plan:
        pb = plan.arrays()["blocks"]
        g = abi.VtxBamIngest.from_buffer_copy(plan.ingest)
        g.file_bytes = int(pb["coff"][-1]) + int(pb["clen"][-1]) + 7
        with lib.Context(default_config(n_barcodes=len(plan.barcodes))) as ctx:
            ctx.set_barcodes(plan.barcodes)
            with pytest.raises(lib.VtxError) as ei:
                ctx.submit_bam(g, plan.n_loci)
            assert ei.value.status == abi.VTX_E_UNSUPPORTED and "trailer" in str(ei.value)
            assert ctx.submit_bam(plan.ingest, plan.n_loci).raw_records > 0


@pytest.mark.parametrize("kind", ["trailer", "stored_payload"])
def test_the_last_block_of_a_segment_is_checked(tmp_path, monkeypatch, kind):
    """A segmented plan (sparse loci): every segment's bytes travel with the trailer of its last block.  Damage in the last block of
    the first, a middle and the last segment is declined; the plan itself ingests as the host packs."""
    hostlib.use_variant("dev")                             # the planner's threshold knob: developer build of the host library only
    try:
        monkeypatch.setenv("VTXH_SPARSE_KIB", su.SPARSE_KIB)
        with crc_util.stored_blocks():
            inputs = su.author(tmp_path, block=4000)
        raw = open(inputs["bam"], "rb").read()
        by_coff = {b["coff"]: b for b in crc_util.blocks_of(raw)}
        with hostlib.plan_ingest(**inputs) as plan:
            assert plan.reason is None and plan.kind == "segmented"
            a = plan.arrays()
            segs = a["segments"]
            assert len(segs) >= 3
            with lib.Context(default_config(n_barcodes=len(plan.barcodes))) as ctx:
                ctx.set_barcodes(plan.barcodes)
                for k in (0, len(segs) // 2, len(segs) - 1):
                    i = int(segs["block_end"][k]) - 1
                    assert a["blocks"]["isize"][i] > 0
                    bad = damaged(raw, by_coff[int(a["blocks"]["coff"][i])], kind)
                    sg = abi.VtxBamSegments.from_buffer_copy(plan.segments)
                    sg.base.file = bad.ctypes.data
                    expect_crc_decline(lambda: ctx.submit_bam_segments(sg, plan.n_loci), i)
                st = ctx.submit_bam_segments(plan.segments, plan.n_loci)
                assert st.raw_records > 100 and int(st.compressed_bytes) < a["contiguous_compressed"]
        from tests.test_gpu_ingest_segments import segmented_ingest_and_compare
        segmented_ingest_and_compare(inputs, pack_kw=dict(use_umi=True))
    finally:
        hostlib.use_variant("dev" if os.environ.get("VTX_LIB_VARIANT") == "dev" else "")


def test_command_line_with_a_crc_damaged_bam(tmp_path):
    """One flipped payload bit in a middle block (stored: it inflates): --ingest device fails with CRC32 and writes nothing; the default
    --ingest auto says that the device declined, packs on the host and fails there; --ingest host fails the same way.  The undamaged
    file gives the same bytes whichever reader reads it, and whether its blocks are stored or deflated."""
    from tests.test_host import make_dna_bam
    (tmp_path / "d").mkdir()
    bam = author_stored(tmp_path, seed=6, n_reads=1200)
    deflated = make_dna_bam(tmp_path / "d", seed=6, n_reads=1200)
    raw = open(bam, "rb").read()
    b = crc_util.first_middle_last(crc_util.blocks_of(raw))["middle"]
    bad = str(tmp_path / "bad.bam")
    damaged(raw, b, "stored_payload").tofile(bad)
    open(bad + ".bai", "wb").write(open(bam + ".bai", "rb").read())
    i = dna_inputs(bam)
    base = ["-v", i["vcf"], "-f", i["fasta"], "-c", i["cell_barcodes"], "--log-level", "info", "-s", "coverage"]

    def cli(path, tag, flags):
        return subprocess.run([hostlib.CLI_PATH] + base + ["-b", path, "-o", str(tmp_path / (tag + ".mtx")), "--ref-matrix", str(tmp_path / (tag + "_ref.mtx"))] + flags,
                              cwd=tmp_path, capture_output=True, text=True, timeout=300)
    outs = []
    for tag, path, flags in (("dev", bam, ["--ingest", "device"]), ("auto", bam, []), ("host", bam, ["--ingest", "host"]), ("defl", deflated, ["--ingest", "device"])):
        r = cli(path, tag, flags)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("ingest on the device" in r.stderr) == (tag != "host")
        outs.append((open(tmp_path / (tag + ".mtx")).read(), open(tmp_path / (tag + "_ref.mtx")).read()))
    assert outs[0] == outs[1] == outs[2] == outs[3] and len(outs[0][0]) > 500
    for tag, flags in (("bad_dev", ["--ingest", "device"]), ("bad_auto", []), ("bad_host", ["--ingest", "host"])):
        r = cli(bad, tag, flags)
        text = r.stdout + r.stderr
        assert r.returncode != 0 and "CRC32" in text and "Vartrix error." in r.stdout, text
        assert not os.path.exists(tmp_path / (tag + ".mtx")) and not os.path.exists(tmp_path / (tag + "_ref.mtx"))
        if tag == "bad_auto":
            assert "the device declined" in r.stderr and "packing on the host" in r.stderr and ("file offset %d:" % b["start"]) in r.stdout, text
        if tag == "bad_host":
            assert ("file offset %d:" % b["start"]) in r.stdout, text
