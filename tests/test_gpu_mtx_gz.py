"""vtx_write_mtx_gz: the Matrix-Market text deflated on the device (mtx_deflate_kernel / mtx_gz_compact_kernel, vartrix_amd/csrc/
vtx_deflate.hip; lane and wavefront logic vtx_deflate_core.h) — the reference writes plain text (src/main.rs:381-389), the readers of
a 10x matrix directory take matrix.mtx.gz.  Decompressed, the file must be vtx_write_mtx's (vtx_write_mtx_f64's) byte for byte, in
every scoring mode, over several chunks and several passes of the slab loop; compressed, it must be byte for byte what the HOST build
of the same encoder makes of the same text (tests/deflatecore/: a dependence on lane timing would show here); and the command line's
--gzip writes it at exactly the paths given, from the device or from the host formatter (vtxh_write_mtx_gz).  The encoder's edge
cases are the CPU suite's (tests/test_deflate_core.py, same source)."""
import gzip
import math
import os
import subprocess

import numpy as np
import pytest

import deflate_util as DU
from vartrix_amd import abi, hostlib, lib, synth
from vartrix_amd.abi import LOCUS_DTYPE, RECORD_DTYPE, PackedBatch, default_config

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def text_spec():
    """The batch of tests/test_gpu_ingest.py::test_matrix_market_text_from_the_device."""
    return synth.SynthSpec(n_loci=700, n_barcodes=900, reads_per_locus=40, indel_frac=0.2, use_umi=True, seed=5)


def chunks_spec():
    """64 loci x 256 barcodes with reads for nearly every pair: about 16 k triplets, 150 KB of text, three chunks."""
    return synth.SynthSpec(n_loci=64, n_barcodes=256, reads_per_locus=1024, seed=7)


@pytest.fixture(scope="module")
def text_batch():
    return synth.make_batch(text_spec())


@pytest.fixture(scope="module")
def chunks_batch():
    return synth.make_batch(chunks_spec())


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def plain_and_gz(ctx, tmp_path, spec, which, real, tag=""):
    """(plain text, gz file bytes) of one context's last run; sum and text_bytes checked against the plain call."""
    p, q = str(tmp_path / ("m%s%d.mtx" % (tag, which))), str(tmp_path / ("m%s%d.mtx.gz" % (tag, which)))
    s = ctx.write_mtx(p, spec.n_loci, spec.n_barcodes, which, real=real)
    t, nbytes = ctx.write_mtx_gz(q, spec.n_loci, spec.n_barcodes, which, real=real)
    text, z = open(p, "rb").read(), open(q, "rb").read()
    assert gzip.decompress(z) == text
    assert nbytes == len(text) and same(s, t), (nbytes, len(text), s, t)
    return text, z


@pytest.mark.parametrize("mode", ["consensus", "coverage", "alt_frac"])
def test_decompressed_bytes_equal_the_plain_file(tmp_path, text_batch, mode):
    spec = text_spec()
    with lib.Context(default_config(scoring_mode=mode, use_umi=1, n_barcodes=spec.n_barcodes)) as ctx:
        ctx.submit(text_batch)
        ctx.run()
        for which in ((0, 1) if mode == "coverage" else (0,)):
            text, z = plain_and_gz(ctx, tmp_path, spec, which, real=mode == "alt_frac")
            assert text.count(b"\n") > 5000
            DU.check_bgzf(z, DU.cut(text))
        if mode == "alt_frac":      # the decline rule of vtx_write_mtx: fractions without `real` are refused and nothing is left at the path
            q = str(tmp_path / "declined.mtx.gz")
            with pytest.raises(lib.VtxError) as e:
                ctx.write_mtx_gz(q, spec.n_loci, spec.n_barcodes, 0, real=False)
            assert e.value.status == abi.VTX_E_UNSUPPORTED and not os.path.exists(q)


def test_several_chunks_and_the_host_build_of_the_encoder(tmp_path, chunks_batch):
    """Three chunks; and the device's file equals, byte for byte, what the host build of vtx_deflate_core.h makes of the same text with
    the same chunking."""
    spec = chunks_spec()
    with lib.Context(default_config(scoring_mode="coverage", n_barcodes=spec.n_barcodes)) as ctx:
        ctx.submit(chunks_batch)
        ctx.run()
        text, z = plain_and_gz(ctx, tmp_path, spec, 0, real=False)
        _, nbytes = ctx.write_mtx_gz(str(tmp_path / "again.gz"), spec.n_loci, spec.n_barcodes, 0)
    assert len(text) > 2 * DU.CHUNK and text.count(b"\n") > 14000
    kinds = DU.check_bgzf(z, DU.cut(text))
    assert len(kinds) >= 3 and set(kinds) == {2}
    assert open(str(tmp_path / "again.gz"), "rb").read() == z                      # run to run
    assert DU.encode_file(text, str(tmp_path)) == z                                # device == host build


def test_alt_frac_text_equals_the_host_build_of_the_encoder(tmp_path, text_batch):
    spec = text_spec()
    with lib.Context(default_config(scoring_mode="alt_frac", use_umi=1, n_barcodes=spec.n_barcodes)) as ctx:
        ctx.submit(text_batch)
        ctx.run()
        text, z = plain_and_gz(ctx, tmp_path, spec, 0, real=True)
    assert DU.encode_file(text, str(tmp_path)) == z


def test_slab_loop_with_short_last_chunks(tmp_path, text_batch):
    """libvtx_dev.so with VTX_MTX_SLAB=4099: several passes, the chunking restarts in each, every pass ends with a short chunk; the
    header lines are in front of the first pass's text."""
    spec = text_spec()
    cfg = default_config(scoring_mode="alt_frac", use_umi=1, n_barcodes=spec.n_barcodes)
    old = os.environ.get("VTX_MTX_SLAB")
    os.environ["VTX_MTX_SLAB"] = "4099"                  # (read by libvtx_dev.so at every call)
    try:
        with lib.Context(cfg, variant="dev") as ctx:
            ctx.submit(text_batch)
            ctx.run()
            nnz = len(ctx.fetch_coo()["row"])
            text, z = plain_and_gz(ctx, tmp_path, spec, 0, real=True, tag="slab")
    finally:
        if old is None:
            del os.environ["VTX_MTX_SLAB"]
        else:
            os.environ["VTX_MTX_SLAB"] = old
    assert nnz > 2 * 4099
    ms = DU.members(z)
    sizes = [len(gzip.decompress(m)) for m in ms]
    assert sum(sizes) == len(text) and sum(1 for n in sizes if n < DU.CHUNK) >= (nnz + 4098) // 4099      # a short chunk per pass
    # the first pass: header lines + 4099 lines
    lines = text.split(b"\n")
    first = len(b"\n".join(lines[:3 + 4099])) + 1
    k, acc = 0, 0
    while acc < first:
        acc += sizes[k]
        k += 1
    assert acc == first, "the first pass's chunks end where its text ends"
    with lib.Context(cfg) as ctx:                        # the production library, one pass: the same text
        ctx.submit(text_batch)
        ctx.run()
        text1, _ = plain_and_gz(ctx, tmp_path, spec, 0, real=True, tag="one")
    assert text1 == text


def test_an_empty_matrix_is_a_valid_file_with_the_header_only(tmp_path):
    empty = PackedBatch(np.zeros(0, LOCUS_DTYPE), np.zeros(0, RECORD_DTYPE), np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    with lib.Context(default_config(scoring_mode="consensus", n_barcodes=34)) as ctx:
        ctx.submit(empty)
        ctx.run()
        q = str(tmp_path / "empty.mtx.gz")
        s, nbytes = ctx.write_mtx_gz(q, 12, 34)
    z = open(q, "rb").read()
    text = b"%%MatrixMarket matrix coordinate real general\n% written by sprs\n12 34 0\n"
    assert gzip.decompress(z) == text and nbytes == len(text) and s == 0.0
    DU.check_bgzf(z, [text])
    assert DU.encode_file(text, str(tmp_path)) == z


def test_an_unwritable_path_is_an_error_and_leaves_no_file(tmp_path, text_batch):
    spec = text_spec()
    with lib.Context(default_config(scoring_mode="consensus", use_umi=1, n_barcodes=spec.n_barcodes)) as ctx:
        ctx.submit(text_batch)
        ctx.run()
        q = str(tmp_path / "no_such_dir" / "m.mtx.gz")
        with pytest.raises(lib.VtxError):
            ctx.write_mtx_gz(q, spec.n_loci, spec.n_barcodes)
        assert not os.path.exists(q) and not os.path.exists(os.path.dirname(q))
        t, nbytes = ctx.write_mtx_gz(str(tmp_path / "after.mtx.gz"), spec.n_loci, spec.n_barcodes)      # the context still works
        assert nbytes == len(gzip.decompress(open(str(tmp_path / "after.mtx.gz"), "rb").read()))


def test_a_prefetch_is_waited_for_and_dropped(tmp_path):
    """The encoder's slots take the buffer vtx_prefetch_file copies a BAM into.  vtx_write_mtx_gz therefore waits for a prefetch and
    drops it: a vtx_submit_bam of the same file afterwards uploads the bytes again (prefetch_ms 0) instead of inflating gzip members
    of matrix text, and gives the same triplets; a prefetch still in flight when the call starts does not reach the file."""
    inputs = dict(vcf=os.path.join(G, "test.vcf"), bam=os.path.join(G, "test.bam"), fasta=os.path.join(G, "test.fa"),
                  cell_barcodes=os.path.join(G, "barcodes.tsv"))
    files = [str(tmp_path / ("m%d.mtx.gz" % i)) for i in range(3)]
    with hostlib.plan_ingest(**inputs) as plan, lib.Context(default_config(n_barcodes=len(plan.barcodes))) as ctx:
        ctx.set_barcodes(plan.barcodes)
        n_rows, n_cols = plan.n_loci, len(plan.barcodes)

        def triplets():
            ctx.run()
            coo = ctx.fetch_coo()
            return coo["row"].tobytes(), coo["col"].tobytes(), coo["value"].tobytes()

        ctx.prefetch_file(inputs["bam"])
        st = ctx.submit_bam(plan.ingest, plan.n_loci)
        assert st.prefetch_ms > 0 and st.raw_records > 0               # the prefetched bytes were used and are still marked valid
        first = triplets()
        ctx.write_mtx_gz(files[0], n_rows, n_cols)
        st = ctx.submit_bam(plan.ingest, plan.n_loci)
        assert st.prefetch_ms == 0                                     # dropped: the file travelled again
        assert triplets() == first
        ctx.prefetch_file(inputs["bam"])                               # in flight (or just landed) when the call starts
        ctx.write_mtx_gz(files[1], n_rows, n_cols)
        st = ctx.submit_bam(plan.ingest, plan.n_loci)
        assert st.prefetch_ms == 0
        assert triplets() == first
        ctx.write_mtx_gz(files[2], n_rows, n_cols)
    z = [open(f, "rb").read() for f in files]
    assert z[0] == z[1] == z[2] and len(first[0]) > 0
    assert gzip.decompress(z[0]).count(b"\n") == 3 + len(first[0]) // 4


# ---- the command line ----
@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(hostlib.CLI_PATH) and os.path.exists(hostlib.LIB_PATH) and os.path.exists(lib.LIB_PATH)):
        import __graft_entry__
        __graft_entry__.build()


def cli(args, cwd):
    base = ["-v", os.path.join(G, "test.vcf"), "-b", os.path.join(G, "test.bam"), "-f", os.path.join(G, "test.fa"), "-c", os.path.join(G, "barcodes.tsv")]
    r = subprocess.run([hostlib.CLI_PATH] + base + args + ["--log-level", "info"], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def golden(name):
    return open(os.path.join(G, name), "rb").read()


HOST_FLAGS = ["--ingest", "host", "--gather", "library"]       # the triplets are fetched: the host formatter writes the matrix


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("mode,want", [("consensus", "test_consensus.mtx"), ("alt_frac", "test_frac.mtx")])
def test_cli_gzip_values(tmp_path, built, mode, want, host):
    """`vartrix --gzip` on the reference's fixtures: -o is a gzip file at exactly the path given; decompressed it is test_consensus.mtx /
    test_frac.mtx.  From the device the log names vtx_write_mtx_gz; with --ingest host --gather library the host formatter writes the
    same decompressed bytes and the log names vtxh_write_mtx_gz."""
    says, not_says = ("(vtxh_write_mtx_gz)", "(vtx_write_mtx_gz)") if host else ("(vtx_write_mtx_gz)", "host formatter")
    out = str(tmp_path / (mode + ".out"))              # no .gz in the name: nothing is appended to it
    r = cli(["-o", out, "-s", mode, "--gzip"] + (HOST_FLAGS if host else []), tmp_path)
    assert says in r.stderr and not_says not in r.stderr, r.stderr
    z = open(out, "rb").read()
    assert gzip.decompress(z) == golden(want) and not os.path.exists(out + ".gz")
    DU.check_bgzf(z, DU.cut(golden(want)))


def test_cli_gzip_coverage_writes_both_matrices(tmp_path, built):
    """Coverage mode: --out-matrix and --ref-matrix are both compressed; decompressed they are what the same command writes without
    --gzip, and the reference's matrices."""
    from oracle import refpipe
    out, ref = str(tmp_path / "cov.mtx.gz"), str(tmp_path / "cov_ref.mtx.gz")
    pout, pref = str(tmp_path / "cov.mtx"), str(tmp_path / "cov_ref.mtx")
    r = cli(["-o", out, "-s", "coverage", "--ref-matrix", ref, "--gzip"], tmp_path)
    assert "(vtx_write_mtx_gz)" in r.stderr and "host formatter" not in r.stderr, r.stderr
    cli(["-o", pout, "-s", "coverage", "--ref-matrix", pref], tmp_path)
    unz = str(tmp_path / "unz.mtx")
    for zpath, ppath, want in ((out, pout, "test_coverage.mtx"), (ref, pref, "test_coverage_ref.mtx")):
        text = gzip.decompress(open(zpath, "rb").read())
        assert text == open(ppath, "rb").read()
        open(unz, "wb").write(text)
        assert refpipe.read_mtx(unz) == refpipe.read_mtx(os.path.join(G, want))


def test_cli_variants_and_barcodes_stay_text(tmp_path, built):
    out, ov, ob = str(tmp_path / "o.mtx.gz"), str(tmp_path / "variants.txt"), str(tmp_path / "barcodes.txt")
    cli(["-o", out, "--gzip", "--out-variants", ov, "--out-barcodes", ob], tmp_path)
    assert open(out, "rb").read()[:2] == b"\x1f\x8b"
    assert open(ob, "rb").read().split() == golden("barcodes.tsv").split() and open(ov, "rb").read()[:2] != b"\x1f\x8b" and open(ov).read().count("\n") > 0


def test_cli_help_lists_gzip(built):
    r = subprocess.run([hostlib.CLI_PATH, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--gzip" in r.stderr
