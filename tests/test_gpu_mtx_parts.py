"""A matrix written from the device in PARTS (vtx_mtx_part / vtx_mtx_join): streamed ranges of loci and the batches of one pack run one
after the other, and after each vtx_run the context turns that run's triplets into a finished piece of the Matrix-Market file — the
lines alone, or their BGZF members deflated on the device — that is plain host bytes when the call returns; nothing stays on the device
between the runs.  The reference writes the whole matrix at the end (sprs::io::write_matrix_market, src/main.rs:381-389); rows ascend
from run to run, so the joined parts must be that file byte for byte: equal to vtx_write_mtx of the whole batch on a fresh context, in
every scoring mode, however the loci are cut; compressed, each part must be what the HOST build of the encoder makes of the part's
text; and the command line must take this path — and say so — for every streamed or multi-batch run on one device, with the host
formatter only for the one run whose part declined.  The host-made parts and the join itself: tests/test_mtx_parts_host.py."""
import ctypes as C
import gzip
import math
import os
import re
import subprocess

import pytest

import deflate_util as DU
from vartrix_amd import abi, hostlib, lib, shard, synth
from vartrix_amd.abi import default_config

from tests.test_gpu_mtx_gz import chunks_spec, text_spec

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not (os.path.exists(hostlib.CLI_PATH) and os.path.exists(hostlib.cli_path("dev")) and os.path.exists(hostlib.LIB_PATH) and os.path.exists(lib.LIB_PATH)):
        import __graft_entry__
        __graft_entry__.build()


@pytest.fixture(scope="module")
def text_batch():
    return synth.make_batch(text_spec())


@pytest.fixture(scope="module")
def chunks_batch():
    return synth.make_batch(chunks_spec())


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def sum_agrees(got, want, real):
    """Integral values: exactly.  alt_frac's fractions are added on the device in no fixed order (vtx_write_mtx_f64's contract): a part
    holds at most 25 000 values in [0, 1], every addition rounds by at most 2^-53 of a partial sum below 25 000 — 1e-9 relative is far
    outside that and far inside any wrong sum (one value more or less moves it by 1 / 3 or more).  NaN must be NaN."""
    return same(got, want) or (real and not math.isnan(got) and not math.isnan(want) and abs(got - want) <= 1e-9 * max(1.0, abs(want)))


def header(spec, nnz):
    return b"%%%%MatrixMarket matrix coordinate real general\n%% written by sprs\n%d %d %d\n" % (spec.n_loci, spec.n_barcodes, nnz)


def pieces_of(batch, n):
    """n locus ranges in row order; five: four ranges of about equal record counts and, in the middle, a range without a locus (a run
    that yields no triplet)."""
    if n == 5:
        r = shard.partition_loci(batch, 4)
        return r[:2] + [(r[2][0], r[2][0])] + r[2:]
    return shard.partition_loci(batch, n)


MODES = {"consensus": ((0,), False), "coverage": ((0, 1), False), "alt_frac": ((0,), True)}      # mode -> (which, real)


def whole_files(tmp_path, batch, spec, mode):
    """{which: vtx_write_mtx's (alt_frac: vtx_write_mtx_f64's) file of the whole batch on a fresh context}"""
    whichs, real = MODES[mode]
    out = {}
    with lib.Context(default_config(scoring_mode=mode, use_umi=1, n_barcodes=spec.n_barcodes)) as ctx:
        ctx.submit(batch)
        ctx.run()
        for w in whichs:
            p = str(tmp_path / ("whole%d.mtx" % w))
            ctx.write_mtx(p, spec.n_loci, spec.n_barcodes, w, real=real)
            out[w] = open(p, "rb").read()
    return out


def run_pieces(ctx, batch, ranges, whichs, real, gz):
    """The pieces in sequence on ONE context, the part(s) taken after each run and checked against that run's fetch_coo.
    -> {which: [MtxPart]}"""
    parts = {w: [] for w in whichs}
    for lo, hi in ranges:
        ctx.submit(batch.slice_loci(lo, hi))
        ctx.run()
        coo = ctx.fetch_coo()
        for w in whichs:
            p = ctx.mtx_part(w, real=real, gz=gz)
            v = coo["ref_value" if w else "value"]
            assert p.nnz == len(coo["row"]) and p.gz == gz
            assert sum_agrees(p.sum, float(v.sum()), real), (p.sum, float(v.sum()))           # (numpy's sum of an array with a NaN is NaN)
            assert (p.nnz > 0) == bool(p.bytes)
            if not gz:
                assert p.text_bytes == len(p.bytes) and p.bytes.count(b"\n") == p.nnz
            parts[w].append(p)
    return parts


@pytest.mark.parametrize("n_pieces", [1, 2, 5])
@pytest.mark.parametrize("mode", ["consensus", "coverage", "alt_frac"])
def test_parts_joined_equal_the_whole_file(tmp_path, text_batch, mode, n_pieces):
    """Every piece in sequence on one context, the part taken after each run (nnz and sum checked against that run's fetch_coo, see
    sum_agrees); the join is vtx_write_mtx of the whole batch on a fresh context, byte for byte."""
    spec = text_spec()
    whichs, real = MODES[mode]
    want = whole_files(tmp_path, text_batch, spec, mode)
    ranges = pieces_of(text_batch, n_pieces)
    assert len(ranges) == n_pieces
    with lib.Context(default_config(scoring_mode=mode, use_umi=1, n_barcodes=spec.n_barcodes)) as ctx:
        parts = run_pieces(ctx, text_batch, ranges, whichs, real, gz=False)
    if n_pieces == 5:
        assert parts[0][2].nnz == 0 and parts[0][2].bytes == b""
    for w in whichs:
        out = str(tmp_path / ("joined%d.mtx" % w))
        nbytes = lib.mtx_join(out, spec.n_loci, spec.n_barcodes, parts[w])
        got = open(out, "rb").read()
        assert got == want[w] and nbytes == len(got)
        assert got.count(b"\n") > 5000


@pytest.mark.parametrize("n_pieces", [1, 2, 5])
@pytest.mark.parametrize("mode", ["consensus", "coverage", "alt_frac"])
def test_gz_parts_joined_decompress_to_the_whole_file(tmp_path, text_batch, mode, n_pieces):
    spec = text_spec()
    whichs, real = MODES[mode]
    want = whole_files(tmp_path, text_batch, spec, mode)
    ranges = pieces_of(text_batch, n_pieces)
    with lib.Context(default_config(scoring_mode=mode, use_umi=1, n_barcodes=spec.n_barcodes)) as ctx:
        parts = run_pieces(ctx, text_batch, ranges, whichs, real, gz=True)
    for w in whichs:
        out = str(tmp_path / ("joined%d.mtx.gz" % w))
        nbytes = lib.mtx_join(out, spec.n_loci, spec.n_barcodes, parts[w], gz=True)
        z = open(out, "rb").read()
        assert gzip.decompress(z) == want[w] and nbytes == len(want[w])
        # member by member: the header, then every non-empty part's text cut from the part's first byte
        nnz = sum(p.nnz for p in parts[w])
        body, chunks = want[w][len(header(spec, nnz)):], [header(spec, nnz)]
        assert want[w].startswith(chunks[0])
        at = 0
        for p in parts[w]:
            assert (p.text_bytes > 0) == (p.nnz > 0)
            if p.nnz:
                chunks += DU.cut(body[at:at + p.text_bytes])
                at += p.text_bytes
        assert at == len(body)
        DU.check_bgzf(z, chunks)


def test_gz_parts_equal_the_host_build_of_the_encoder_and_mix_with_host_parts(tmp_path, chunks_batch):
    """chunks_spec in two pieces: each part is several chunks, and its bytes are what the host build of vtx_deflate_core.h makes of the
    part's text (its end-of-file member taken off).  And a join of part 0 from the device with part 1 from the host formatter
    (vtxh_mtx_part on the fetched triplets: what the command line does for a part that declined) decompresses to the same text."""
    spec = chunks_spec()
    cfg = default_config(scoring_mode="coverage", n_barcodes=spec.n_barcodes)
    ranges = pieces_of(chunks_batch, 2)
    with lib.Context(cfg) as ctx:
        ctx.submit(chunks_batch)
        ctx.run()
        p = str(tmp_path / "whole.mtx")
        ctx.write_mtx(p, spec.n_loci, spec.n_barcodes, 0)
        want = open(p, "rb").read()
        gzp, txt, coos = [], [], []
        for lo, hi in ranges:
            ctx.submit(chunks_batch.slice_loci(lo, hi))
            ctx.run()
            gzp.append(ctx.mtx_part(0, gz=True))
            txt.append(ctx.mtx_part(0, gz=False))
            coos.append(ctx.fetch_coo())
    assert len(want) > 2 * DU.CHUNK
    n_members = 0
    for g, t in zip(gzp, txt):
        assert g.nnz == t.nnz > 0 and g.text_bytes == len(t.bytes)
        enc = DU.encode_file(t.bytes, str(tmp_path))
        assert enc.endswith(DU.EOF_BLOCK) and g.bytes == enc[:-len(DU.EOF_BLOCK)]                 # device == host build
        n_members += len(DU.cut(t.bytes))
    assert n_members >= 3 and max(len(t.bytes) for t in txt) > DU.CHUNK
    out = str(tmp_path / "joined.mtx.gz")
    lib.mtx_join(out, spec.n_loci, spec.n_barcodes, gzp, gz=True)
    assert gzip.decompress(open(out, "rb").read()) == want
    host1 = hostlib.mtx_part(coos[1]["row"], coos[1]["col"], coos[1]["value"], gz=True)
    assert host1.nnz == gzp[1].nnz and host1.text_bytes == gzp[1].text_bytes and same(host1.sum, gzp[1].sum)
    mixed = str(tmp_path / "mixed.mtx.gz")
    lib.mtx_join(mixed, spec.n_loci, spec.n_barcodes, [gzp[0], host1], gz=True)
    z = open(mixed, "rb").read()
    assert gzip.decompress(z) == want
    DU.members(z)
    # and the plain parts: the device's text is the host formatter's
    assert hostlib.mtx_part(coos[0]["row"], coos[0]["col"], coos[0]["value"]).bytes == txt[0].bytes


def test_slab_passes_leave_the_text_unchanged_and_end_their_members(tmp_path, text_batch):
    """libvtx_dev.so with VTX_MTX_SLAB=4099: a part is made in several passes; its text is the one-pass text, and with gz the chunking
    restarts with every pass — the members end where each pass's text ends."""
    spec = text_spec()
    cfg = default_config(scoring_mode="alt_frac", use_umi=1, n_barcodes=spec.n_barcodes)
    with lib.Context(cfg) as ctx:                        # the production library: one pass
        ctx.submit(text_batch)
        ctx.run()
        one = ctx.mtx_part(0, real=True)
    old = os.environ.get("VTX_MTX_SLAB")
    os.environ["VTX_MTX_SLAB"] = "4099"                  # (read by libvtx_dev.so at every call)
    try:
        with lib.Context(cfg, variant="dev") as ctx:
            ctx.submit(text_batch)
            ctx.run()
            text = ctx.mtx_part(0, real=True)
            z = ctx.mtx_part(0, real=True, gz=True)
    finally:
        if old is None:
            del os.environ["VTX_MTX_SLAB"]
        else:
            os.environ["VTX_MTX_SLAB"] = old
    assert one.nnz == text.nnz == z.nnz > 2 * 4099
    assert text.bytes == one.bytes and sum_agrees(text.sum, one.sum, True) and sum_agrees(z.sum, one.sum, True)
    lines = one.bytes.split(b"\n")[:-1]
    pass_texts = [b"".join(ln + b"\n" for ln in lines[k:k + 4099]) for k in range(0, len(lines), 4099)]
    chunks = [c for t in pass_texts for c in DU.cut(t)]
    assert len(pass_texts) == (one.nnz + 4098) // 4099 and z.text_bytes == len(one.bytes)
    DU.check_bgzf(z.bytes + DU.EOF_BLOCK, chunks)        # one member per chunk of each pass: a short one ends every pass


def test_declines_and_call_order(tmp_path, text_batch):
    spec = text_spec()
    cfg = default_config(scoring_mode="alt_frac", use_umi=1, n_barcodes=spec.n_barcodes)
    with lib.Context(cfg) as ctx:
        ctx.submit(text_batch)
        with pytest.raises(lib.VtxError) as e:           # before a completed run
            ctx.mtx_part(0, real=True)
        assert e.value.status == abi.VTX_E_STATE
        ctx.run()
        for gz in (0, 1):                                # fractions without `real`: declined, *out zeroed, the context usable
            st = abi.VtxMtxPart(None, 7, 7, 7, 7.0, 7, 7)
            assert ctx._L.vtx_mtx_part(ctx._h, 0, 0, gz, C.byref(st)) == abi.VTX_E_UNSUPPORTED
            assert (st.bytes, st.n_bytes, st.text_bytes, st.nnz, st.sum, st.gz, st.reserved) == (None, 0, 0, 0, 0.0, 0, 0)
            ctx._L.vtx_mtx_part_free(C.byref(st))        # nothing to do on a zeroed struct
            with pytest.raises(lib.VtxError) as e:
                ctx.mtx_part(0, real=False, gz=bool(gz))
            assert e.value.status == abi.VTX_E_UNSUPPORTED and "vtxh_mtx_part" in str(e.value)
        with pytest.raises(lib.VtxError) as e:
            ctx.mtx_part(2, real=True)
        assert e.value.status == abi.VTX_E_INVAL
        st = abi.VtxMtxPart(None, 7, 7, 7, 7.0, 7, 7)     # a bad argument zeroes *out too: vtx_mtx_part_free on it is safe
        assert ctx._L.vtx_mtx_part(ctx._h, 2, 1, 0, C.byref(st)) == abi.VTX_E_INVAL
        assert (st.bytes, st.n_bytes, st.text_bytes, st.nnz, st.sum, st.gz, st.reserved) == (None, 0, 0, 0, 0.0, 0, 0)
        ctx._L.vtx_mtx_part_free(C.byref(st))
        p = ctx.mtx_part(0, real=True)
        out = str(tmp_path / "after.mtx")
        ctx.write_mtx(out, spec.n_loci, spec.n_barcodes, 0, real=True)
        assert header(spec, p.nnz) + p.bytes == open(out, "rb").read()


def test_a_gz_part_waits_for_a_prefetch_and_drops_it(tmp_path):
    """The rule tests/test_gpu_mtx_gz.py::test_a_prefetch_is_waited_for_and_dropped pins for vtx_write_mtx_gz: the encoder's slots take
    the buffer vtx_prefetch_file copies a BAM into, so a gz part waits for a prefetch and drops it — a vtx_submit_bam of the same file
    afterwards uploads the bytes again (prefetch_ms 0) and gives the same triplets."""
    inputs = dict(vcf=os.path.join(G, "test.vcf"), bam=os.path.join(G, "test.bam"), fasta=os.path.join(G, "test.fa"),
                  cell_barcodes=os.path.join(G, "barcodes.tsv"))
    with hostlib.plan_ingest(**inputs) as plan, lib.Context(default_config(n_barcodes=len(plan.barcodes))) as ctx:
        ctx.set_barcodes(plan.barcodes)

        def triplets():
            ctx.run()
            coo = ctx.fetch_coo()
            return coo["row"].tobytes(), coo["col"].tobytes(), coo["value"].tobytes()

        ctx.prefetch_file(inputs["bam"])
        st = ctx.submit_bam(plan.ingest, plan.n_loci)
        assert st.prefetch_ms > 0 and st.raw_records > 0
        first = triplets()
        parts = [ctx.mtx_part(0, gz=True)]
        st = ctx.submit_bam(plan.ingest, plan.n_loci)
        assert st.prefetch_ms == 0                                     # dropped: the file travelled again
        assert triplets() == first
        ctx.prefetch_file(inputs["bam"])                               # in flight (or just landed) when the call starts
        parts.append(ctx.mtx_part(0, gz=True))
        st = ctx.submit_bam(plan.ingest, plan.n_loci)
        assert st.prefetch_ms == 0
        assert triplets() == first
        parts.append(ctx.mtx_part(0, gz=True))
        # a PLAIN part waits for a prefetch in flight too (it comes back through the copy workers the prefetch uses) but keeps its bytes
        ctx.prefetch_file(inputs["bam"])
        plain = ctx.mtx_part(0)
        st = ctx.submit_bam(plan.ingest, plan.n_loci)
        assert st.prefetch_ms > 0 and triplets() == first
        assert plain.bytes == gzip.decompress(parts[0].bytes)
    assert parts[0].bytes == parts[1].bytes == parts[2].bytes and parts[0].nnz == len(first[0]) // 4 > 0
    assert gzip.decompress(parts[0].bytes).count(b"\n") == parts[0].nnz


# ---- the command line ----
from tests.test_gpu_cli import PATHS      # noqa: E402  (the three ways the reads are prepared)

DNA = [os.path.join(G, n) for n in ("test_dna.vcf", "test_dna.fa", "dna_barcodes.tsv")]


@pytest.fixture(scope="module")
def dna_bam(tmp_path_factory):
    from tests.test_host import make_dna_bam
    return make_dna_bam(tmp_path_factory.mktemp("parts_bam"), seed=5, n_reads=2500)


def run_cli(exe, bam, args, cwd, env=None):
    vcfp, fap, bcp = DNA
    r = subprocess.run([exe, "-v", vcfp, "-b", bam, "-f", fap, "-c", bcp, "--threads", "4", "--log-level", "info"] + args, cwd=cwd,
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout + r.stderr


def outputs(tmp_path, name, mode, gz):
    sfx = ".mtx.gz" if gz else ".mtx"
    out, ref = str(tmp_path / (name + sfx)), str(tmp_path / (name + "_ref" + sfx))
    return out, ref, ["-o", out, "--ref-matrix", ref, "-s", mode, "--umi"] + (["--gzip"] if gz else [])


def matrices(out, ref, mode, gz):
    """The matrix files' bytes, decompressed (and checked as BGZF) with --gzip."""
    res = []
    for p in (out, ref) if mode == "coverage" else (out,):
        data = open(p, "rb").read()
        if gz:
            DU.members(data)
            data = gzip.decompress(data)
        res.append(data)
    assert mode == "coverage" or not os.path.exists(ref)
    return res


def counters(log):
    c = re.findall(r"Number of [^:]+: (\d+)", log)
    assert len(c) == 9
    return c


def n_parts_logged(log):
    m = re.search(r"Matrix written from the device in (\d+) parts \(vtx_mtx_part\)", log)
    assert m, log
    return int(m.group(1))


@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("mode", ["consensus", "alt_frac", "coverage"])
@pytest.mark.parametrize("prep", ["host", "device", "ingest"])
def test_cli_streamed_ranges_write_the_matrix_in_parts(tmp_path, dna_bam, prep, mode, gz):
    """--stream-loci 7 (7 ranges of test_dna.vcf's 46 records) and --stream-loci 1 (46) against the whole input at once: the same
    bytes (with --gzip: the same decompressed bytes, a valid BGZF file), the same nine counters, and the log names the parts — the host
    formatter is not on this path."""
    got = {}
    for name, sl in (("whole", "0"), ("ranges", "7"), ("single", "1")):
        out, ref, args = outputs(tmp_path, name, mode, gz)
        log = run_cli(hostlib.CLI_PATH, dna_bam, args + ["--stream-loci", sl] + PATHS[prep], tmp_path)
        got[name] = (matrices(out, ref, mode, gz), counters(log))
        assert "host formatter" not in log
        if name == "whole":                                   # one range, one batch, one device: unchanged
            assert re.search(r"Matrix written from the device \(vtx_write_mtx", log) and "vtx_mtx_part" not in log
        else:
            assert n_parts_logged(log) == {"ranges": 7, "single": 46}[name] and "formatted on the host" not in log
    assert got["whole"] == got["ranges"] == got["single"]
    assert got["whole"][0][0].count(b"\n") > 50


@pytest.mark.parametrize("prep", ["host", "device"])
def test_cli_batches_of_one_pack_write_the_matrix_in_parts(tmp_path, dna_bam, prep):
    """The hook of tests/test_gpu_cli.py::test_multi_batch_run_equals_single_batch (bin/vartrix_dev, VTXH_BATCH_BYTES=12000): the batches
    of ONE range each give a part; the file is the production binary's single-batch file."""
    flags = ["--stream-loci", "0", "--ingest", "host", "--prep", prep]
    out1, ref1, a1 = outputs(tmp_path, "one", "alt_frac", False)
    log1 = run_cli(hostlib.CLI_PATH, dna_bam, a1 + flags, tmp_path)
    assert "Matrix written from the device (vtx_write_mtx_f64)" in log1
    out2, ref2, a2 = outputs(tmp_path, "many", "alt_frac", False)
    log2 = run_cli(hostlib.cli_path("dev"), dna_bam, a2 + flags, tmp_path, env={"VTXH_BATCH_BYTES": "12000"})
    n_batches = int(re.search(r"pack of range 0: [\d.]+ s \((\d+) batch", log2).group(1))
    assert n_batches > 3 and n_parts_logged(log2) == n_batches and "host formatter" not in log2
    assert open(out1, "rb").read() == open(out2, "rb").read() and counters(log1) == counters(log2)


@pytest.mark.parametrize("mode,gz", [("consensus", False), ("alt_frac", True), ("coverage", True)])
def test_cli_a_declined_part_is_formatted_on_the_host(tmp_path, dna_bam, mode, gz):
    """bin/vartrix_dev with VTX_MTX_PART_DECLINE=2: the second vtx_mtx_part of the process declines (consensus / alt_frac: the second
    range's; coverage: the first range's ref matrix) — that ONE run's triplets are fetched and vtxh_mtx_part formats them, the other
    parts stay device-made, and the files are the same."""
    out1, ref1, a1 = outputs(tmp_path, "whole", mode, gz)
    log1 = run_cli(hostlib.CLI_PATH, dna_bam, a1 + ["--stream-loci", "0"], tmp_path)
    out2, ref2, a2 = outputs(tmp_path, "declined", mode, gz)
    log2 = run_cli(hostlib.cli_path("dev"), dna_bam, a2 + ["--stream-loci", "7"], tmp_path, env={"VTX_MTX_PART_DECLINE": "2"})
    assert "Matrix written from the device in 7 parts (vtx_mtx_part), 1 formatted on the host" in log2 and "host formatter" not in log2
    assert matrices(out1, ref1, mode, gz) == matrices(out2, ref2, mode, gz) and counters(log1) == counters(log2)


def test_cli_gather_library_keeps_the_host_formatter(tmp_path, dna_bam):
    """Two ranges (every range joins an RCCL communicator of its own: seconds each) through --gather library: fetched and formatted on
    the host as before; the same two ranges without it: two parts, the same bytes."""
    out, ref, args = outputs(tmp_path, "lib", "consensus", False)
    log = run_cli(hostlib.CLI_PATH, dna_bam, args + ["--stream-loci", "23", "--ingest", "host", "--gather", "library"], tmp_path,
                  env={"HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    assert "Matrix written by the host formatter (vtxh_write_mtx)" in log and "vtx_mtx_part" not in log
    out2, ref2, args2 = outputs(tmp_path, "parts", "consensus", False)
    log2 = run_cli(hostlib.CLI_PATH, dna_bam, args2 + ["--stream-loci", "23", "--ingest", "host"], tmp_path)
    assert n_parts_logged(log2) == 2 and open(out, "rb").read() == open(out2, "rb").read()
