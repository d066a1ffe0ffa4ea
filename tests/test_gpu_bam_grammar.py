"""The grammar BAMs of tests/bam_grammar_util.py (every record one case: CIGAR ops, the end-position rule, the aux grammar, the sixteen
base codes, the record layout) through the DEVICE: bam_scan_kernel and what follows it against the host packer's raw pack — records,
loci, tag arena, read arena, counters, then the triplets after vtx_run — and the command line against the oracle pipeline
(oracle/refpipe.py's pack + the C oracle), byte for byte.  The same BAMs go through the host packer against refpipe and the model in
tests/test_bam_grammar.py; the kernel's record logic alone runs on the CPU in tests/test_scan_core.py."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bam_grammar_util as M  # noqa: E402
from oracle import bamwriter, oracle, refpipe  # noqa: E402
from vartrix_amd import abi, hostlib, lib  # noqa: E402
from vartrix_amd.abi import default_config  # noqa: E402

pytestmark = pytest.mark.gpu

G = os.path.join(HERE, "golden")
VCF, FA, BCS = (os.path.join(G, n) for n in ("test_dna.vcf", "test_dna.fa", "dna_barcodes.tsv"))


@pytest.fixture(scope="module", autouse=True)
def dev_host_library():
    # (the planner's threshold knob of the segmented case exists in the developer build of the host library only)
    hostlib.use_variant("dev")
    if not (os.path.exists(hostlib.CLI_PATH) and os.path.exists(hostlib.LIB_PATH) and os.path.exists(lib.LIB_PATH)):
        import __graft_entry__
        __graft_entry__.build()
    yield
    hostlib.use_variant("dev" if os.environ.get("VTX_LIB_VARIANT") == "dev" else "")


def family_bam(family, tmp_path, block=700, index="linear"):
    fa = refpipe.read_fasta(FA)["1"].upper()
    vcf = refpipe.read_vcf(VCF)
    bcs = list(refpipe.load_barcodes(BCS).keys())
    cases = M.family_cases(family, fa, vcf, bcs)
    return cases, M.write_family(str(tmp_path / ("%s_%s.bam" % (family, index))), cases, len(fa), block=block, index=index)


@pytest.mark.parametrize("opts", [dict(), dict(mapq=30), dict(primary_only=True, no_duplicates=True), dict(use_umi=True)],
                         ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()) or "default")
@pytest.mark.parametrize("family", M.FAMILIES)
def test_family_through_the_device_ingest(tmp_path, family, opts):
    """Device ingest == the host's raw pack, byte for byte, and the same triplets after vtx_run."""
    from test_gpu_ingest import ingest_and_compare
    cases, bam = family_bam(family, tmp_path)
    st = ingest_and_compare(dict(vcf=VCF, bam=bam, fasta=FA, cell_barcodes=BCS), pack_kw=opts)
    assert 0 < int(st.bam_records) <= len(cases) and int(st.raw_records) > 5      # (the plan may stop in front of the unplaced reads)
    # the counters the scan is responsible for, against the model
    pm, _ = M.predict(cases, refpipe.read_vcf(VCF), [], **opts)          # (no list: every pair with a barcode tag ends at num_not_cell_bc)
    for name, got in (("num_reads", st.num_reads), ("num_low_mapq", st.num_low_mapq), ("num_non_primary", st.num_non_primary),
                      ("num_duplicates", st.num_duplicates), ("num_not_useful", st.num_not_useful)):
        assert int(got) == pm[name], (name, int(got), pm[name])


@pytest.mark.parametrize("family", M.FAMILIES)
def test_family_with_a_csi_index_and_larger_blocks(tmp_path, family):
    from test_gpu_ingest import ingest_and_compare
    cases, bam = family_bam(family, tmp_path, block=3000, index="csi")
    st = ingest_and_compare(dict(vcf=VCF, bam=bam, fasta=FA, cell_barcodes=BCS), pack_kw=dict(use_umi=True, mapq=10))
    assert 0 < int(st.bam_records) <= len(cases)


def sparse_inputs(tmp_path, family="ops", n_background=9000):
    """The family's records among plain reads all over the contig, and a VCF of two loci far apart: a segmented plan."""
    rng = np.random.default_rng(17)
    fa = refpipe.read_fasta(FA)["1"].upper()
    vcf = refpipe.read_vcf(VCF)
    bcs = list(refpipe.load_barcodes(BCS).keys())
    cases = M.family_cases(family, fa, [v for v in vcf if v.pos in (13115, 13117, 236720, 239163)], bcs)      # every case at one of the four loci
    for k in range(n_background):
        start = int(rng.integers(0, len(fa) - 200))
        cases.append(dict(name="background", tid=0, pos=start, cigar=M.parse("100M"), flag=0, mapq=60, seq=fa[start:start + 100].decode(), qname="b%05d" % k,
                          aux=bamwriter.aux_bytes([("CB", "Z", bcs[k % 40]), ("UB", "Z", "U%02d" % (k % 50))])))
    bam = M.write_family(str(tmp_path / "sparse.bam"), cases, len(fa), block=4000)
    lines = open(VCF).read().splitlines()
    keep = [ln for ln in lines if ln.startswith("#") or ln.split("\t")[1] in ("13116", "13118", "236721", "239164")]
    sv = str(tmp_path / "sparse.vcf")
    open(sv, "w").write("\n".join(keep) + "\n")
    return dict(vcf=sv, bam=bam, fasta=FA, cell_barcodes=BCS)


def test_ops_family_through_a_segmented_plan(tmp_path, monkeypatch):
    """vtx_submit_bam_segments: the ops family's records around two groups of loci 220 kb apart, background reads between them."""
    import segments_util as su
    from test_gpu_ingest_segments import segmented_ingest_and_compare
    monkeypatch.setenv("VTXH_SPARSE_KIB", su.SPARSE_KIB)
    st = segmented_ingest_and_compare(sparse_inputs(tmp_path), pack_kw=dict(use_umi=True))
    assert int(st.raw_records) > 60 and int(st.num_not_useful) > 20


def test_a_record_whose_fields_run_past_its_block_size_is_declined(tmp_path):
    """l_seq larger than the record: the scan sets VTXG_ERR_RECORD, vtx_submit_bam answers VTX_E_UNSUPPORTED (the caller packs on the
    host, which reports the malformed record), and the context is fine afterwards.  Nothing is read outside the record: the scan
    looks at the fixed fields only."""
    fa = refpipe.read_fasta(FA)["1"].upper()
    vcf = refpipe.read_vcf(VCF)
    bcs = list(refpipe.load_barcodes(BCS).keys())
    cases = M.family_cases("layout", fa, vcf, bcs)
    good = M.write_family(str(tmp_path / "good.bam"), cases, len(fa), block=3000)
    order = sorted(range(len(cases)), key=lambda i: (cases[i]["tid"] < 0, cases[i]["tid"], cases[i]["pos"], i))
    recs = []
    for n, i in enumerate(order):
        c = cases[i]
        r = bytearray(bamwriter.record(c["tid"], c["pos"], c["qname"], c["seq"], M.encode(c["cigar"]), flag=c["flag"], mapq=c["mapq"], tags=[(None, "raw", c["aux"])]))
        if n == 7:
            struct.pack_into("<i", r, 20, len(r))               # l_seq: the bases alone would fill the record
        recs.append(bytes(r))
    bad = str(tmp_path / "bad.bam")
    bamwriter.write_bam(bad, [("1", len(fa))], recs, block=3000)
    with pytest.raises(hostlib.HostError, match="malformed BAM record"):
        hostlib.pack_files(VCF, bad, FA, BCS)
    with hostlib.plan_ingest(VCF, bad, FA, BCS) as plan, hostlib.plan_ingest(VCF, good, FA, BCS) as gplan:
        assert plan.reason is None, plan.reason
        with lib.Context(default_config(n_barcodes=len(plan.barcodes))) as ctx:
            ctx.set_barcodes(plan.barcodes)
            with pytest.raises(lib.VtxError) as ei:
                ctx.submit_bam(plan.ingest, plan.n_loci)
            assert ei.value.status == abi.VTX_E_UNSUPPORTED
            st = ctx.submit_bam(gplan.ingest, gplan.n_loci)
            assert 0 < int(st.bam_records) <= len(cases)


PATHS = {"host": ["--ingest", "host", "--prep", "host"], "device": ["--ingest", "host", "--prep", "device"], "ingest": ["--ingest", "device"]}
_oracle_cache = {}


def oracle_text(family, bam, mode, aligner):
    key = (family, mode, aligner)
    if key not in _oracle_cache:
        bcs = refpipe.load_barcodes(BCS)
        vcf = refpipe.read_vcf(VCF)
        if family not in _oracle_cache:
            _oracle_cache[family] = refpipe.pack(vcf, refpipe.read_fasta(FA), refpipe.read_bam(bam), bcs, refpipe.Args())
        batch, wm = _oracle_cache[family]
        cfg = default_config(aligner=aligner, scoring_mode=mode, use_umi=0, n_barcodes=len(bcs))
        r, a = oracle.batch_scores(batch, cfg, threads=8)
        coo = oracle.batch_reduce(batch, cfg, r, a)
        _oracle_cache[key] = (refpipe.mtx_text(len(vcf), len(bcs), coo["row"], coo["col"], coo["value"]),
                              refpipe.mtx_text(len(vcf), len(bcs), coo["row"], coo["col"], coo["ref_value"]), wm, len(coo["row"]))
    return _oracle_cache[key]


@pytest.mark.parametrize("prep", ["host", "device", "ingest"])
@pytest.mark.parametrize("aligner", ["banded", "full"])
@pytest.mark.parametrize("mode", ["consensus", "alt_frac", "coverage"])
@pytest.mark.parametrize("family", ["ops", "bases"])
def test_cli_equals_the_oracle_pipeline(tmp_path, family, mode, aligner, prep):
    """The command line on the ops and bases families: byte-identical to refpipe.pack + oracle.batch_scores + batch_reduce + mtx_text."""
    cases, bam = family_bam(family, tmp_path)
    out, ref = str(tmp_path / "out.mtx"), str(tmp_path / "ref.mtx")
    args = ["-v", VCF, "-b", bam, "-f", FA, "-c", BCS, "-o", out, "-s", mode, "--ref-matrix", ref, "--threads", "4", "--aligner", aligner,
            "--log-level", "info"] + PATHS[prep]
    r = subprocess.run([hostlib.CLI_PATH] + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("ingest on the device" in r.stderr) == (prep == "ingest")
    text, ref_text, wm, nnz = oracle_text(family, bam, mode, aligner)
    log = r.stdout + r.stderr
    for ln in ("Number of alignments evaluated: %d" % wm["num_reads"],
               "Number of alignments skipped due to not being associated with a cell barcode: %d" % wm["num_not_cell_bc"],
               "Number of alignments skipped due to not intersecting variant: %d" % wm["num_not_useful"]):
        assert ln + "\n" in log, ln
    assert open(out).read() == text
    if mode == "coverage":
        assert open(ref).read() == ref_text
    assert nnz > 10


def _banded_run(batch, nb):
    cfg = default_config(aligner="banded", scoring_mode="coverage", use_umi=0, n_barcodes=nb)
    with lib.Context(cfg) as ctx:
        ctx.set_stage_trace(True)
        ctx.submit(batch)
        ctx.run()
        r, a = ctx.fetch_scores()
        stage = ctx.fetch_stage().reshape(-1, 2)
    oref, oalt = oracle.batch_scores(batch, cfg, threads=8)
    assert np.array_equal(r, oref) and np.array_equal(a, oalt)
    return stage


def _outside(batch):
    return np.array([bool(set(batch.read_arena[int(rec["read_off"]):int(rec["read_off"]) + int(rec["read_len"])].tobytes()) - set(b"ACGTN"))
                     for rec in batch.records])


def test_reads_with_ambiguity_codes_take_the_general_kernels(tmp_path):
    """Reads that hold IUPAC codes or '=' are outside band_sweep_kernel's ACGTN alphabet: the sweep declines them and the general
    kernel of vtx_band.hip builds their band.  (a) The bases family: every score equals the oracle's and no such task is decided by
    the sweep.  (b) Whether a task gets as far as the sweep at all depends on the certificates in front of it, so the second part
    takes the reads of a noisy indel batch whose tasks the sweep DID decide, writes the twelve codes that are not ACGTN into them,
    and runs again: none of them is decided by the sweep any more, at least one is decided by the general kernel + masked DP, and
    every score of the batch equals the oracle's — so that path's scores are compared."""
    from vartrix_amd import synth
    cases, bam = family_bam("bases", tmp_path)
    bcs = refpipe.load_barcodes(BCS)
    batch, _ = refpipe.pack(refpipe.read_vcf(VCF), refpipe.read_fasta(FA), refpipe.read_bam(bam), bcs, refpipe.Args())
    stage = _banded_run(batch, len(bcs))
    outside = _outside(batch)
    print("bases family, %d tasks whose read leaves ACGTN: %s" % (2 * int(outside.sum()), {abi.STAGE_NAMES[int(k)]: int((stage[outside] == k).sum()) for k in np.unique(stage[outside])}))
    assert outside.sum() >= 12
    assert not (stage[outside] == abi.STAGE_SWEEP_DP).any()
    # (b)
    spec = synth.SynthSpec(n_loci=200, n_barcodes=300, reads_per_locus=48, sub_error=0.05, indel_frac=0.3, seed=3)
    noisy = synth.make_batch(spec)
    stage = _banded_run(noisy, spec.n_barcodes)
    swept = np.nonzero((stage == abi.STAGE_SWEEP_DP).any(axis=1))[0]
    print("noisy batch: %d records with a task the sweep decided" % swept.size)
    assert swept.size >= 20
    arena = noisy.read_arena.copy()
    codes = b"=MRSVWYHKDB" + b"M"
    for n, rid in enumerate(swept):
        off, ln = int(noisy.records["read_off"][rid]), int(noisy.records["read_len"][rid])
        for k, j in enumerate(range(7, ln, 29)):
            arena[off + j] = codes[(n + k) % 12]
    changed = abi.PackedBatch(noisy.loci, noisy.records, noisy.hap_arena, arena)
    stage2 = _banded_run(changed, spec.n_barcodes)
    hist = {abi.STAGE_NAMES[int(k)]: int((stage2[swept] == k).sum()) for k in np.unique(stage2[swept])}
    print("the same records with ambiguity codes written in: %s" % hist)
    assert _outside(changed)[swept].all()
    assert not (stage2[swept] == abi.STAGE_SWEEP_DP).any(), hist
    assert (stage2[swept] == abi.STAGE_GENERAL_DP).any(), hist
