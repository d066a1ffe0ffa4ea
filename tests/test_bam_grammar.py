"""A grammar BAM through the host packer: every record is one case of tests/bam_grammar_util.py's families — CIGAR ops (H, P, =, X,
leading I / D / N, H between operations, zero-length ops, no ops), the end-position rule (flag 0x4 with a CIGAR, no
reference-consuming op), the aux grammar (every type and B subtype, duplicates, the empty Z, values at the 16-bit edge, UB before CB,
no aux bytes), the sixteen base codes with l_seq 0 / 1 / odd, and the record layout (l_read_name 1 .. 255, tid -1 at the file's end)
— placed over the loci of test_dna.vcf, with BGZF blocks small enough that records straddle them.

hostlib.pack_files == oracle/refpipe.py's pack (batch and all nine metrics) for each option set of
tests/test_host.py::test_packer_on_authored_indel_bam, and the independently written model predicts, per case, which (read, locus)
pairs survive and which counter each dropped pair lands in.  The device ingest runs the same BAMs in tests/test_gpu_bam_grammar.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bam_grammar_util as M  # noqa: E402
from oracle import refpipe  # noqa: E402
from test_host import same_batch  # noqa: E402
from vartrix_amd import hostlib  # noqa: E402

G = os.path.join(HERE, "golden")
VCF, FA, BCS = (os.path.join(G, n) for n in ("test_dna.vcf", "test_dna.fa", "dna_barcodes.tsv"))
OPTION_SETS = [dict(), dict(use_umi=True), dict(mapq=30), dict(primary_only=True, no_duplicates=True), dict(padding=20), dict(use_umi=True, padding=150)]


@pytest.fixture(scope="module", autouse=True)
def built():
    hostlib.use_variant("dev")
    if not (os.path.exists(hostlib.LIB_PATH) and os.path.exists(hostlib.CLI_PATH)):
        import __graft_entry__
        __graft_entry__.build()
    yield
    hostlib.use_variant("dev" if os.environ.get("VTX_LIB_VARIANT") == "dev" else "")


def inputs_of(family, tmp_path, block=700, index="linear"):
    fa = refpipe.read_fasta(FA)["1"].upper()
    vcf = refpipe.read_vcf(VCF)
    bcs = list(refpipe.load_barcodes(BCS).keys())
    cases = M.family_cases(family, fa, vcf, bcs)
    bam = M.write_family(str(tmp_path / (family + ".bam")), cases, len(fa), block=block, index=index)
    return cases, vcf, bcs, bam


@pytest.mark.parametrize("kw", OPTION_SETS, ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()) or "default")
@pytest.mark.parametrize("family", M.FAMILIES)
def test_grammar_bam_through_the_packer(tmp_path, family, kw, monkeypatch):
    if family in ("ops", "layout"):
        monkeypatch.setenv("VTXH_CHUNK_BLOCKS", "2")            # many windows: records straddle them too
    cases, vcf, bcs, bam = inputs_of(family, tmp_path)
    batch, metrics, nv, barcodes, variants = hostlib.pack_files(VCF, bam, FA, BCS, threads=2, **kw)
    args = refpipe.Args(mapq=kw.get("mapq", 0), primary=kw.get("primary_only", False), duplicates=kw.get("no_duplicates", False),
                        use_umi=kw.get("use_umi", False), padding=kw.get("padding", 100))
    rbam = refpipe.read_bam(bam)
    assert len(rbam.recs) == len(cases)
    want, wm = refpipe.pack(vcf, refpipe.read_fasta(FA), rbam, refpipe.load_barcodes(BCS), args)
    # the model first: it names the case
    opts = {k: v for k, v in kw.items() if k != "padding"}
    pm, kept = M.predict(cases, vcf, bcs, **opts)
    by_len = {len(c["seq"]): c["name"] for c in cases}
    for side, b, m in (("refpipe.pack", want, wm), ("hostlib.pack_files", batch, metrics)):
        got = {int(L["row"]): sorted(int(x) for x in b.records["read_len"][int(L["rec_begin"]):int(L["rec_begin"]) + int(L["rec_count"])]) for L in b.loci}
        for row in kept:
            extra = sorted(set(got[row]) ^ set(kept[row]))
            assert got[row] == kept[row], "%s, locus row %d (pos %d): cases that differ from the model: %s" % (side, row, vcf[row].pos, [by_len[x] for x in extra])
        for name, v in pm.items():
            assert m[name] == v, "%s: %s = %d, model %d" % (side, name, m[name], v)
    assert metrics == wm and set(metrics) == set(refpipe.METRIC_NAMES) and len(metrics) == 9
    assert nv == 46 and batch.n_loci == 45 and metrics["num_multiallelic_recs"] == 1
    assert same_batch(batch, want)
    assert metrics["num_reads"] > 20


def test_every_family_exercises_what_it_is_for():
    """The corpus itself, on the model alone: each family produces kept pairs and the dropped kinds it exists for."""
    fa = refpipe.read_fasta(FA)["1"].upper()
    vcf = refpipe.read_vcf(VCF)
    bcs = list(refpipe.load_barcodes(BCS).keys())
    seen = {}
    for family in M.FAMILIES:
        cases = M.family_cases(family, fa, vcf, bcs)
        pm, kept = M.predict(cases, vcf, bcs, use_umi=True)
        seen[family] = pm
        assert sum(len(v) for v in kept.values()) > 5, family
        assert max(len(c["aux"]) for c in cases) > 700 or family != "aux"
    assert seen["ops"]["num_not_useful"] > 20 and seen["endpos"]["num_not_useful"] > 5
    assert seen["aux"]["num_not_cell_bc"] > 10 and seen["aux"]["num_non_umi"] > 3
    # an unmapped record with a CIGAR that starts in front of a locus is not fetched at all (bam_endpos = pos + 1) ...
    cases = [c for c in M.family_cases("endpos", fa, vcf, bcs) if c["flag"] & 4 and M.text(c["cigar"]) == "60M"]
    fetched = [(c["name"], v.pos) for c in cases for v in vcf if len(v.alleles) <= 2 and M.pair_outcome(c, v.pos, v.pos + len(v.alleles[0]), set(bcs)) is not None]
    assert cases and all(n.split("@-")[1].startswith("0 ") for n, _ in fetched) and fetched
    # ... although its CIGAR alone would reach it: the rule refpipe.read_bam did not have
    assert any(c["pos"] < v.pos < c["pos"] + 60 for c in cases for v in vcf)
    # several loci under one read
    ops = M.family_cases("ops", fa, vcf, bcs)
    both = next(c for c in ops if c["name"].endswith("61987 and 61989 both"))
    assert sum(M.pair_outcome(both, v.pos, v.pos + len(v.alleles[0]), set(bcs)) == "kept" for v in vcf) == 2


def test_umi_of_65535_bytes_is_beyond_the_tag_length_format(tmp_path):
    """A KNOWN LIMIT, pinned as it is: vtx_raw_record carries tag lengths as 16 bits and 0xffff (VTX_TAG_MISSING) means "no such
    tag", so a UB value of 65 535 bytes or more cannot travel.  The reference (and refpipe, and the model) keeps such a read under
    --umi; the host packer and the device count it in num_non_umi.  65 534 bytes is the longest value that survives (it is a case of
    the aux family).  A barcode that long is in nobody's list, so there the outcome is the same on every side."""
    from oracle import bamwriter
    fa = refpipe.read_fasta(FA)["1"].upper()
    vcf = refpipe.read_vcf(VCF)
    bcs = list(refpipe.load_barcodes(BCS).keys())
    at = vcf[0].pos
    case = dict(name="UB of 65535 bytes", tid=0, pos=at - 20, cigar=M.parse("60M"), flag=0, mapq=60, seq=fa[at - 20:at + 40].decode(), qname="q",
                aux=bamwriter.aux_bytes([("CB", "Z", bcs[0]), ("UB", "Z", b"G" * 65535)]))
    bam = M.write_family(str(tmp_path / "umi.bam"), [case], len(fa))
    pm, _ = M.predict([case], vcf, bcs, use_umi=True)
    _, wm = refpipe.pack(vcf, refpipe.read_fasta(FA), refpipe.read_bam(bam), refpipe.load_barcodes(BCS), refpipe.Args(use_umi=True))
    _, hm, *_ = hostlib.pack_files(VCF, bam, FA, BCS, use_umi=True)
    assert pm["num_reads"] == wm["num_reads"] == hm["num_reads"] == 2          # (13116 and 13118)
    assert pm["num_non_umi"] == wm["num_non_umi"] == 0 and hm["num_non_umi"] == 2
    _, hm0, *_ = hostlib.pack_files(VCF, bam, FA, BCS)                          # without --umi the read is kept on every side
    assert hm0["num_non_umi"] == 0 and hm0["num_not_cell_bc"] == 0
