"""Device-side BAM ingest of a SEGMENTED plan (sparse loci: vtx_submit_bam_segments, bam_chain_seg_kernel) against the host packer.

The same comparison tests/test_gpu_ingest.py makes for the contiguous plan: the raw records, their loci, the tag arena and the read
arena the device builds are the bytes vtxh_pack_files_raw builds (after a stable sort by locus), every Metrics counter is equal, and
the resolved records, scores and triplets equal the host-packed run's.  Plus what is new: only the segments' bytes travel and are
inflated, a plan that is wrong is declined with a reason and leaves the context usable, and the CLI takes the segmented path where it
used to say "sparse loci" — with the production binary on a BAM above the real thresholds."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from vartrix_amd import abi, hostlib, lib
from vartrix_amd.abi import default_config

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import segments_util as su  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def dev_host_library():
    # the planner's threshold knob exists in the developer build of the host library only; the device library is the production one
    hostlib.use_variant("dev")
    yield
    hostlib.use_variant("dev" if os.environ.get("VTX_LIB_VARIANT") == "dev" else "")


@pytest.fixture()
def knob(monkeypatch):
    monkeypatch.setenv("VTXH_SPARSE_KIB", su.SPARSE_KIB)


def segmented_ingest_and_compare(inputs, cfg_kw=None, pack_kw=None, want_kind="segmented"):
    pack_kw = dict(pack_kw or {})
    use_umi = bool(pack_kw.get("use_umi", False))
    want, wmetrics, nv, barcodes, variants = hostlib.pack_files(raw=True, nibbles=True, threads=3, **inputs, **pack_kw)
    with hostlib.plan_ingest(**inputs, **pack_kw) as plan:
        assert plan.reason is None, plan.reason
        assert plan.kind == want_kind
        assert plan.n_variants == nv and plan.barcodes == barcodes and plan.variants == variants
        a = plan.arrays()
        cfg = default_config(n_barcodes=len(barcodes), use_umi=int(use_umi), **(cfg_kw or {}))
        with lib.Context(cfg) as ctx:
            ctx.set_barcodes(barcodes)
            st = ctx.submit_bam_segments(plan.segments, plan.n_loci) if plan.kind == "segmented" else ctx.submit_bam(plan.ingest, plan.n_loci)
            raw = ctx.debug_ingest(abi.INGEST_RAW_RECORDS, abi.RAW_RECORD_DTYPE)
            locus = ctx.debug_ingest(abi.INGEST_RAW_LOCUS, np.uint32)
            tags = ctx.debug_ingest(abi.INGEST_TAGS)
            reads = ctx.debug_ingest(abi.INGEST_READS_PACKED)
            stream = ctx.debug_ingest(abi.INGEST_INFLATED)
            offs = ctx.debug_ingest(abi.INGEST_RECORD_OFFSETS, np.uint64)
            recs, begin, count = ctx.fetch_records()
            ctx.run()
            coo = ctx.fetch_coo()
            sc = ctx.fetch_scores()
        order = np.argsort(locus, kind="stable")
        raw_s, locus_s = raw[order], locus[order]
        wl = np.repeat(np.arange(want.n_loci, dtype=np.uint32), want.loci["rec_count"])
        assert np.array_equal(locus_s, wl)
        assert np.array_equal(raw_s, want.records), np.nonzero(raw_s != want.records)[0][:5]
        assert np.array_equal(tags, want.tag_arena)
        assert np.array_equal(reads, want.read_arena)
        got = dict(plan.metrics)
        got.update(num_reads=int(st.num_reads), num_low_mapq=int(st.num_low_mapq), num_non_primary=int(st.num_non_primary),
                   num_duplicates=int(st.num_duplicates), num_not_useful=int(st.num_not_useful),
                   num_not_cell_bc=int(st.num_no_barcode_tag), num_non_umi=0)
        assert got == wmetrics, (got, wmetrics)
        with lib.Context(cfg) as c2:
            c2.set_barcodes(barcodes)
            rs = c2.submit_raw(want)
            recs2, begin2, count2 = c2.fetch_records()
            c2.run()
            coo2 = c2.fetch_coo()
            sc2 = c2.fetch_scores()
        assert (int(st.raw.num_not_cell_bc), int(st.raw.num_non_umi), int(st.raw.kept)) == (int(rs.num_not_cell_bc), int(rs.num_non_umi), int(rs.kept))
        assert np.array_equal(recs, recs2) and np.array_equal(begin, begin2) and np.array_equal(count, count2)
        assert np.array_equal(sc[0], sc2[0]) and np.array_equal(sc[1], sc2[1])
        for k in coo:
            x, y = np.asarray(coo[k]), np.asarray(coo2[k])
            assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k
        if plan.kind == "segmented":
            # only the segments' bytes were inflated: the stream is the concatenation of the planned blocks, the record offsets point
            # into it, and it is smaller than the one stretch the contiguous plan would have inflated
            f = open(inputs["bam"], "rb").read()
            assert int(st.inflated_bytes) == int(a["blocks"]["isize"].sum()) == stream.size
            assert int(st.inflated_bytes) < a["contiguous_inflated"] and int(st.compressed_bytes) < a["contiguous_compressed"]
            assert stream.tobytes() == su.inflate(f, a["blocks"])
            assert offs.size == int(st.bam_records) and np.all(np.diff(offs.astype(np.int64)) > 0) and int(offs[-1]) < stream.size
        return st


@pytest.mark.parametrize("block,index", [(700, "linear"), (4000, "csi"), (20000, "linear")])
@pytest.mark.parametrize("umi", [False, True])
def test_segmented_ingest_equals_the_host_packer(tmp_path, knob, block, index, umi):
    st = segmented_ingest_and_compare(su.author(tmp_path, block=block, index=index), pack_kw=dict(use_umi=umi))
    assert st.raw_records > 100


@pytest.mark.parametrize("opts", [dict(), dict(mapq=30), dict(primary_only=True, no_duplicates=True), dict(use_umi=True, mapq=10),
                                  dict(bam_tag="CR"), dict(padding=30)])
def test_segmented_ingest_with_every_filter(tmp_path, knob, opts):
    """The option sets of tests/test_gpu_ingest.py::test_authored_bam_with_every_filter (the authored reads carry mapping qualities
    0 - 60, duplicate and secondary flags, and some lack the UB tag)."""
    st = segmented_ingest_and_compare(su.author(tmp_path, block=4000), pack_kw=opts)
    assert (st.raw_records > 0) == ("bam_tag" not in opts)


def test_ranges_of_rows_add_up(tmp_path, knob):
    """Streamed ranges: a range may be segmented or not; each equals the host pack of that range, and the pairs add up."""
    inputs = su.author(tmp_path, block=4000)
    whole = segmented_ingest_and_compare(inputs, pack_kw=dict(use_umi=True))
    parts = [segmented_ingest_and_compare(inputs, pack_kw=dict(use_umi=True, rows=r), want_kind=k)
             for r, k in (((0, 3), "segmented"), ((3, 4), "contiguous"), ((4, len(su.LOCI)), "segmented"))]
    assert sum(int(p.raw_records) for p in parts) == int(whole.raw_records)
    assert sum(int(p.num_reads) for p in parts) == int(whole.num_reads)


def test_wrong_plans_are_declined(tmp_path, knob):
    """A moved seed, a stated end that is not a record start, an end that does not prove itself: VTX_E_UNSUPPORTED with a reason (the
    caller packs on the host).  A segment cut short by one block, a seed outside its segment: VTX_E_INVAL.  Nothing is submitted, and
    the context takes the right plan afterwards."""
    inputs = su.author(tmp_path, block=4000)
    with hostlib.plan_ingest(**inputs) as plan:
        assert plan.kind == "segmented"
        a = plan.arrays()
        with lib.Context(default_config(n_barcodes=len(plan.barcodes))) as ctx:
            with pytest.raises(lib.VtxError) as ei:
                ctx.submit_bam_segments(plan.segments, plan.n_loci)
            assert ei.value.status == abi.VTX_E_STATE                    # no barcode list
            ctx.set_barcodes(plan.barcodes)

            def attempt(seeds=None, segs=None, n_blocks=None):
                g = abi.VtxBamSegments.from_buffer_copy(plan.segments)
                keep = (seeds, segs)
                if seeds is not None:
                    g.base.seeds = seeds.ctypes.data
                if segs is not None:
                    g.segments = segs.ctypes.data
                if n_blocks is not None:
                    g.base.n_blocks = n_blocks
                with pytest.raises(lib.VtxError) as ei:
                    ctx.submit_bam_segments(g, plan.n_loci)
                del keep
                with pytest.raises(lib.VtxError):
                    ctx.run()                                            # nothing was submitted
                return ei.value
            seeds = a["seeds"].copy()
            seeds[int(a["segments"]["seed_begin"][1]) + 1] += 1          # a seed that is not a record start
            e = attempt(seeds=seeds)
            assert e.status == abi.VTX_E_UNSUPPORTED and "record chain" in str(e)
            segs = a["segments"].copy()
            assert not int(segs["flags"][1]) & abi.SEGMENT_TO_EOF
            segs["end_upos"][1] -= 1                                     # a stated end that is not a record start
            e = attempt(segs=segs)
            assert e.status == abi.VTX_E_UNSUPPORTED and "record chain" in str(e)
            segs = a["segments"].copy()
            segs["end_pos"][1] = 2**31 - 1                               # the record at the end does not lie behind THIS coordinate
            e = attempt(segs=segs)
            assert e.status == abi.VTX_E_UNSUPPORTED and "cannot prove" in str(e)
            segs = a["segments"].copy()
            segs["block_end"][-1] -= 1                                   # the last segment cut short by one block
            e = attempt(segs=segs, n_blocks=len(a["blocks"]) - 1)
            assert e.status == abi.VTX_E_INVAL and "outside its blocks" in str(e)
            seeds = a["seeds"].copy()
            seeds[int(a["segments"]["seed_begin"][2])] = seeds[int(a["segments"]["seed_begin"][2]) - 1]      # a seed of the segment before
            e = attempt(seeds=seeds)
            assert e.status == abi.VTX_E_INVAL
            st = ctx.submit_bam_segments(plan.segments, plan.n_loci)     # the context is fine afterwards
            assert st.bam_records > 1000 and int(st.inflated_bytes) == int(a["blocks"]["isize"].sum())
            ctx.run()


def test_a_prefetch_in_flight_is_dropped(tmp_path, knob):
    """vtx_prefetch_file of the whole BAM (what the CLI starts at launch for a BAM below 4 GiB), then a segmented plan: the same
    ingest, and no prefetch is reported as used."""
    inputs = su.author(tmp_path, block=20000)
    with hostlib.plan_ingest(**inputs) as plan:
        outs = []
        for pf in (False, True):
            with lib.Context(default_config(n_barcodes=0 if pf else len(plan.barcodes))) as ctx:
                if pf:
                    ctx.prefetch_file(inputs["bam"], 0, 0)
                ctx.set_barcodes(plan.barcodes)
                st = ctx.submit_bam_segments(plan.segments, plan.n_loci)
                assert st.prefetch_ms == 0 and st.prefetch_wait_ms == 0
                ctx.run()
                coo = ctx.fetch_coo()
                outs.append((int(st.raw_records), ctx.debug_ingest(abi.INGEST_RAW_RECORDS).tobytes(), coo["row"].tobytes(), coo["value"].tobytes()))
        assert outs[0] == outs[1] and outs[0][0] > 0


def cli(variant, inputs, out, extra, env=None, cwd=None):
    args = ["-v", inputs["vcf"], "-b", inputs["bam"], "-f", inputs["fasta"], "-c", inputs["cell_barcodes"], "-o", out, "--log-level", "info"] + extra
    return subprocess.run([hostlib.cli_path(variant)] + args, cwd=cwd, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, **(env or {})))


@pytest.mark.parametrize("mode", ["consensus", "coverage", "alt_frac"])
def test_cli_segmented_equals_host_ingest(tmp_path, mode):
    """Developer binary with the threshold knob: --ingest device takes the segmented plan and writes the bytes --ingest host writes."""
    inputs = su.author(tmp_path, block=4000)
    outs = {}
    for ingest in ("device", "host"):
        out, ref = str(tmp_path / ("%s.mtx" % ingest)), str(tmp_path / ("%s_ref.mtx" % ingest))
        extra = ["-s", mode, "--umi", "--ingest", ingest] + (["--ref-matrix", ref] if mode == "coverage" else [])
        r = cli("dev", inputs, out, extra, env=dict(VTXH_SPARSE_KIB=su.SPARSE_KIB), cwd=tmp_path)
        assert r.returncode == 0, r.stdout + r.stderr
        log = r.stdout + r.stderr
        assert ("segmented plan" in log and "segmented plan ran" in log) == (ingest == "device"), log
        assert "packing on the host" not in log
        outs[ingest] = (open(out, "rb").read(), open(ref, "rb").read() if mode == "coverage" else b"")
    assert outs["device"] == outs["host"] and len(outs["device"][0].splitlines()) > 50


def test_production_cli_on_a_bam_above_the_real_thresholds(tmp_path):
    """About 100 MiB of inflated BAM, 20 loci on it, the PRODUCTION binary: the planner used to answer "sparse loci" (--ingest device
    failed, auto packed on the host); now --ingest device succeeds on the segmented plan, never falls back, and writes --ingest host's
    bytes."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import e2e_cli_bench
    V = 16000                                                            # 22 reads of 311 bytes per locus: 109 MB inflated
    fa, vcf, bam, bcs, n_reads = e2e_cli_bench.author_fast(str(tmp_path), V, 22, 500, procs=8)
    lines = open(vcf).read().splitlines()
    head, rows = [ln for ln in lines if ln.startswith("#")], [ln for ln in lines if not ln.startswith("#")]
    sparse = str(tmp_path / "sparse.vcf")
    open(sparse, "w").write("\n".join(head + rows[400::800]) + "\n")
    assert len(rows[400::800]) == 20
    inputs = dict(vcf=sparse, bam=bam, fasta=fa, cell_barcodes=bcs)
    outs = {}
    for ingest in ("device", "host"):
        out = str(tmp_path / ("%s.mtx" % ingest))
        r = cli("", inputs, out, ["--umi", "--ingest", ingest], cwd=tmp_path)
        log = r.stdout + r.stderr
        assert r.returncode == 0, log
        assert "packing on the host" not in log and "sparse loci" not in log
        if ingest == "device":
            assert "segmented plan: 20 segments" in log and "segmented plan ran" in log, log
        outs[ingest] = open(out, "rb").read()
    assert outs["device"] == outs["host"] and len(outs["device"].splitlines()) > 200
