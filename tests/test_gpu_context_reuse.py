"""One vtx_ctx, many UNLIKE batches (include/vtx.h: "The batch stays resident until the next vtx_submit"; a context serves any number
of submits).  Every other GPU test opens a fresh context per batch, or runs the same batch again; here each step runs inside buffers
that a different, usually larger, predecessor left dirty, and must give what the CPU oracle and a fresh context give
(tests/reuse_util.py: check_step).  The shapes of the sequences are pinned on the CPU by tests/test_reuse_sequences.py.

  a  ten unlike batches through vtx_submit, three configurations, production library: oracle, stage invariant, stage bytes and task
     counts equal to the fresh context's on every step; the state errors between a submit and its run; Matrix-Market text of a
     small batch after a large one
  b  big / small / big / small under the developer library's hooks for the rare paths (second stage, buffer caps, tail buffer)
  d  failed submits between two good batches leave nothing behind
  e  vtx_gather_coo's staging after batches of different sizes

Non-vacuity: the fresh-context run of a step must have taken the path the step is there for (hard tasks, overflow, the two-pass
split, the slow path, the second stage); the assertions are next to the steps."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import reuse_util as RU
from audit_util import stage_report
from vartrix_amd import abi, hostlib, lib, synth
from vartrix_amd.abi import PackedBatch, default_config

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def seqs():
    return RU.sequences()


def same_result(x, y):
    assert np.array_equal(x["ref"], y["ref"]) and np.array_equal(x["alt"], y["alt"]) and np.array_equal(x["stage"], y["stage"])
    for k in x["coo"]:
        assert np.array_equal(x["coo"][k].view(np.uint8), y["coo"][k].view(np.uint8)), k
    assert x["counts"] == y["counts"] and x["cells"] == y["cells"]


def check_mtx(ctx, got, cfg, batch, tmp_path, tag):
    """vtx_write_mtx / vtx_write_mtx_f64 of the resident result: the host writer's bytes from the fetched triplets, and its sum."""
    coo = got["coo"]
    n_rows, n_cols = max(batch.n_loci, 1), int(cfg.n_barcodes)
    real = cfg.scoring_mode == abi.MODE_ALT_FRAC
    texts = []
    for which, key in ((0, "value"), (1, "ref_value")) if cfg.scoring_mode == abi.MODE_COVERAGE else ((0, "value"),):
        p, q = str(tmp_path / ("%s_dev%d.mtx" % (tag, which))), str(tmp_path / ("%s_host%d.mtx" % (tag, which)))
        s = ctx.write_mtx(p, n_rows, n_cols, which, real=real)
        hostlib.write_mtx(q, n_rows, n_cols, coo["row"], coo["col"], coo[key])
        text = open(p, "rb").read()
        assert text == open(q, "rb").read(), "%s: Matrix-Market text (which = %d) differs from the host writer's" % (tag, which)
        v = np.asarray(coo[key])
        if np.isnan(v).any():
            assert math.isnan(s)
        elif real:
            assert s == pytest.approx(float(v.sum()), rel=1e-9, abs=0.0)
        else:
            assert s == float(v.sum())
        texts.append(text)
    return texts


@pytest.mark.parametrize("name", ["unlike-banded-coverage-umi0", "unlike-banded-alt_frac-umi1", "unlike-full-consensus-umi0"])
def test_unlike_batches_in_sequence_equal_fresh_contexts(seqs, name, tmp_path):
    seq = seqs[name]
    cfg = RU.config_of(seq)
    banded = seq["aligner"] == "banded"
    fresh, got, texts = {}, {}, {}
    with RU.open_context(cfg) as ctx:
        for label, batch in seq["steps"]:
            if id(batch) not in fresh:
                fresh[id(batch)] = RU.run_fresh(batch, cfg)
            f = fresh[id(batch)]
            got[label] = RU.check_step(ctx, batch, cfg, f, "%s, step %s" % (name, label))
            if label[0] in "134":
                texts[label] = check_mtx(ctx, got[label], cfg, batch, tmp_path, "step" + label[0])
            if not banded:
                continue
            # ---- the path the step is there for was taken (on the fresh context) ----
            c = f["counts"]
            if label.startswith("1 "):
                assert c["hard_tasks"] > 0 and (c["swept_tasks"] > 0 or c["checked_tasks"] > 0), c
            if label.startswith("5 "):
                is_long = np.maximum(batch.loci["ref_len"], batch.loci["alt_len"]) > 255
                long_tasks = np.repeat(is_long[np.repeat(np.arange(batch.n_loci), batch.loci["rec_count"])], 2)
                # The two-pass split: the long loci took round 3's kernels, the ordinary ones did not.  band_diag_kernel (and
                # band_refine_kernel behind it) runs in front of BOTH passes, so its certificates decide tasks of long loci too (94 of
                # 138 here; tests/test_gpu_shape.py allows the same two stages): every long task it did NOT decide lies in ROUND3_STAGES,
                # there are such tasks, and no long task carries a stage of the sweep path.
                first = np.isin(f["stage"], (abi.STAGE_DIAG_CERT, abi.STAGE_REFINE_CERT))
                rest = long_tasks & ~first
                assert rest.any() and np.isin(f["stage"][rest], RU.ROUND3_STAGES).all(), stage_report(f["stage"][long_tasks])
                assert not np.isin(f["stage"][~long_tasks], RU.ROUND3_STAGES).all()
                assert np.isin(f["stage"][~long_tasks], (abi.STAGE_SWEEP_DP, abi.STAGE_DIAG_DP, abi.STAGE_BAND_CERT)).any()
            if label.startswith("6 "):
                assert (batch.records["read_len"] > 1024).any() and (f["stage"] == abi.STAGE_SLOW).any()
        if banded:
            over = fresh[id(dict(seq["steps"])["2a repeat-rich"])]["counts"]["overflow_tasks"] + \
                fresh[id(dict(seq["steps"])["2b poly-A / tandem"])]["counts"]["overflow_tasks"]
            assert over > 0, "step 2 sent nothing to the general kernel"
    same_result(got["8 tiny clean again"], got["3 tiny clean"])
    same_result(got["9 noisy indels again"], got["1 noisy indels"])
    # the text of the small batch is the small batch's alone: a header and one line per triplet of ITS matrix
    for label in ("3 tiny clean", "4 empty"):
        for text in texts[label]:
            lines = text.decode().splitlines()
            body = [ln for ln in lines if not ln.startswith("%")]
            assert len(body) == 1 + len(got[label]["coo"]["row"]), label
            assert all(int(ln.split()[0]) <= max(dict(seq["steps"])[label].n_loci, 1) for ln in body[1:])
    assert len(texts["1 noisy indels"][0]) > 50 * len(texts["3 tiny clean"][0])


RARE_CHILD = r'''
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import reuse_util as RU
seq = RU.sequences()["rare-paths"]
cfg = RU.config_of(seq)
caps = sys.argv[1] == "caps"
out = []
with RU.open_context(cfg) as ctx:
    for label, batch in seq["steps"]:
        f = RU.run_fresh(batch, cfg)
        # under a buffer cap, WHICH task spills into the general kernel depends on the order of the atomics that hand out the slots
        # (band_run_kernel's hard / pending lists, vtx_band.hip): no stage-byte equality, no task counts there
        RU.check_step(ctx, batch, cfg, f, label, stage_equal=not caps, counts=() if caps else RU.TASK_COUNTS)
        out.append(f["counts"])
print("REUSE-COUNTS " + json.dumps(out))
''' % (ROOT, HERE)

HOOKS = {
    "diag2": (dict(VTX_BAND_DIAG2_MIN="1"), False),
    "hard_cap": (dict(VTX_BAND_HARD_CAP="3", VTX_BAND_LEGACY="1"), True),
    "slots": (dict(VTX_BAND_SLOTS="3"), True),
    # (band_tail_kernel's record buffer: a lane that finds no slot finishes its task in its wavefront, with the result and the stage byte
    #  the tail kernel would have given it — tests/test_gpu_tail.py compares exactly that, stage bytes and counts, under this cap — so
    #  WHICH lanes find no slot changes no byte: stage-byte equality holds)
    "tail_cap": (dict(VTX_DIAG_TAIL_CAP="700"), False),
}


@pytest.mark.parametrize("hook", list(HOOKS))
def test_rare_paths_on_a_reused_context(hook):
    """libvtx_dev.so (the hooks exist there only), one child process per hook: big, small, big, small."""
    extra, caps = HOOKS[hook]
    env = dict(os.environ, VTX_LIB_VARIANT="dev")
    for k in ("VTX_BAND_DIAG2_MIN", "VTX_BAND_HARD_CAP", "VTX_BAND_LEGACY", "VTX_BAND_SLOTS", "VTX_DIAG_TAIL_CAP"):
        env.pop(k, None)
    env.update(extra)
    p = subprocess.run([sys.executable, "-c", RARE_CHILD, "caps" if caps else "exact"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    counts = json.loads(p.stdout.split("REUSE-COUNTS ")[1])
    print(hook, counts)
    if hook == "diag2":
        assert counts[1]["diag2_tasks"] > 0, counts[1]                     # the second stage ran on the small repeat-rich step
    if caps:
        assert counts[0]["overflow_tasks"] > 0 and counts[2]["overflow_tasks"] > 0, counts          # the general kernel took tasks on both big steps


def good_batches(n_barcodes):
    big = synth.make_batch(synth.SynthSpec(n_loci=120, n_barcodes=n_barcodes, reads_per_locus=40, indel_frac=0.4, read_len_jitter=40,
                                           sub_error=0.02, use_umi=True, seed=51))
    small = synth.make_batch(synth.SynthSpec(n_loci=6, n_barcodes=n_barcodes, reads_per_locus=7, use_umi=True, seed=52))
    return big, small


def test_failed_submits_leave_no_trace(tmp_path):
    """Between two good, different batches: a vtx_submit that fails validation, a vtx_submit_raw with tag bytes outside the arena, a
    vtx_submit_bam whose seed is not a record start, a vtx_submit_bam of a file with one flipped payload bit (CRC32).  All four are
    declines the suite exercises on fresh contexts; after each, vtx_run raises and the next good batch gives the fresh result."""
    import crc_util
    from test_host import make_dna_bam
    with crc_util.stored_blocks():
        bam = make_dna_bam(tmp_path, seed=7, n_reads=1500)
    inputs = dict(vcf=os.path.join(G, "test_dna.vcf"), bam=bam, fasta=os.path.join(G, "test_dna.fa"), cell_barcodes=os.path.join(G, "dna_barcodes.tsv"))
    raw_bytes = open(bam, "rb").read()
    with hostlib.plan_ingest(**inputs) as plan:
        assert plan.reason is None
        nb = len(plan.barcodes)
        cfg = default_config(aligner="banded", scoring_mode="coverage", use_umi=1, n_barcodes=nb)
        big, small = good_batches(nb)
        fresh = {id(b): RU.run_fresh(b, cfg) for b in (big, small)}
        raw, _ = synth.make_raw(small, nb, True, seed=4)
        a = plan.arrays()
        pb = a["blocks"]
        by_coff = {b["coff"]: b for b in crc_util.blocks_of(raw_bytes)}
        data_idx = [i for i in range(len(pb)) if pb["isize"][i]]
        damaged = bytearray(raw_bytes)
        crc_util.flip_stored_payload(damaged, by_coff[int(pb["coff"][data_idx[len(data_idx) // 2]])])
        damaged = np.frombuffer(bytes(damaged), np.uint8).copy()
        seeds = a["seeds"].copy()
        seeds[min(1, len(seeds) - 1)] += 1

        def bad_submit(ctx):
            bad = PackedBatch(big.loci.copy(), big.records.copy(), big.hap_arena, big.read_arena)
            bad.records["cell_index"][bad.n_records // 2] = nb + 7
            ctx.submit(bad)

        def bad_raw(ctx):
            bad = abi.RawBatch(raw.loci, raw.records.copy(), raw.hap_arena, raw.read_arena, raw.tag_arena)
            bad.records["bc_off"][3] = raw.tag_arena.size
            ctx.submit_raw(bad)

        def bad_seed(ctx):
            g = abi.VtxBamIngest.from_buffer_copy(plan.ingest)
            g.seeds = seeds.ctypes.data
            ctx.submit_bam(g, plan.n_loci)

        def bad_crc(ctx):
            g = abi.VtxBamIngest.from_buffer_copy(plan.ingest)
            g.file = damaged.ctypes.data
            ctx.submit_bam(g, plan.n_loci)
        failures = [("validation", bad_submit, abi.VTX_E_INVAL, "cell_index"), ("raw tags", bad_raw, abi.VTX_E_INVAL, ""),
                    ("seed", bad_seed, abi.VTX_E_UNSUPPORTED, ""), ("crc", bad_crc, abi.VTX_E_UNSUPPORTED, "CRC32")]
        with RU.open_context(cfg) as ctx:
            ctx.set_barcodes(plan.barcodes)
            before, after = big, small
            for what, call, status, word in failures:
                RU.check_step(ctx, before, cfg, fresh[id(before)], "before the failed %s submit" % what)
                with pytest.raises(lib.VtxError) as ei:
                    call(ctx)
                assert ei.value.status == status and word in str(ei.value), (what, ei.value)
                with pytest.raises(lib.VtxError) as ei:
                    ctx.run()                                                # nothing is resident: not the batch before, not a part of the failed one
                assert ei.value.status == abi.VTX_E_STATE, (what, ei.value)
                RU.assert_state_errors(ctx)
                RU.check_step(ctx, after, cfg, fresh[id(after)], "after the failed %s submit" % what)
                before, after = after, before


GATHER_CHILD = r'''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import reuse_util as RU
from vartrix_amd import lib
seq = RU.sequences()["unlike-banded-alt_frac-umi1"]
cfg = RU.config_of(seq)
steps = dict(seq["steps"])
with RU.open_context(cfg) as ctx:
    ctx.comm_init(lib.comm_id(), 0, 1)
    for label in ("1 noisy indels", "3 tiny clean", "5 mixed with long haplotypes", "4 empty", "7 edge cases"):
        batch = steps[label]
        ctx.submit(batch)
        ctx.run()
        got = RU.collect(ctx)
        RU.compare_with_oracle(got, batch, cfg, label)
        d = ctx.gather_coo(0)
        gathered = ctx.fetch_gathered()
        assert d["nnz"] == len(got["coo"]["row"]), (label, d["nnz"])
        for k in got["coo"]:
            assert np.array_equal(gathered[k].view(np.uint8), got["coo"][k].view(np.uint8)), (label, k)
        print(label, d["nnz"])
print("reuse-gather-ok")
''' % (ROOT, HERE)


def test_gather_on_reused_staging():
    """vtx_comm_init once (world 1), then vtx_gather_coo + vtx_fetch_gathered after batches of different sizes, alt_frac:
    values_from_counts_kernel writes the gathered values into staging that the larger batch before filled.  (A child process, as
    tests/test_gpu_shard.py runs its communicator.)"""
    p = subprocess.run([sys.executable, "-c", GATHER_CHILD], env=dict(os.environ), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "reuse-gather-ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_switching_submit_paths_on_one_context(tmp_path, monkeypatch):
    """Sequence (c), use_umi = 1, coverage, banded, ONE context: vtx_submit; vtx_set_barcodes + vtx_submit_raw; vtx_prefetch_file of a
    BAM, an unrelated vtx_submit, then vtx_submit_bam of that BAM (the prefetched bytes are still there and are used);
    vtx_submit_bam_segments of the sparse plan; a nibble batch, the same batch in bytes; vtx_submit_raw again WITHOUT another
    vtx_set_barcodes.  Every step equals the same step on a fresh context; submit and raw steps (and the BAM steps' resident records)
    are scored by the oracle; the BAM steps' raw records, loci, tag and read arenas and filter counters are the host packer's."""
    from oracle import prep
    import segments_util as su
    hostlib.use_variant("dev")                             # the planner's threshold knob: developer build of the host library only
    try:
        inputs = su.author(tmp_path, block=4000)
        kw = dict(use_umi=True)
        want, wmetrics, nv, barcodes, variants = hostlib.pack_files(raw=True, nibbles=True, threads=3, **inputs, **kw)
        monkeypatch.delenv("VTXH_SPARSE_KIB", raising=False)
        plan_c = hostlib.plan_ingest(**inputs, **kw)
        monkeypatch.setenv("VTXH_SPARSE_KIB", su.SPARSE_KIB)
        plan_s = hostlib.plan_ingest(**inputs, **kw)
        with plan_c, plan_s:
            assert plan_c.reason is None and plan_s.reason is None and (plan_c.kind, plan_s.kind) == ("contiguous", "segmented")
            assert plan_c.barcodes == barcodes == plan_s.barcodes
            _switching(inputs, want, wmetrics, barcodes, plan_c, plan_s, prep)
    finally:
        hostlib.use_variant("dev" if os.environ.get("VTX_LIB_VARIANT") == "dev" else "")


def _switching(inputs, want, wmetrics, barcodes, plan_c, plan_s, prep):
    nb = len(barcodes)
    cfg = default_config(aligner="banded", scoring_mode="coverage", use_umi=1, n_barcodes=nb)

    def spec(seed, **k):
        return synth.make_batch(synth.SynthSpec(**dict(dict(n_barcodes=nb, use_umi=True, seed=seed, sub_error=0.02), **k)))
    first = spec(61, n_loci=120, reads_per_locus=40, indel_frac=0.4, read_len_jitter=40)
    between = spec(63, n_loci=10, reads_per_locus=12)
    plain = spec(64, n_loci=80, reads_per_locus=24, indel_frac=0.2, read_len_jitter=0)
    nibbles = plain.to_nibbles()
    assert nibbles.read_format == abi.READS_NIBBLES and nibbles.read_arena.size * 2 >= plain.read_arena.size
    raw2 = RU.raw_over_barcodes(spec(62, n_loci=60, reads_per_locus=30, indel_frac=0.3, read_len_jitter=30), barcodes, True, seed=9)
    raw7 = RU.raw_over_barcodes(spec(65, n_loci=25, reads_per_locus=50, read_len_jitter=60), barcodes, True, seed=10)

    def ingest_arrays(c):
        return (c.debug_ingest(abi.INGEST_RAW_RECORDS, abi.RAW_RECORD_DTYPE), c.debug_ingest(abi.INGEST_RAW_LOCUS, np.uint32),
                c.debug_ingest(abi.INGEST_TAGS), c.debug_ingest(abi.INGEST_READS_PACKED))

    def fresh_of(do, bam=False):
        with RU.open_context(cfg) as c:
            c.set_barcodes(barcodes)
            st = do(c)
            arrays = ingest_arrays(c) if bam else None
            c.run()
            return RU.collect(c), st, arrays

    def finish(ctx, label):
        RU.assert_state_errors(ctx)
        ctx.run()
        got = RU.collect(ctx)
        print("%s: %d records, counts %s" % (label, ctx.n_records, got["counts"]))
        return got

    def raw_step(ctx, raw, label, set_list):
        """vtx_submit_raw: counters and prepared records against oracle/prep.py, every score and the triplets against the oracle."""
        def do(c):
            return c.submit_raw(raw)
        f, fst, _ = fresh_of(do)
        if set_list:
            ctx.set_barcodes(barcodes)
        st = do(ctx)
        got = finish(ctx, label)
        packed, wstats = prep.prep_raw(raw, barcodes, True)
        for s in (st, fst):
            assert (int(s.num_not_cell_bc), int(s.num_non_umi), int(s.kept)) == (wstats["num_not_cell_bc"], wstats["num_non_umi"], packed.n_records)
            assert s.hash_rounds >= 1 and s.num_not_cell_bc > 0 and s.num_non_umi > 0, label          # the lookups and the UMI grouping really ran
        for g in (got, f):
            assert prep.canonical_records(*g["records"]) == prep.canonical_records(packed.records, packed.loci["rec_begin"], packed.loci["rec_count"]), label
            RU.compare_with_oracle(g, RU.resident_batch(g["records"], raw.loci, raw.hap_arena, raw.read_arena, raw.read_format), cfg, label)
        RU.compare_with_fresh(got, f, label)
        assert np.array_equal(got["records"][0], f["records"][0]), label

    def bam_step(ctx, do, plan, label, prefetched):
        """A device ingest: everything the device built against the host packer's raw pack (tests/test_gpu_ingest.py's comparison),
        the run against the fresh context and the oracle."""
        f, fst, farr = fresh_of(do, bam=True)
        st = do(ctx)
        arr = ingest_arrays(ctx)
        got = finish(ctx, label)
        assert (st.prefetch_ms > 0) == prefetched and fst.prefetch_ms == 0, (label, st.prefetch_ms)
        wl = np.repeat(np.arange(want.n_loci, dtype=np.uint32), want.loci["rec_count"])
        for (raw, locus, tags, reads), s in ((arr, st), (farr, fst)):
            order = np.argsort(locus, kind="stable")
            assert np.array_equal(locus[order], wl) and np.array_equal(raw[order], want.records), label
            assert np.array_equal(tags, want.tag_arena) and np.array_equal(reads, want.read_arena), label
            m = dict(plan.metrics)
            m.update(num_reads=int(s.num_reads), num_low_mapq=int(s.num_low_mapq), num_non_primary=int(s.num_non_primary),
                     num_duplicates=int(s.num_duplicates), num_not_useful=int(s.num_not_useful), num_not_cell_bc=int(s.num_no_barcode_tag), num_non_umi=0)
            assert m == wmetrics, (label, m, wmetrics)
            assert int(s.raw_records) == want.n_records > 100
        assert (int(st.raw.num_not_cell_bc), int(st.raw.num_non_umi), int(st.raw.kept)) == (int(fst.raw.num_not_cell_bc), int(fst.raw.num_non_umi), int(fst.raw.kept))
        for g in (got, f):
            RU.compare_with_oracle(g, RU.resident_batch(g["records"], want.loci, want.hap_arena, want.read_arena, want.read_format), cfg, label)
        RU.compare_with_fresh(got, f, label)
        assert np.array_equal(got["records"][0], f["records"][0]), label
        return got

    fresh = {id(b): RU.run_fresh(b, cfg) for b in (first, between, plain, nibbles)}
    with RU.open_context(cfg) as ctx:
        RU.check_step(ctx, first, cfg, fresh[id(first)], "c1 submit")
        raw_step(ctx, raw2, "c2 set_barcodes + submit_raw", set_list=True)
        ctx.prefetch_file(inputs["bam"])
        RU.check_step(ctx, between, cfg, fresh[id(between)], "c3 an unrelated submit behind the prefetch")
        a = bam_step(ctx, lambda c: c.submit_bam(plan_c.ingest, plan_c.n_loci), plan_c, "c3 submit_bam of the prefetched file", True)
        b = bam_step(ctx, lambda c: c.submit_bam_segments(plan_s.segments, plan_s.n_loci), plan_s, "c4 submit_bam_segments", False)
        same_result(a, b)                                                  # (the two plans of one BAM prepare the same batch)
        ctx.set_read_format(abi.READS_NIBBLES)
        n = RU.check_step(ctx, nibbles, cfg, fresh[id(nibbles)], "c5 nibble submit", oracle_batch=plain)
        ctx.set_read_format(abi.READS_BYTES)
        p = RU.check_step(ctx, plain, cfg, fresh[id(plain)], "c6 byte submit")
        same_result(n, p)
        raw_step(ctx, raw7, "c7 submit_raw, the barcode list of step 2", set_list=False)
