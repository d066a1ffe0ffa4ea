"""Context reuse (include/vtx.h: "one vtx_ctx serves many batches"): sequences of UNLIKE batches for one context, and the check of one
step of such a sequence.

A reused context runs a batch inside buffers that only grow (DevBuf::reserve, vtx_api.hip) and therefore still hold the previous
batches' bytes: work lists, hard / pending / overflow lists, band slabs, k-mer tables, per-group counters, Matrix-Market staging.  A
fresh context cannot show a reset that is missing — new device memory mostly reads as zero and nothing larger ran before.  So every
step here is compared with the CPU oracle (scores of every record, the triplets, the DP cell count) and, for what the oracle does
not give (stage bytes, task counts, prepared records), with the same batch on a fresh context.

Plain helper module: tests/test_reuse_sequences.py (CPU) pins what the sequences contain, tests/test_gpu_context_reuse.py runs them."""
import os

import numpy as np

import stress_batches as SB
from audit_util import assert_stage_invariant
from oracle import oracle, prep
from vartrix_amd import abi, lib, synth
from vartrix_amd.abi import LOCUS_DTYPE, RECORD_DTYPE, PackedBatch, default_config

POISON = -4242
N_BARCODES = 200                            # every batch of a sequence keeps its cell indices below this
ROUND3_STAGES = (abi.STAGE_UNKNOWN, abi.STAGE_RUN_DP, abi.STAGE_GENERAL_DP)      # (0 = decided by band_run_kernel's certificate)
# vtx_timing's task counts.  All of them are compared with the fresh context's on the production library: each is a count of tasks
# with a property of the task (list lengths read back after the kernels finished), none depends on the order of the atomics that
# built the lists.
# (resweep_tasks is not listed: nothing sets it since round 4's sweep kernel left the developer library, last in commit 5c0dd06; it is always 0.)
TASK_COUNTS = ("hard_tasks", "overflow_tasks", "diag_left", "checked_tasks", "swept_tasks", "diag2_tasks", "diag2_scored", "diag2_streamed")
COO_INT = ("row", "col", "alt", "ref", "unk")


# ---- the generators of tests/test_gpu_shape.py (moved here; it imports them) ----
def long_loci_batch(n, seed, reads=64, max_indel=90, n_barcodes=5000):
    """n loci whose REF or ALT haplotype exceeds 255 bases: indels of 56 .. max_indel bases at padding 100."""
    spec = synth.SynthSpec(n_loci=4 * n + 8, n_barcodes=n_barcodes, reads_per_locus=reads, indel_frac=1.0, max_indel=max_indel, seed=seed)
    b = synth.make_batch(spec)
    long_ = np.nonzero(np.maximum(b.loci["ref_len"], b.loci["alt_len"]) > 255)[0][:n]
    assert len(long_) == n
    return [b.slice_loci(int(l), int(l) + 1) for l in long_]


def mixed_batch(n_loci, positions, reads=64, seed=11, n_barcodes=5000):
    base = synth.make_batch(synth.SynthSpec(n_loci=n_loci, n_barcodes=n_barcodes, reads_per_locus=reads, seed=seed))
    longs = long_loci_batch(len(positions), seed + 1, reads, n_barcodes=n_barcodes)
    parts, prev = [], 0
    for pos, lb in zip(positions, longs):
        parts += [base.slice_loci(prev, pos), lb]
        prev = pos
    parts.append(base.slice_loci(prev, n_loci))
    out = PackedBatch.concat(parts)
    is_long = np.maximum(out.loci["ref_len"], out.loci["alt_len"]) > 255
    assert int(is_long.sum()) == len(positions)
    return out, is_long


# ---- batches restated from the tests that introduced them (same seeds, same bytes) ----
def low_complexity_batch():
    """tests/test_gpu_parity.py::test_banded_low_complexity_overflow_slabs: poly-A / tandem-repeat reads on repeat-rich haplotypes."""
    rng = np.random.default_rng(99)
    haps, reads = [], []
    for i in range(6):
        flank = bytes(rng.choice(list(b"ACGT"), 80).tolist())
        rep = [b"A" * 60, b"AC" * 30, b"AAAAAT" * 10, b"A" * 25 + b"G" + b"A" * 34, b"ACG" * 20, b"T" * 60][i]
        ref = flank + rep + flank[::-1]
        alt = flank + rep[:30] + b"C" + rep[31:] + flank[::-1]
        haps.append((ref, alt))
        rl = []
        for k in range(10):
            o = int(rng.integers(0, 60))
            rd = bytearray((flank + rep + flank[::-1])[o:o + 150])
            if k % 3 == 0:
                rd = bytearray(b"A" * 150) if i % 2 == 0 else bytearray((b"AC" * 75))
            rl.append((k % 5, 0, bytes(rd)))
        reads.append(rl)
    return SB.manual_batch(haps, reads, 8)


def beyond_limits_batch():
    """tests/test_gpu_parity.py::test_records_beyond_the_fast_limits_take_the_exact_slow_path: a 3 000-base read, haplotypes of
    2 600 / 5 400 bases, ordinary records around them."""
    rng = np.random.default_rng(41)
    g = bytes(rng.choice(list(b"ACGT"), 12000).tolist())

    def mutate(seq, n):
        b = bytearray(seq)
        for _ in range(n):
            b[int(rng.integers(0, len(b)))] = b"ACGT"[int(rng.integers(0, 4))]
        return bytes(b)
    ins = bytes(rng.choice(list(b"ACGT"), 2800).tolist())
    haps = [
        (g[100:301], g[100:200] + b"T" + g[201:301]),
        (g[1000:3600], g[1000:2300] + ins + g[2300:3600]),
        (g[5000:5201], g[5000:5100] + b"G" + g[5101:5201]),
        (g[7000:7201], g[7000:7100] + g[7108:7201]),
    ]
    reads = [
        [(0, 0, g[120:270]), (1, 0, mutate(g[130:280], 2)), (2, 0, g[100:200] + b"T" + g[201:260])],
        [(0, 0, g[2200:2350]), (1, 0, g[2250:2300] + ins[:100]), (2, 0, mutate(g[1000:2300] + ins[:700], 12)),
         (3, 0, ins[2700:] + g[2300:2400]), (4, 0, b"ACG")],
        [(0, 0, g[5050:5200]), (1, 0, mutate(g[4000:5100] + b"G" + g[5101:7000], 25)), (2, 0, g[5090:5101] + b"G" + g[5101:5160])],
        [(0, 0, g[7010:7160]), (0, 1, g[7020:7100] + g[7108:7180])],
    ]
    return SB.manual_batch(haps, reads, 8)


def edge_case_batch():
    """tests/test_gpu_parity.py::test_edge_cases: a locus without reads, empty reads, N / lower-case bytes, ties, sub-threshold reads,
    a cell with only None calls."""
    rng = np.random.default_rng(3)
    g = bytes(rng.choice(list(b"ACGT"), 400).tolist())
    ref = g[100:301]
    alt = g[100:200] + b"t" + g[201:301]
    altn = g[100:200] + b"N" + g[201:301]
    haps = [(ref, alt), (ref, altn), (ref, ref), (g[0:50], g[0:20] + g[30:50]), (ref, alt)]
    reads = [
        [(0, 0, g[120:270]), (0, 0, g[150:300]), (1, 0, b""), (2, 5, b"ACGT"), (3, 1, g[190:215])],
        [(0, 0, g[120:200] + b"N" + g[201:270]), (0, 1, g[120:270]), (7, 0, b"N" * 60)],
        [(4, 0, g[130:280]), (4, 0, g[131:281])],
        [(1, 0, g[0:50]), (2, 0, g[0:20] + g[30:50]), (5, 0, g[5:45])],
        [],
    ]
    return SB.manual_batch(haps, reads, 8)


def empty_batch():
    return PackedBatch(np.zeros(0, LOCUS_DTYPE), np.zeros(0, RECORD_DTYPE), np.zeros(0, np.uint8), np.zeros(0, np.uint8))


def noisy_indel_batch(banded, umi):
    """Step 1.  Banded: the spec of tests/test_gpu_parity.py::test_banded_differs_from_full_and_device_follows_the_band (hard_tasks > 0
    there); full: 5 % substitution errors on top of the indels."""
    if banded:
        return synth.make_batch(synth.SynthSpec(n_loci=256, n_barcodes=N_BARCODES, reads_per_locus=48, indel_frac=0.6, read_len_jitter=60,
                                                seed=23, sub_error=0.02, use_umi=bool(umi)))
    return synth.make_batch(synth.SynthSpec(n_loci=256, n_barcodes=N_BARCODES, reads_per_locus=48, indel_frac=0.5, read_len_jitter=60,
                                            seed=29, sub_error=0.05, use_umi=bool(umi)))


MIXED_LOCI, MIXED_POSITIONS = 300, (0, 150, 300)          # long-haplotype loci first, in the middle and last


def unlike_steps(banded, umi):
    """Sequence (a): each step runs in buffers that a DIFFERENT predecessor dirtied.  [(label, batch)]; steps that repeat an earlier
    one hold the same batch object."""
    noisy = noisy_indel_batch(banded, umi)
    tiny = synth.make_batch(synth.SynthSpec(n_loci=4, n_barcodes=N_BARCODES, reads_per_locus=5, seed=3, use_umi=bool(umi)))
    repeat = next(iter(SB.repeat_rich_batches(trials=1, loci=40, reads=24, pad_range=(30, 110))))[1]       # (every haplotype within 255 bases: the sweep path)
    mixed, _ = mixed_batch(MIXED_LOCI, list(MIXED_POSITIONS), reads=24, seed=17, n_barcodes=N_BARCODES)
    return [("1 noisy indels", noisy), ("2a repeat-rich", repeat), ("2b poly-A / tandem", low_complexity_batch()), ("3 tiny clean", tiny),
            ("4 empty", empty_batch()), ("5 mixed with long haplotypes", mixed), ("6 beyond the fast limits", beyond_limits_batch()),
            ("7 edge cases", edge_case_batch()), ("8 tiny clean again", tiny), ("9 noisy indels again", noisy)]


def rare_path_steps():
    """Sequence (b): big, small, big, small for the developer library's hooks.  The big batches mix noisy indel loci (the batch of
    tests/test_gpu_parity.py::test_band_buffer_caps_spill_into_the_general_kernel), tandem repeats and the adversarial "edges"
    family (bytes outside ACGTN: declined by the sweep); the first small one is repeat-rich (material for the second stage)."""
    noisy = synth.make_batch(synth.SynthSpec(n_loci=150, n_barcodes=100, reads_per_locus=48, indel_frac=0.5, read_len_jitter=50, seed=15,
                                             sub_error=0.03))
    reps = [b for _, b, _ in SB.repeat_rich_batches(trials=2, loci=30, reads=16, pad_range=(30, 120), seed=77)]
    edges = SB.adversarial_batch(60, 32, 31337, ("edges", "repeats"), n_barcodes=100)
    big1 = PackedBatch.concat([noisy, reps[0], edges])
    big2 = PackedBatch.concat([reps[1], noisy.slice_loci(0, 100)])
    small = next(iter(SB.repeat_rich_batches(trials=1, loci=10, reads=10, pad_range=(30, 110), seed=5)))[1]     # (within 255 bases: the second stage takes it)
    tiny = synth.make_batch(synth.SynthSpec(n_loci=4, n_barcodes=100, reads_per_locus=5, seed=3))
    return [("big 1", big1), ("small repeat-rich", small), ("big 2", big2), ("tiny clean", tiny)]


def sequences():
    """name -> dict(aligner, mode, umi, n_barcodes, steps=[(label, batch)]).  Seeded: the same bytes in every process."""
    out = {}
    for aligner, mode, umi in (("banded", "coverage", 0), ("banded", "alt_frac", 1), ("full", "consensus", 0)):
        out["unlike-%s-%s-umi%d" % (aligner, mode, umi)] = dict(aligner=aligner, mode=mode, umi=umi, n_barcodes=N_BARCODES,
                                                                  steps=unlike_steps(aligner == "banded", umi))
    out["rare-paths"] = dict(aligner="banded", mode="coverage", umi=0, n_barcodes=100, steps=rare_path_steps())
    return out


def config_of(seq, aligner=None):
    return default_config(aligner=aligner or seq["aligner"], scoring_mode=seq["mode"], use_umi=seq["umi"], n_barcodes=seq["n_barcodes"])


def validate_packed(batch, n_barcodes):
    """vtx_submit's checks (vtx_api.hip, prep_check_kernel), restated: loci cover the records contiguously, everything lies inside its
    arena, cell indices fit, records are sorted by (cell, UMI) inside their locus."""
    L, R = batch.loci, batch.records
    begin = np.concatenate([[0], np.cumsum(L["rec_count"], dtype=np.int64)])
    assert np.array_equal(L["rec_begin"], begin[:-1]) and begin[-1] == batch.n_records
    for k in ("ref", "alt"):
        assert np.all(L[k + "_off"].astype(np.int64) + L[k + "_len"] <= batch.hap_arena.size)
    assert np.all(R["read_off"].astype(np.int64) + R["read_len"] <= batch.read_arena.size)
    assert batch.n_records == 0 or int(R["cell_index"].max()) < n_barcodes
    locus = np.repeat(np.arange(batch.n_loci), L["rec_count"])
    key = R["cell_index"].astype(np.int64) << 32 | R["umi_id"]
    same = locus[1:] == locus[:-1]
    assert np.all(key[1:][same] >= key[:-1][same])


# ---- the oracle, once per batch ----
_scores = {}             # (id(batch), aligner) -> (batch, (ref, alt)); the batch is held so that its id stays its own
_oracle = {}             # (id(batch), aligner, mode, umi, n_barcodes) -> (batch, dict)


def oracle_of(batch, cfg):
    """dict(ref, alt, coo, cells, full=(ref, alt) of the full flavour for a banded cfg) — cached per batch object and configuration."""
    key = (id(batch), cfg.aligner, cfg.scoring_mode, cfg.use_umi, cfg.n_barcodes)
    if key not in _oracle:
        threads = min(os.cpu_count() or 8, 16)

        def scores(aligner):
            k = (id(batch), aligner)
            if k not in _scores:
                _scores[k] = (batch, oracle.batch_scores(batch, default_config(aligner=aligner, n_barcodes=cfg.n_barcodes), threads=threads))
            return _scores[k][1]
        r, a = scores(cfg.aligner)
        out = dict(ref=r, alt=a, coo=oracle.batch_reduce(batch, cfg, r, a))
        if cfg.aligner == abi.ALIGNER_BANDED:
            out["full"] = scores(abi.ALIGNER_FULL)
        # (vtx_last_cells is the prepared batch's rows x columns in both flavours, vtx_submit's cnt[3]: the oracle's full-matrix count)
        out["cells"] = oracle.batch_cells(batch, default_config(aligner="full", n_barcodes=cfg.n_barcodes))
        _oracle[key] = (batch, out)
    return _oracle[key][1]


def open_context(cfg, variant=None):
    ctx = lib.Context(cfg, variant=variant)
    ctx.set_stage_trace(True)
    ctx.set_poison(POISON)
    return ctx


def collect(ctx):
    """Everything a completed run leaves, as host arrays."""
    r, a = ctx.fetch_scores()
    t = ctx.timing()
    recs, begin, count = ctx.fetch_records()
    return dict(ref=r, alt=a, coo=ctx.fetch_coo(), cells=ctx.cells(), stage=ctx.fetch_stage(),
                counts={k: int(getattr(t, k)) for k in TASK_COUNTS}, records=(recs, begin, count))


def run_fresh(batch, cfg, variant=None):
    with open_context(cfg, variant) as ctx:
        ctx.submit(batch)
        ctx.run()
        return collect(ctx)


def assert_state_errors(ctx):
    """Between a submit and its run nothing of the previous batch is readable."""
    for name in ("fetch_scores", "fetch_coo", "device_coo", "timing", "cells"):
        try:
            getattr(ctx, name)()
        except lib.VtxError as e:
            assert e.status == abi.VTX_E_STATE, "%s after submit: %s" % (name, e)
        else:
            raise AssertionError("%s after a submit and before its run returned the previous batch's result" % name)


def compare_with_oracle(got, batch, cfg, label):
    want = oracle_of(batch, cfg)
    r, a = got["ref"], got["alt"]
    assert r.shape == want["ref"].shape
    bad = np.nonzero((r != want["ref"]) | (a != want["alt"]))[0]
    assert bad.size == 0, "%s: %d records differ from the oracle, first %d: device (%d, %d) oracle (%d, %d), stages %s" % (
        label, bad.size, bad[0], r[bad[0]], a[bad[0]], want["ref"][bad[0]], want["alt"][bad[0]], got["stage"][2 * bad[0]:2 * bad[0] + 2])
    for k in COO_INT:
        assert np.array_equal(got["coo"][k], want["coo"][k]), "%s: COO field %s" % (label, k)
    for k in ("value", "ref_value"):        # bit patterns: alt_frac holds NaN (0 / 0)
        assert np.array_equal(got["coo"][k].view(np.uint64), want["coo"][k].view(np.uint64)), "%s: COO field %s" % (label, k)
    assert got["cells"] == want["cells"], "%s: cells %d, oracle %d" % (label, got["cells"], want["cells"])
    assert not (r == POISON).any() and not (a == POISON).any(), "%s: a score was never written" % label
    if cfg.aligner == abi.ALIGNER_BANDED:
        assert_stage_invariant(got["stage"], (r, a), want["full"], label)
    else:
        assert np.isin(got["stage"], (abi.STAGE_FULL_DP, abi.STAGE_SLOW)).all(), label      # (the slow path marks its records in both flavours)


def compare_with_fresh(got, fresh, label, stage_equal=True, counts=TASK_COUNTS):
    if stage_equal:
        ne = np.nonzero(got["stage"] != fresh["stage"])[0]
        assert ne.size == 0, "%s: %d stage bytes differ from the fresh context's, first task %d: %d vs %d" % (
            label, ne.size, ne[0], got["stage"][ne[0]], fresh["stage"][ne[0]])
    for k in counts:
        assert got["counts"][k] == fresh["counts"][k], "%s: vtx_timing.%s is %d, on a fresh context %d" % (label, k, got["counts"][k], fresh["counts"][k])
    assert got["cells"] == fresh["cells"], label
    assert prep.canonical_records(*got["records"]) == prep.canonical_records(*fresh["records"]), "%s: prepared records" % label


def check_step(ctx, batch, cfg, fresh, label="", stage_equal=True, counts=TASK_COUNTS, oracle_batch=None):
    """One step on the reused context `ctx` (poison and stage trace on: open_context): submit, the state errors, run, then every
    score, the triplets (values bit for bit) and the cell count against the CPU oracle, the stage invariant on a banded step, and
    stage bytes / task counts / prepared records against `fresh`, the same step's run_fresh.  oracle_batch: the batch the oracle reads
    when `batch` holds its reads as nibbles (the same batch, one byte per base).  Returns what the step produced."""
    ctx.submit(batch)
    assert_state_errors(ctx)
    ctx.run()
    got = collect(ctx)
    print("%s: %d records, counts %s" % (label, batch.n_records, got["counts"]))
    ob = batch if oracle_batch is None else oracle_batch
    compare_with_oracle(fresh, ob, cfg, label + " (fresh context)")
    compare_with_oracle(got, ob, cfg, label)
    compare_with_fresh(got, fresh, label, stage_equal, counts)
    assert prep.canonical_records(*got["records"]) == prep.canonical_records(batch.records, batch.loci["rec_begin"], batch.loci["rec_count"]), label
    return got


# ---- switching submit paths (sequence c) ----
def raw_over_barcodes(batch, barcodes, use_umi, seed):
    """synth.make_raw's raw form of `batch` (tag bytes, records shuffled inside their locus, extra records with an unlisted barcode
    or without a UB tag) with the listed barcodes' bytes replaced by those of `barcodes` (18 bytes each, as make_raw's own): a raw
    batch for a context whose barcode list came from somewhere else (a BAM's barcode file)."""
    raw, own = synth.make_raw(batch, len(barcodes), use_umi, seed=seed)
    theirs = [b if isinstance(b, bytes) else b.encode() for b in barcodes]
    assert len(own) == len(theirs) and all(len(b) == 18 for b in theirs) and len(set(theirs)) == len(theirs)
    index = {b: i for i, b in enumerate(own)}
    tags = raw.tag_arena.reshape(-1, 28).copy()
    for k in np.nonzero(raw.records["bc_len"] == 18)[0]:
        tags[k, :18] = np.frombuffer(theirs[index[bytes(tags[k, :18])]], np.uint8)
    return abi.RawBatch(raw.loci, raw.records, raw.hap_arena, raw.read_arena, tags.reshape(-1))


def resident_batch(records, loci, hap_arena, read_arena, read_format=0):
    """The batch a context holds after vtx_submit_raw / vtx_submit_bam, as a PackedBatch the oracle can score: the device's own
    prepared records (vtx_fetch_records) over the arenas that were submitted, one byte per base."""
    recs, begin, count = records
    lc = np.array(loci, LOCUS_DTYPE, copy=True)
    lc["rec_begin"], lc["rec_count"] = begin, count
    return PackedBatch(lc, recs, hap_arena, read_arena, read_format).to_bytes()
