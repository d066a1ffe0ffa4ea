"""band_diag_kernel against its launch (vtx_band.hip, vtxk_launch_band_diag).  Since round 21 the unit of work is a wavefront's block of
64 consecutive tasks, the workgroup is one wavefront, and the kernel has a second form in which a wavefront loops over blocks it claims
from one counter per XCD (the developer library's VTX_DIAG_CLAIM=1).  In that form a wavefront runs block after block
in the LDS the block before left behind, so the cases here send a few wavefronts round the loop dozens of times on batches that leave
every kind of stale state:

  * libvtx_dev.so, VTX_DIAG_CLAIM=1 and VTX_DIAG_GRID=n: grids of 1, 3 and 8 workgroups of 64 and of 256 threads on a batch of a few
    thousand tasks that mixes whole reads, repeat-rich loci (a full match list, a walk list that overflows), tasks for the tail and
    the recheck, a haplotype below six bases and empty reads;
  * more wavefronts than blocks: one block and seven blocks (fewer than the XCDs) under four-wavefront workgroups;
  * task counts of 64 k + 2 and 256 k - 2: the last block is partial, its idle lanes sit in a live wavefront;
  * a later chunk (VTX_BAND_CHUNK: task_base != 0, the counters zeroed again) and a second run on the same context;
  * a 250-base read: the build with four mask words;
  * the production library's own launch on more tasks than the device holds at once (300 k at 16 reads per locus).

Every case: every score equals the oracle's; on the developer library the stage bytes (vtx_fetch_stage) and vtx_timing's task counts
also equal those of the launch of rounds 3 - 20 on the same batch (VTX_DIAG_CLAIM=0, VTX_DIAG_WG=256: a workgroup per 256 tasks)."""
import os

import numpy as np
import pytest

from oracle import oracle
from vartrix_amd import synth
from vartrix_amd.abi import PackedBatch, default_config

import reuse_util as RU
import stress_batches as SB
import test_gpu_tables_grid as TG

pytestmark = pytest.mark.gpu
HOOKS = ("VTX_DIAG_CLAIM", "VTX_DIAG_WG", "VTX_DIAG_GRID", "VTX_BAND_CHUNK")
PARENT = dict(VTX_DIAG_CLAIM="0", VTX_DIAG_WG="256")


def cfg_of(nb):
    return default_config(aligner="banded", scoring_mode="coverage", n_barcodes=nb)


def run(batch, nb, variant=None, runs=1, **env):
    """What `runs` runs of one context leave (reuse_util.collect), the last one's; env: hooks of libvtx_dev.so, read at every launch."""
    assert not env or variant == "dev"
    for k in HOOKS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        with RU.open_context(cfg_of(nb), variant) as ctx:
            for _ in range(runs):
                ctx.submit(batch)
                ctx.run()
            return RU.collect(ctx)
    finally:
        for k in HOOKS:
            os.environ.pop(k, None)


_ref = {}            # name -> what the checks of a batch compare with, computed once and left alone


def reference(name, batch, nb, **env):
    """The oracle's scores, and the developer library's run with the launch of rounds 3 - 20 (env: the chunking hook of the case)."""
    if name not in _ref:
        _ref[name] = (oracle.batch_scores(batch, cfg_of(nb), threads=min(os.cpu_count() or 8, 16)), run(batch, nb, "dev", **PARENT, **env))
    return _ref[name]


def check(name, batch, nb, got, label, dev=True, **env):
    (oref, oalt), parent = reference(name, batch, nb, **env)
    bad = np.nonzero((got["ref"] != oref) | (got["alt"] != oalt))[0]
    assert bad.size == 0, "%s: %d records differ from the oracle, first %d" % (label, bad.size, bad[0])
    assert not (got["ref"] == RU.POISON).any() and not (got["alt"] == RU.POISON).any(), "%s: a score was never written" % label
    assert np.array_equal(parent["ref"], oref) and np.array_equal(parent["alt"], oalt), "%s: the launch of rounds 3 - 20, scores" % label
    if dev:
        RU.compare_with_fresh(got, parent, label)


def nb_of(batch):
    return int(batch.records["cell_index"].max()) + 1 if batch.n_records else 1


def _repeats(loci=30, reads=16, seed=77):
    """stress_batches.repeat_rich_batches with its reads kept within 192 bases: loci on a sequence of short tandem units, SNVs."""
    rng = np.random.default_rng(seed)
    units = [b"A", b"AC", b"AAT", b"ACGT", b"AAAAC", b"AG", b"T", b"CAG", b"ACACAT", b"GATTACA"]
    g = bytearray()
    while len(g) < 20000:
        g += units[int(rng.integers(0, len(units)))] * int(rng.integers(2, 40))
        g += bytes(rng.choice(list(b"ACGT"), int(rng.integers(0, 30))).tolist())
    g = bytes(g)
    haps, rds = [], []
    for _ in range(loci):
        p, pad = int(rng.integers(400, len(g) - 600)), int(rng.integers(30, 110))
        ref = g[p - pad:p + pad + 1]
        haps.append((ref, ref[:pad] + bytes([b"ACGT"[(b"ACGT".index(ref[pad:pad + 1]) + 1) % 4]]) + ref[pad + 1:]))
        rl = []
        for _k in range(reads):
            ln = int(rng.integers(40, 193))
            rd = bytearray(g[max(p - int(rng.integers(0, ln)), 0):][:ln])
            for e in np.nonzero(rng.random(len(rd)) < rng.choice([0.0, 0.02, 0.08]))[0]:
                rd[e] = b"ACGT"[int(rng.integers(0, 4))]
            rl.append((int(rng.integers(0, 30)), 0, bytes(rd)))
        rds.append(rl)
    return SB.manual_batch(haps, rds, 30)


def _mixed():
    """A few thousand tasks of every kind the kernel tells apart, haplotypes within 255 bases and reads within 192 (two-byte entries,
    three mask words): noisy indel reads (whole reads beside tasks for the tail, the recheck and the lists), repeat-rich loci and
    poly-A / tandem repeats (more than 40 off-diagonal matches; the walk list overflows), an ALT of three bases, empty reads."""
    noisy = synth.make_batch(synth.SynthSpec(n_loci=120, n_barcodes=100, reads_per_locus=12, indel_frac=0.5, read_len_jitter=50, seed=15,
                                             sub_error=0.03))
    rep = _repeats()
    batch = PackedBatch.concat([noisy.slice_loci(0, 60), rep, RU.low_complexity_batch(), TG._short_alt()[0], RU.edge_case_batch(),
                                noisy.slice_loci(60, noisy.n_loci)])
    assert int(np.maximum(batch.loci["ref_len"], batch.loci["alt_len"]).max()) <= 255 and int(batch.records["read_len"].max()) <= 192
    assert int(np.minimum(batch.loci["ref_len"], batch.loci["alt_len"]).min()) < 6 and int(batch.records["read_len"].min()) == 0
    assert 2 * batch.n_records >= 40 * 64                      # a grid of one wavefront goes round the loop 40 times and more
    return batch, nb_of(batch)


def _records(n):
    """Exactly n records (bench.py's generator with every read kept), 10 reads per locus and a last locus with the rest."""
    parts = [TG.exactly(n // 10, 10, 100)] if n >= 10 else []
    if n % 10:
        parts.append(TG.exactly(1, n % 10, 100))
    batch = PackedBatch.concat(parts)
    assert batch.n_records == n
    return batch, 100


def _long_reads():
    """Reads of up to 250 bases (the four-word build) on haplotypes within 255: a padding of 125 bases."""
    batch = synth.make_batch(synth.SynthSpec(n_loci=40, n_barcodes=100, reads_per_locus=12, read_len=250, padding=125, read_len_jitter=80,
                                             indel_frac=0.3, max_indel=4, sub_error=0.02, seed=21))
    assert 192 < int(batch.records["read_len"].max()) <= 250 and int(np.maximum(batch.loci["ref_len"], batch.loci["alt_len"]).max()) <= 255
    return batch, 100


@pytest.mark.parametrize("wg", [64, 256])
def test_a_few_wavefronts_take_every_block(wg):
    name = "mixed"
    batch, nb = _mixed()
    for grid in (1, 3, 8):
        got = run(batch, nb, "dev", VTX_DIAG_CLAIM="1", VTX_DIAG_WG=str(wg), VTX_DIAG_GRID=str(grid))
        check(name, batch, nb, got, "%s, %d workgroups of %d threads" % (name, grid, wg))
    parent = reference(name, batch, nb)[1]
    # the batch reaches what leaves stale state: tasks decided here, tasks for the sweep (repeats) and for the masked DP
    assert (parent["stage"] == 1).any() and parent["counts"]["swept_tasks"] > 0 and parent["counts"]["hard_tasks"] > 0, parent["counts"]


@pytest.mark.parametrize("n_tasks", [64, 7 * 64, 64 * 9 + 2, 256 * 3 - 2])
def test_blocks_fewer_than_wavefronts_and_partial_last_blocks(n_tasks):
    """64 and 448 tasks: one block, and seven (an XCD's eighth holds one block or none) — under four-wavefront workgroups some
    wavefronts find nothing.  578 and 766 tasks: a last block of 2 and of 62 tasks."""
    name = "%d tasks" % n_tasks
    batch, nb = _records(n_tasks // 2)
    for wg in (64, 256):
        check(name, batch, nb, run(batch, nb, "dev", VTX_DIAG_CLAIM="1", VTX_DIAG_WG=str(wg)), "%s, the loop's own grid, %d threads" % (name, wg))
        check(name, batch, nb, run(batch, nb, "dev", VTX_DIAG_CLAIM="0", VTX_DIAG_WG=str(wg)), "%s, no loop, %d threads" % (name, wg))
    check(name, batch, nb, run(batch, nb), "%s, production library" % name, dev=False)


def test_a_later_chunk_and_a_second_run():
    """Chunks of 1 024 tasks: task_base != 0 and the block counters zeroed per chunk; then the same batch again on the same context,
    where the counters hold the first run's end values until the launch zeroes them."""
    name = "mixed in chunks"
    batch, nb = _mixed()
    env = dict(VTX_BAND_CHUNK="1024")
    for wg in (64, 256):
        for runs in (1, 2):
            got = run(batch, nb, "dev", runs=runs, VTX_DIAG_CLAIM="1", VTX_DIAG_WG=str(wg), VTX_DIAG_GRID="3", **env)
            check(name, batch, nb, got, "%s, run %d, %d threads" % (name, runs, wg), **env)
    check(name, batch, nb, run(batch, nb, runs=2), "%s: second run, production library" % name, dev=False, **env)


def test_reads_of_250_bases_take_the_four_word_build():
    name = "250-base reads"
    batch, nb = _long_reads()
    for wg in (64, 256):
        got = run(batch, nb, "dev", VTX_DIAG_CLAIM="1", VTX_DIAG_WG=str(wg), VTX_DIAG_GRID="3")
        check(name, batch, nb, got, "%s, 3 workgroups of %d threads" % (name, wg))
        check(name, batch, nb, run(batch, nb, "dev", VTX_DIAG_CLAIM="0", VTX_DIAG_WG=str(wg)), "%s, no loop, %d threads" % (name, wg))
    check(name, batch, nb, run(batch, nb), "%s, production library" % name, dev=False)


def test_more_tasks_than_the_device_holds():
    """300 800 tasks at 16 reads per locus: 4 700 blocks against the 4 096 wavefronts the device holds at once.  The production
    library's own launch, and the developer library's loop on its own grid."""
    name = "9 400 loci x 16 reads"
    batch, nb = TG.exactly(9400, 16, 500), 500
    assert 2 * batch.n_records >= 300000
    check(name, batch, nb, run(batch, nb), "%s, production library" % name, dev=False)
    check(name, batch, nb, run(batch, nb, "dev", VTX_DIAG_CLAIM="1"), "%s, the loop's own grid" % name)
