"""band_diag_kernel addresses the read arena and the table buffer as a scalar base plus ONE 32-bit offset per lane (round 24;
vtx_fast_core.h, the loaders).  The offsets are unsigned and may use all 32 bits, so the batches here put reads and tables where an
offset taken as signed, or a sum that wraps, reads other bytes: above 2^31 and against the upper end of what the library accepts.
Every case runs the production library and the developer build and holds the scores to the oracle (computed once per batch, on a
copy of the batch with small offsets where the batch itself is large); stage bytes are held to the CPU build of the same header
(recheck_util.mirror, as tests/test_gpu_diag_round19.py does) where the mirror covers the batch: haplotypes of at most 255 bases.

  reads high     16 loci x 16 reads behind an unused prefix of the arena: every read_off above 2^31; and the same reads at the end of
                 the largest arena vtx_submit takes (0xffffffff bytes): the last read ends at the arena's last byte, its 16-byte loads
                 run into the padding beyond 2^32.  No access stayed in 64 bits for that: an access STARTS below read_off + read_len.
  tables high    300 000 loci x 1 read at padding 100: 4.1 GB of tables, those of the last 64 loci far above 2^31.  Their scores must be
                 those of the same loci submitted alone (slice_loci) and the oracle's.
  later chunk    300 loci in two chunks with a table buffer for 200 (gt_l0 != 0), equal to the run in one chunk
  instantiations four-byte entries (haplotypes of 301 bases), four mask words (reads of 230 bases), both, a three-base ALT beside an
                 ordinary REF, and a last wavefront of 2, 62 and 64 tasks — a record is two tasks, so a wavefront never ends on an odd one:
                 the 1 and 63 of a wavefront's first and last lane are not reachable through the API, 2 and 62 are the nearest."""
import os

import numpy as np
import pytest

import recheck_util as RU
import test_gpu_sweep as TS
from oracle import oracle
from stress_batches import manual_batch
from vartrix_amd import lib, synth
from vartrix_amd.abi import PackedBatch, default_config

pytestmark = pytest.mark.gpu
NB = 100
VARIANTS = [None, "dev"]
IDS = ["libvtx", "libvtx_dev"]
HOOKS = ("VTX_BAND_CHUNK", "VTX_BAND_GT_BYTES")
STAGE_DIAG_CERT, STAGE_DIAG_DP, STAGE_CORRIDOR_CERT = 1, 7, 11


def cfg():
    return default_config(aligner="banded", scoring_mode="coverage", n_barcodes=NB)


def run(batch, variant, **env):
    """(ref, alt, stage bytes) of one run on a fresh context; env: hooks of the developer build, read at every run"""
    assert not env or variant == "dev"
    for k in HOOKS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        with lib.Context(cfg(), variant=variant) as ctx:
            ctx.set_stage_trace(True)
            ctx.submit(batch)
            ctx.run()
            ref, alt = ctx.fetch_scores()
            return ref, alt, np.asarray(ctx.fetch_stage()).copy()
    finally:
        for k in HOOKS:
            os.environ.pop(k, None)


_oracle = {}


def want(name, batch):
    """the oracle's (ref, alt) of a batch, computed once"""
    if name not in _oracle:
        _oracle[name] = oracle.batch_scores(batch, cfg(), threads=8)
    return _oracle[name]


def same(got, exp, label):
    bad = np.nonzero((got[0] != exp[0]) | (got[1] != exp[1]))[0]
    assert len(bad) == 0, "%s: %d records differ; first: record %d: (%d, %d), expected (%d, %d)" % (
        label, len(bad), bad[0], got[0][bad[0]], got[1][bad[0]], exp[0][bad[0]], exp[1][bad[0]])


def exactly(n_loci, reads, **kw):
    """bench.py's generator with every read kept"""
    batch = synth.make_batch(synth.SynthSpec(n_loci=n_loci, n_barcodes=NB, reads_per_locus=reads, unlisted_frac=0.0, seed=2400 + n_loci + reads, **kw))
    assert batch.n_records == n_loci * reads
    return batch


# ---- reads high in the arena ----
def moved(batch, read_bytes, at):
    """the batch with an arena of read_bytes bytes, its reads from byte `at` on (the bytes in front are never looked at)"""
    n = batch.read_arena.size
    assert at + n <= read_bytes <= 0xffffffff
    arena = np.zeros(read_bytes, np.uint8)
    arena[at:at + n] = batch.read_arena
    recs = batch.records.copy()
    recs["read_off"] = (recs["read_off"].astype(np.uint64) + np.uint64(at)).astype(recs["read_off"].dtype)
    return PackedBatch(batch.loci, recs, batch.hap_arena, arena)


def _small_reads():
    return exactly(16, 16, read_len_jitter=40, sub_error=0.02)


def _above_2_31(small):
    return moved(small, (1 << 31) + 4097 + small.read_arena.size, (1 << 31) + 4097)          # (an odd offset: no read is aligned)


def _end_of_largest_arena(small):
    return moved(small, 0xffffffff, 0xffffffff - small.read_arena.size)


@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
@pytest.mark.parametrize("place", [_above_2_31, _end_of_largest_arena], ids=["above 2^31", "the end of the largest arena"])
def test_reads_high_in_the_arena(place, variant):
    small = _small_reads()
    big = place(small)
    off, ln = big.records["read_off"].astype(np.int64), big.records["read_len"].astype(np.int64)
    assert int(off.min()) > (1 << 31)
    if place is _end_of_largest_arena:
        assert big.read_arena.size == 0xffffffff and int((off + ln).max()) == 0xffffffff      # the last read ends at the arena's last byte
    ref, alt, stage = run(big, variant)
    same((ref, alt), want("reads", small), place.__name__)
    assert (np.isin(stage, (STAGE_DIAG_CERT, STAGE_CORRIDOR_CERT, STAGE_DIAG_DP))).mean() > 0.5, "band_diag_kernel decides most of these tasks"


# ---- tables high in the buffer ----
N_HIGH, LAST = 300_000, 64
_high = []


@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
def test_tables_high_in_the_buffer(variant):
    if not _high:
        _high.append(exactly(N_HIGH, 1))                       # (built once, left unchanged)
    batch = _high[0]
    tail = batch.slice_loci(N_HIGH - LAST, N_HIGH)
    with lib.Context(cfg(), variant=variant) as ctx:
        ctx.submit(tail)
        ctx.run()
        alone = ctx.fetch_scores()
        tables = ctx.debug_tables()
    assert len(tables) > 0 and len(tables) % (2 * LAST) == 0, "this shape keeps its tables in global memory"
    stride = len(tables) // (2 * LAST)
    assert int(batch.loci["ref_len"].max()) == int(tail.loci["ref_len"].max())               # (one table stride for both batches)
    first_of_last = (N_HIGH - LAST) * 2 * stride
    assert (1 << 31) < first_of_last and N_HIGH * 2 * stride <= (4 << 30) - 65536, "the whole batch in one table buffer, its end above 2^31"
    ref, alt, _ = run(batch, variant)
    r0 = int(batch.loci["rec_begin"][N_HIGH - LAST])
    exp = want("tables high, last loci", tail)
    same(alone, exp, "the last loci alone")
    same((ref[r0:], alt[r0:]), exp, "the last loci of the whole batch")
    # (and a sample of the loci on either side of 2^31: 64 loci around the table that crosses it)
    mid = (1 << 31) // (2 * stride)
    part = batch.slice_loci(mid - 32, mid + 32)
    m0 = int(batch.loci["rec_begin"][mid - 32])
    same((ref[m0:m0 + part.n_records], alt[m0:m0 + part.n_records]), want("tables high, across 2^31", part), "the loci across 2^31")


# ---- a later chunk: gt_l0 != 0 ----
def test_a_later_chunk():
    batch = exactly(300, 12)
    exp = want("chunks", batch)
    for variant in VARIANTS:
        same(run(batch, variant)[:2], exp, "one chunk, %s" % (variant or "production"))
    with lib.Context(cfg()) as ctx:
        ctx.submit(batch)
        ctx.run()
        stride = len(ctx.debug_tables()) // (2 * batch.n_loci)
    assert stride > 0
    # (the chunk hook alone rebuilds every table per chunk from locus 0; a table buffer for 200 of the 300 loci makes the second
    #  chunk's tables start at a later locus: tests/test_gpu_tables_grid.py::test_three_workgroups_on_a_later_chunk shows gt_l0 = 170)
    same(run(batch, "dev", VTX_BAND_CHUNK="4096", VTX_BAND_GT_BYTES=str(200 * 2 * stride))[:2], exp, "two chunks")


# ---- every instantiation of the kernel ----
def _stub_and_short_wavefront(last):
    """ordinary loci, one with an ALT of three bases (one lane of every pair never reaches a table), and as many records as leave the
    last wavefront `last` tasks"""
    rng = np.random.default_rng(24 + last)
    g = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 1400)].tolist())
    haps, reads = [], []
    n_rec = 64 + last // 2                                      # two full wavefronts and the last one
    per = [n_rec // 6 + (1 if i < n_rec % 6 else 0) for i in range(6)]
    for i in range(6):
        ref = g[200 * i:200 * i + 201]
        haps.append((ref, b"ACG" if i == 2 else ref[:100] + (b"T" if ref[100:101] != b"T" else b"G") + ref[101:]))
        reads.append([(k % NB, k, ref[(3 * k) % 50:(3 * k) % 50 + 150]) for k in range(per[i])])
    batch = manual_batch(haps, reads, NB)
    assert (2 * batch.n_records - 1) % 64 + 1 == last
    return batch


SHAPES = {
    "four-byte entries": lambda: exactly(8, 16, padding=150, sub_error=0.02),
    "four mask words": lambda: exactly(8, 16, read_len=230, padding=125, sub_error=0.02),
    "four-byte entries, four mask words": lambda: exactly(8, 16, read_len=230, padding=150, sub_error=0.02),
    "a three-base ALT, 2 tasks in the last wavefront": lambda: _stub_and_short_wavefront(2),
    "a three-base ALT, 62 tasks in the last wavefront": lambda: _stub_and_short_wavefront(62),
    "a three-base ALT, 64 tasks in the last wavefront": lambda: _stub_and_short_wavefront(64),
}
_mirror = {}


@pytest.fixture(scope="module")
def mirror_lib(tmp_path_factory):
    return RU.load_mirror(tmp_path_factory.mktemp("offsets32"))


@pytest.mark.parametrize("variant", VARIANTS, ids=IDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_instantiation(shape, variant, mirror_lib):
    batch = SHAPES[shape]()
    longest = max(int(batch.loci["ref_len"].max()), int(batch.loci["alt_len"].max()))
    assert (longest > 255) == shape.startswith("four-byte") and (int(batch.records["read_len"].max()) > 192) == ("four mask words" in shape)
    ref, alt, stage = run(batch, variant)
    same((ref, alt), want(shape, batch), shape)
    if shape not in _mirror:
        _mirror[shape] = RU.mirror(mirror_lib, batch)
    rc, score, why, route, _ = _mirror[shape]
    assert rc == (-1 if longest > 255 else 0)
    if rc != 0:
        return                                                  # (the mirror holds two-byte entries only: scores alone for these)
    got = np.empty(2 * batch.n_records, np.int64)
    got[0::2], got[1::2] = ref, alt
    decided, corridor, band = (route & RU.DECIDED) != 0, (route & RU.CORRIDOR) != 0, (route & RU.BAND) != 0
    exp = np.where(decided, STAGE_DIAG_CERT, np.where(corridor, STAGE_CORRIDOR_CERT, np.where(band, STAGE_DIAG_DP, 0)))
    known = exp != 0
    bad = np.nonzero(known & (stage != exp))[0]
    assert len(bad) == 0, "%d tasks decided elsewhere than the mirror says; first: task %d: stage %d, mirror %d (why %d)" % (
        len(bad), bad[0], stage[bad[0]], exp[bad[0]], why[bad[0]])
    left = ~known & (why != 1)                                  # (W_SHAPE: a haplotype below six bases, scored without a table)
    assert not np.isin(stage[left], (STAGE_DIAG_CERT, STAGE_CORRIDOR_CERT, STAGE_DIAG_DP)).any(), "the device decided a task the mirror leaves"
    fin = decided | corridor
    assert np.array_equal(got[fin], score[fin].astype(np.int64))
    assert known.any()
