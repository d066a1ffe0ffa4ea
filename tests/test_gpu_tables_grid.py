"""band_tables_kernel against its grid (vtx_band.hip, launch_band_tables).  The kernel loops over the tables with stride gridDim.x;
until round 17 the launch capped the grid at 8 192 one-wavefront workgroups and no test ever sent a workgroup round that loop a
second time (at most 400 tables).  The launch now gives every table a workgroup of its own (the fastest of the grids measured,
DESIGN.md 4.3.2) and the developer library takes any grid, so both ends are pinned here:

  * libvtx_dev.so, VTX_BAND_TABLES_GRID=n: grids of 1, 3 and 8 workgroups (one workgroup builds up to 86 tables in sequence, in the
    LDS the table before left behind), exactly one workgroup per table, and one more than that (a workgroup without a table);
  * the production library's own grid on 9 000 tables, more than the device holds at once with and without t3[] and more than the
    8 192 of the earlier cap;
  * a context that ran the 9 000 tables and then a batch of 74.

Every case: the defined bytes of the tables (vtx_debug_tables) equal round 3's kernel (VTX_BAND_TABLES_V1=1 in libvtx_dev.so, a locus
per wavefront, no loop over tables of its own design), and every score equals the oracle's."""
import os

import numpy as np
import pytest

from oracle import oracle
from vartrix_amd import synth
from vartrix_amd.abi import PackedBatch, default_config

import stress_batches as SB
import test_gpu_sweep as TS
from reuse_util import mixed_batch

pytestmark = pytest.mark.gpu
HOOKS = ("VTX_BAND_TABLES_GRID", "VTX_BAND_TABLES_V1", "VTX_BAND_CHUNK", "VTX_BAND_GT_BYTES")


def run(batch, nb, variant=None, **env):
    """(tables, (ref, alt)) of one run on a fresh context; env: hooks of libvtx_dev.so, read at every launch."""
    assert not env or variant == "dev"
    for k in HOOKS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return TS._tables_and_scores(batch, nb, variant=variant)
    finally:
        for k in HOOKS:
            os.environ.pop(k, None)


_ref = {}            # name -> what the checks of a batch compare with, computed once and left alone


def reference(name, batch, nb, loci=None, **env):
    """Round 3's tables (their defined bytes) and the oracle's scores.  loci: the loci whose tables the dump holds and that mean
    something (default: all of the batch); env: the chunking hooks of the case, the same for both kernels."""
    if name not in _ref:
        tables, scores = run(batch, nb, "dev", VTX_BAND_TABLES_V1="1", **env)
        assert len(tables) > 0, "%s: this shape keeps its tables in LDS" % name
        _ref[name] = (defined(tables, batch, loci), scores,
                      oracle.batch_scores(batch, default_config(aligner="banded", n_barcodes=nb), threads=min(os.cpu_count() or 8, 16)))
    return _ref[name]


def defined(tables, batch, loci=None):
    """tests/test_gpu_sweep.py's _defined_bytes; loci = (first locus of the dump, the loci to look at): the tables of those loci only."""
    if loci is None:
        return TS._defined_bytes(tables, batch)
    first, keep = loci
    n_dump = batch.n_loci - first                           # (every dump of these tests ends with the batch's last locus)
    assert len(tables) % (2 * n_dump) == 0
    stride = len(tables) // (2 * n_dump)
    sub = PackedBatch.concat([batch.slice_loci(int(l), int(l) + 1) for l in keep])
    picked = np.concatenate([tables[2 * (int(l) - first) * stride:2 * (int(l) - first + 1) * stride] for l in keep])
    assert TS._uses_t3(sub) == TS._uses_t3(batch)
    return TS._defined_bytes(picked, sub)


def check(name, batch, nb, got, label, loci=None, **env):
    want_tables, want_scores, (oref, oalt) = reference(name, batch, nb, loci, **env)
    tables, (r, a) = got
    d = defined(tables, batch, loci)
    assert len(d) == len(want_tables), label
    assert np.array_equal(d, want_tables), "%s: tables differ from round 3's (%d of %d defined bytes)" % (label, int((d != want_tables).sum()), len(d))
    assert np.array_equal(r, oref) and np.array_equal(a, oalt), "%s: %d records differ from the oracle" % (label, int(((r != oref) | (a != oalt)).sum()))
    assert np.array_equal(want_scores[0], oref) and np.array_equal(want_scores[1], oalt), "%s: round 3's tables, scores" % label


def exactly(n_loci, reads, nb):
    """bench.py's generator with every read kept (by default it drops the 5 % whose barcode is not listed: 8 reads drawn would be
    15 tasks per locus, below t3[]'s threshold of 16)."""
    batch = synth.make_batch(synth.SynthSpec(n_loci=n_loci, n_barcodes=nb, reads_per_locus=reads, unlisted_frac=0.0, seed=1000 * n_loci + reads))
    assert batch.n_records == n_loci * reads
    return batch


def _shallow():
    return exactly(37, 6, 100), 100, None


def _deep():
    return exactly(40, 12, 100), 100, None


def _repeated_units():
    """The haplotypes of tests/test_gpu_sweep.py::test_table_kernel_against_round3s: one repeated unit (a bucket with many k-mers in
    one round of 64 positions: as many trips of the link), a byte above 0x7f (no uniqueness flags, no twin list)."""
    haps = [(b"A" * 201, b"A" * 100 + b"C" + b"A" * 100), (b"AC" * 100 + b"A", b"AC" * 50 + b"T" + b"AC" * 50),
            (b"ACG" * 67, b"ACG" * 33 + b"T" + b"ACG" * 33), (b"ACGTN" * 5 + b"\x90" + b"ACGGT" * 20, b"ACGTTGCA" * 12)]
    return SB.manual_batch(haps, [[(0, 0, h[0][20:170])] * 4 for h in haps], 10), 10, None


def _short_alt():
    """An ALT of three bases (a deletion that leaves less than one 6-mer: nk = 0, no round of the link, of the flags or of the tags)
    between ordinary loci: the table after it is built in LDS that a table without entries left."""
    rng = np.random.default_rng(3)
    g = bytes(rng.choice(list(b"ACGT"), 1400).tolist())
    haps, reads = [], []
    for i in range(6):
        ref = g[200 * i:200 * i + 201]
        haps.append((ref, b"ACG" if i == 2 else ref[:100] + (b"T" if ref[100:101] != b"T" else b"G") + ref[101:]))
        reads.append([(k, 0, ref[8 * k:8 * k + 150]) for k in range(6)])
    return SB.manual_batch(haps, reads, 10), 10, None


def _long_and_short():
    """Three loci with a haplotype above 255 bases among 40 ordinary ones: two passes (tests/test_gpu_shape.py).  The first builds the
    tables of the short loci and an empty one (hn = 0) for each long locus; the second leaves every short locus out, by the
    `continue` at the top of the loop.  The dump is the second pass': first to last long locus = the whole batch, long loci defined."""
    batch, is_long = mixed_batch(40, [0, 20, 40], reads=12, seed=5, n_barcodes=200)
    assert is_long[0] and is_long[-1]
    return batch, 200, (0, np.nonzero(is_long)[0])


CASES = {"37 loci x 6 reads": _shallow, "40 loci x 12 reads (t3[])": _deep, "repeated units, a byte above 0x7f": _repeated_units,
         "an ALT of three bases": _short_alt, "haplotypes above 255 bases among shorter ones": _long_and_short}


@pytest.mark.parametrize("name", list(CASES))
def test_any_grid_leaves_the_same_tables(name):
    batch, nb, loci = CASES[name]()
    assert TS._uses_t3(batch) == (name in ("40 loci x 12 reads (t3[])", "haplotypes above 255 bases among shorter ones"))
    n = batch.n_loci
    for grid in (1, 3, 8, 2 * n, 2 * n + 1):
        check(name, batch, nb, run(batch, nb, "dev", VTX_BAND_TABLES_GRID=str(grid)), "%s, grid %d" % (name, grid), loci)
    check(name, batch, nb, run(batch, nb), "%s, production library" % name, loci)


def test_three_workgroups_on_a_later_chunk():
    """VTX_BAND_CHUNK=4096 and a table buffer for 200 of the 300 loci (VTX_BAND_GT_BYTES; the chunk hook alone rebuilds every table
    per chunk from locus 0): the second chunk's tables are those of loci 170 .. 299, gt_l0 = 170, built by three workgroups."""
    name = "300 loci x 12 reads in two chunks"
    batch = exactly(300, 12, 100)
    whole, _ = run(batch, 100)
    stride = len(whole) // (2 * batch.n_loci)
    env = dict(VTX_BAND_CHUNK="4096", VTX_BAND_GT_BYTES=str(200 * 2 * stride))
    tables, scores = run(batch, 100, "dev", VTX_BAND_TABLES_GRID="3", **env)
    n_dump = len(tables) // (2 * stride)
    assert len(tables) == n_dump * 2 * stride and 0 < n_dump < 200, n_dump
    first = batch.n_loci - n_dump
    assert first > 0                                           # gt_l0 != 0
    loci = (first, np.arange(first, batch.n_loci))
    check(name, batch, 100, (tables, scores), name, loci, **env)
    # the same loci's tables in the dump of the whole batch, default grid
    assert np.array_equal(defined(tables, batch, loci), defined(whole[2 * first * stride:], batch, loci))


def _many(reads):
    return exactly(4500, reads, 500), 500


@pytest.mark.parametrize("reads", [2, 8])
def test_more_tables_than_the_device_holds(reads):
    """9 000 tables: the device holds 22 workgroups per CU with t3[] (8 reads: 16 tasks per locus) and 30 without — 5 632 / 7 680 on
    256 CUs.  The production library's own grid (9 000 workgroups: most of them wait for a place), and the developer library on
    what the device holds at once (some workgroups build two tables and some one) and on the 8 192 of rounds 4 - 16."""
    batch, nb = _many(reads)
    assert TS._uses_t3(batch) == (reads == 8)
    name = "4 500 loci x %d reads" % reads
    check(name, batch, nb, run(batch, nb), name)
    for grid in (5632 if reads == 8 else 7680, 8192):
        check(name, batch, nb, run(batch, nb, "dev", VTX_BAND_TABLES_GRID=str(grid)), "%s, grid %d" % (name, grid))


def test_a_reused_context_equals_fresh_ones():
    """9 000 tables, then 74 on the same context: a grid of 74 workgroups, in a table buffer that holds the first batch's bytes."""
    from vartrix_amd import lib
    (big, nb_big), (small, nb_small, _) = _many(8), _shallow()
    with lib.Context(default_config(aligner="banded", scoring_mode="coverage", n_barcodes=nb_big)) as ctx:
        got = []
        for batch in (big, small):
            ctx.submit(batch)
            ctx.run()
            got.append((ctx.debug_tables(), ctx.fetch_scores()))
    check("4 500 loci x 8 reads", big, nb_big, got[0], "first batch of the context")
    check("37 loci x 6 reads", small, nb_small, got[1], "second batch of the context")
    fresh = run(small, nb_small)
    assert np.array_equal(defined(got[1][0], small), defined(fresh[0], small))
    assert np.array_equal(got[1][1][0], fresh[1][0]) and np.array_equal(got[1][1][1], fresh[1][1])
