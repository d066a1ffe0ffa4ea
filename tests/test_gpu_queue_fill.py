"""The queue fill of band_diag_kernel's pooled probes, blocks of three rows (vtx_band.hip, the t3 path): a lane walks its block ends in
place, 32 bits at a time, and takes a block's three membership bits from the pair's rows shifted by two.  The batches of
tests/queue_fill_util.py (2 loci x 16 reads: read lengths at the mask-word edges and below three rows, reads hanging over the window by
0 - 49 bases on either side, a substitution at either end of the read) go through libvtx_dev.so four times, a process each (the hooks are
read once):

  default                      blocks of three rows on by depth
  VTX_DIAG_T3=1                ... forced
  VTX_DIAG_NO_T3=1             a queue entry per row: the fill that has no block arithmetic
  VTX_DIAG_T3=1 VTX_DIAG_FOUR_WORDS=1   the build for reads up to 256 bases on every batch

(a) the scores of the first two are the oracle's; (b) scores, the stage byte of every task and the task counts of every later stage are
the same in the last three."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import queue_fill_util as QF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COUNTS = ("hard_tasks", "overflow_tasks", "diag_left", "checked_tasks", "swept_tasks", "resweep_tasks", "diag2_tasks", "diag2_scored",
          "diag2_streamed")
RUNS = {"default": {}, "t3": {"VTX_DIAG_T3": "1"}, "no_t3": {"VTX_DIAG_NO_T3": "1"},
        "t3_four": {"VTX_DIAG_T3": "1", "VTX_DIAG_FOUR_WORDS": "1"}}

CODE = r'''
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import queue_fill_util as QF
from vartrix_amd import lib
from vartrix_amd.abi import default_config
out = {}
for i, (label, batch, nb) in enumerate(QF.batches()):
    with lib.Context(default_config(aligner="banded", scoring_mode="coverage", n_barcodes=nb)) as ctx:
        ctx.set_stage_trace(True)
        ctx.submit(batch)
        ctx.run()
        out["ref%%d" %% i], out["alt%%d" %% i] = ctx.fetch_scores()
        out["stage%%d" %% i] = ctx.fetch_stage()
        t = ctx.timing()
        out["counts%%d" %% i] = np.array([int(getattr(t, k)) for k in %r], np.int64)
np.savez(sys.argv[1], **out)
''' % (ROOT, os.path.join(ROOT, "tests"), COUNTS)


@pytest.fixture(scope="module")
def runs():
    """name -> the arrays of one process; the four run side by side."""
    with tempfile.TemporaryDirectory() as td:
        procs = {}
        for name, extra in RUNS.items():
            env = dict(os.environ, VTX_LIB_VARIANT="dev")                 # (the hooks exist in libvtx_dev.so only)
            for k in ("VTX_DIAG_T3", "VTX_DIAG_NO_T3", "VTX_DIAG_FOUR_WORDS", "VTX_DIAG_ABLATE", "VTX_DIAG_NO_TWINS", "VTX_DIAG_WIDE"):
                env.pop(k, None)
            env.update(extra)
            procs[name] = subprocess.Popen([sys.executable, "-c", CODE, os.path.join(td, name + ".npz")], env=env)
        codes = {name: p.wait(timeout=600) for name, p in procs.items()}
        assert not any(codes.values()), codes
        yield {name: dict(np.load(os.path.join(td, name + ".npz"))) for name in RUNS}


@pytest.fixture(scope="module")
def expected():
    from oracle import oracle
    from vartrix_amd.abi import default_config
    return [oracle.batch_scores(batch, default_config(aligner="banded", scoring_mode="coverage", n_barcodes=nb), threads=4)
            for _, batch, nb in QF.batches()]


def test_batches_cover_the_shapes():
    specs = QF.read_specs()
    assert {m for m, _, _, _ in specs} == set(QF.LENS3 + QF.LENS4)
    for m in (150, 250):
        assert {(s, h) for mm, s, h, _ in specs if mm == m} == {("L", 0)} | {(s, h) for s in "LR" for h in (1, 2, 3, 5, 49)}
        assert {sub for mm, _, _, sub in specs if mm == m} == {None, 0, 1, 2, m - 3, m - 2, m - 1}
    assert all(b.n_records == 32 and len(b.loci) == 2 for _, b, _ in QF.batches())


@pytest.mark.parametrize("name", ["default", "t3"])
def test_scores_are_the_oracles(runs, expected, name):
    for i, (label, _, _) in enumerate(QF.batches()):
        oref, oalt = expected[i]
        ref, alt = runs[name]["ref%d" % i], runs[name]["alt%d" % i]
        bad = np.nonzero((ref != oref) | (alt != oalt))[0]
        assert len(bad) == 0, "%s, %s: %d records differ from the oracle; first %d: device %d / %d, oracle %d / %d" % (
            name, label, len(bad), bad[0], ref[bad[0]], alt[bad[0]], oref[bad[0]], oalt[bad[0]])


@pytest.mark.parametrize("name", ["no_t3", "t3_four"])
def test_fill_variants_agree(runs, name):
    a, b = runs["t3"], runs[name]
    for i, (label, _, _) in enumerate(QF.batches()):
        assert np.array_equal(a["ref%d" % i], b["ref%d" % i]) and np.array_equal(a["alt%d" % i], b["alt%d" % i]), "%s: scores differ" % label
        sa, sb = a["stage%d" % i], b["stage%d" % i]
        assert np.array_equal(sa, sb), "%s: stages differ at %d tasks" % (label, int((sa != sb).sum()))
        assert np.array_equal(a["counts%d" % i], b["counts%d" % i]), "%s: %s vs %s" % (
            label, dict(zip(COUNTS, a["counts%d" % i].tolist())), dict(zip(COUNTS, b["counts%d" % i].tolist())))
