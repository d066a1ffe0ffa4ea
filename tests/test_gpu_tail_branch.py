"""band_tail_kernel on the side branch (vtx_api.hip: BandPass::tail_on_side).  Where the certificate stage's two
branches run side by side the kernel is launched on the side stream, beside band_sweep_kernel, and the host sizes the side branch's
grids from bounds instead of final counts.  libvtx_dev.so's VTX_BAND_TAIL_INLINE=1 keeps the kernel behind band_diag_kernel on the main
stream, as before: both must leave the same scores, stage bytes, triplets and task counts — on the ordinary path, with full buffers,
over several chunks and on a reused context — and the developer build's counter of records that the kernel routed towards the main
branch's lists must stay 0.  One process per run: the hooks are read once."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COUNTS = ("checked_tasks", "swept_tasks", "hard_tasks", "diag_left", "overflow_tasks")
COO = ("row", "col", "alt", "ref", "unk", "value", "ref_value")
LABELS = ("headline", "3 % errors", "repeat-rich")
HOOKS = ("VTX_BAND_TAIL_INLINE", "VTX_DIAG_TAIL_CAP", "VTX_DIAG_TAIL_GRID", "VTX_DIAG_REFINE_CAP", "VTX_BAND_CHUNK", "VTX_BAND_NO_FORK", "VTX_BAND_NO_TIGHT",
         "VTX_DIAG_NO_TAIL", "VTX_DIAG_ABLATE", "VTX_BAND_LEGACY", "VTX_DEBUG")

# 300 loci x 64 reads of bench.py's generator (38 k tasks: ~7 % deferred to band_tail_kernel, a handful left for the sweep), the same
# at 3 % substitution errors (corridor records and tight entries), a repeat-rich batch (a dense list).  argv[2] == "reuse": batch 0,
# batch 2, batch 0 again on ONE context, stored as 0, 1, 2.
CODE = r'''
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import stress_batches as SB
from vartrix_amd import lib, synth
from vartrix_amd.abi import default_config
NB = 2000
batches = [
    synth.make_batch(synth.SynthSpec(n_loci=300, n_barcodes=NB, reads_per_locus=64)),
    synth.make_batch(synth.SynthSpec(n_loci=300, n_barcodes=NB, reads_per_locus=64, sub_error=0.03)),
    next(iter(SB.repeat_rich_batches(trials=1, loci=60, reads=24, pad_range=(30, 110))))[1],
]
out = {}
def run(ctx, i, batch):
    ctx.submit(batch)
    ctx.run()
    out["ref%%d" %% i], out["alt%%d" %% i] = ctx.fetch_scores()
    out["stage%%d" %% i] = ctx.fetch_stage()
    coo = ctx.fetch_coo()
    for k in %r:
        out["%%s%%d" %% (k, i)] = np.array(coo[k], copy=True)
    t = ctx.timing()
    out["counts%%d" %% i] = np.array([int(getattr(t, k)) for k in %r], np.int64)
def context():
    ctx = lib.Context(default_config(aligner="banded", scoring_mode="coverage", n_barcodes=NB))
    ctx.set_stage_trace(True)
    return ctx
if len(sys.argv) > 2 and sys.argv[2] == "reuse":
    with context() as ctx:
        for i, b in enumerate((batches[0], batches[2], batches[0])):
            run(ctx, i, b)
else:
    for i, b in enumerate(batches):
        with context() as ctx:
            run(ctx, i, b)
np.savez(sys.argv[1], **out)
''' % (ROOT, os.path.join(ROOT, "tests"), COO, COUNTS)


def run_dev(env_extra, mode="fresh"):
    """One process on libvtx_dev.so with the given hooks: (its arrays, its stderr)."""
    env = dict(os.environ, VTX_LIB_VARIANT="dev")                     # (the hooks exist in libvtx_dev.so only)
    for k in HOOKS:
        env.pop(k, None)
    env.update(env_extra)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "out.npz")
        p = subprocess.run([sys.executable, "-c", CODE, path, mode], env=env, timeout=600, stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0, p.stderr[-4000:]
        with np.load(path) as z:
            return {k: z[k] for k in z.files}, p.stderr


_default = {}


def default_run():
    """The default run (band_tail_kernel on the side branch), once for the tests that compare with it."""
    if not _default:
        _default["out"] = run_dev({})[0]
    return _default["out"]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()       # (bit patterns: a value may be NaN)


def assert_same(a, b, what, stage=True, counts=True, pairs=((0, 0), (1, 1), (2, 2)), labels=LABELS):
    for (i, j), label in zip(pairs, labels):
        label = "%s, %s" % (what, label)
        assert np.array_equal(a["ref%d" % i], b["ref%d" % j]) and np.array_equal(a["alt%d" % i], b["alt%d" % j]), "%s: scores differ" % label
        for k in COO:
            assert same_bits(a["%s%d" % (k, i)], b["%s%d" % (k, j)]), "%s: COO field %s differs" % (label, k)
        if stage:
            sa, sb = a["stage%d" % i], b["stage%d" % j]
            assert np.array_equal(sa, sb), "%s: stages differ at %d tasks" % (label, int((sa != sb).sum()))
        if counts:
            assert np.array_equal(a["counts%d" % i], b["counts%d" % j]), "%s: %s vs %s" % (
                label, dict(zip(COUNTS, a["counts%d" % i].tolist())), dict(zip(COUNTS, b["counts%d" % j].tolist())))


def test_batches_reach_the_lists_the_move_rests_on():
    """The batches are what the cases need: a handful of tasks for the sweep on the headline batch, tasks that leave with a
    certificate (corridor records, tight entries) at 3 % errors, a dense list — tasks for the sweep — on the repeat-rich one."""
    d = default_run()
    c = [dict(zip(COUNTS, d["counts%d" % i].tolist())) for i in range(len(LABELS))]
    for label, ci in zip(LABELS, c):
        print(label, ci)
    assert c[0]["swept_tasks"] > 0, "headline: nothing for band_sweep_kernel"
    assert c[1]["checked_tasks"] > 0, "3 % errors: no task left the stage with a certificate"
    assert c[2]["swept_tasks"] > 0, "repeat-rich: nothing for band_sweep_kernel"


def test_side_branch_equals_inline():
    inline, _ = run_dev({"VTX_BAND_TAIL_INLINE": "1"})
    assert_same(default_run(), inline, "default vs VTX_BAND_TAIL_INLINE=1")


# VTX_DIAG_TAIL_CAP=64: the records that find no slot stay in their wavefront.  VTX_DIAG_REFINE_CAP=0: no record for the second look
# fits, so every undecided record of band_tail_kernel spills to the tight list — the second of the host's two bounds alone has to
# cover the list.  VTX_BAND_CHUNK=4096: ten chunks, the events re-recorded and the branches joined per chunk.  VTX_DIAG_TAIL_GRID=8:
# 512 lanes for the ~2 700 records, so every lane loops over several of them, as the lanes of the side launch's resident grid do
# on a batch of millions (the launch on the main stream has a workgroup per 64 records there).
@pytest.mark.parametrize("extra", [{"VTX_DIAG_TAIL_CAP": "64"}, {"VTX_DIAG_REFINE_CAP": "0"}, {"VTX_BAND_CHUNK": "4096"}, {"VTX_DIAG_TAIL_GRID": "8"}],
                         ids=["tail-buffer-full", "refine-buffer-none", "chunks", "looping-lanes"])
def test_side_branch_equals_inline_with(extra):
    side, _ = run_dev(dict(extra))
    inline, _ = run_dev(dict(extra, VTX_BAND_TAIL_INLINE="1"))
    assert_same(side, inline, "%s, side vs inline" % extra)
    # (neither hook changes a score or a triplet; VTX_BAND_CHUNK=4096 splits loci between chunks, which moves tasks between stages)
    assert_same(side, default_run(), "%s vs default" % extra, stage=False, counts=False)


def test_side_branch_equals_inline_with_a_small_refine_buffer():
    """VTX_DIAG_REFINE_CAP=64: band_diag_kernel's and band_tail_kernel's records compete for 64 slots, the others spill to the tight
    list.  WHICH records get a slot is the order of the wavefronts' atomics, in either mode: a task that loses its slot takes the
    masked DP where band_corridor_kernel might have decided it, so stage bytes and checked_tasks vary from run to run and are not
    compared.  Scores and triplets do not depend on it."""
    extra = {"VTX_DIAG_REFINE_CAP": "64"}
    side, _ = run_dev(dict(extra))
    inline, _ = run_dev(dict(extra, VTX_BAND_TAIL_INLINE="1"))
    assert_same(side, inline, "%s, side vs inline" % extra, stage=False, counts=False)
    assert_same(side, default_run(), "%s vs default" % extra, stage=False, counts=False)


def test_context_reuse():
    """headline, repeat-rich, headline again on one context: each step equals the same batch on a fresh context."""
    reused, _ = run_dev({}, mode="reuse")
    assert_same(reused, default_run(), "reused context vs fresh", pairs=((0, 0), (1, 2), (2, 0)),
                labels=("headline", "repeat-rich after headline", "headline again"))


def test_tail_routes_nothing_to_the_main_branch():
    """libvtx_dev.so counts the records band_tail_kernel's routing sends towards dense_list / fail_list although a tight list exists
    (vtx_band_counters::tail_stray; printed with VTX_DEBUG's statistics): 0 on every batch.  Inline, so that such a record would be counted and
    listed, not written through the null lists of the side launch."""
    out, err = run_dev({"VTX_DEBUG": "1", "VTX_BAND_TAIL_INLINE": "1"})
    stray = [int(n) for n in re.findall(r"band_tail_kernel: (\d+) records routed towards the dense or fail list", err)]
    assert len(stray) == len(LABELS), err[-4000:]
    assert stray == [0] * len(LABELS), stray
    assert_same(out, default_run(), "VTX_DEBUG=1 inline vs default")


@pytest.mark.parametrize("hook", ["VTX_BAND_NO_FORK", "VTX_BAND_NO_TIGHT"])
def test_inline_paths_unchanged(hook):
    """Without the fork, or without a tight list, the kernel stays behind band_diag_kernel on the main stream: the default's scores."""
    out, _ = run_dev({hook: "1"})
    assert_same(out, default_run(), "%s=1 vs default" % hook, stage=False, counts=False)
