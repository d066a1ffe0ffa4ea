"""The recheck of the tasks that fail band_diag_kernel's harmless test (vtx_band.hip: band_tail_kernel's recheck mode; vtx_api.hip:
BandPass::diag_sweep_path).  Such a task leaves the tail's record; the kernel runs the tight form of the test on the
record's list and routes the task — decided, a record for band_corridor_kernel or a tight entry when cleared, the fail list when not.
libvtx_dev.so's VTX_DIAG_NO_RECHECK=1 switches it off, VTX_DIAG_RECHECK_CAP=n makes the buffer small.  One process per run: the
hooks are read once.

Scores must be the same bytes in all three runs.  The stage byte of a task (vtx_fetch_stage) says WHICH stage decided it, so it cannot
be the same where the recheck does its work: a cleared task is decided by the certificate stages (1, 7 or 11) instead of the sweep's
DP (4).  Pinned here instead: the stage bytes are identical on every task the mirror does not clear; on a cleared task the stage with
the recheck is the one the mirror names, and without it the sweep's; with a buffer of 8 records every task has one of the two."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import recheck_util as RU

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("VTX_DIAG_NO_RECHECK", "VTX_DIAG_RECHECK_CAP", "VTX_BAND_TAIL_INLINE", "VTX_DIAG_TAIL_CAP", "VTX_DIAG_REFINE_CAP", "VTX_BAND_CHUNK", "VTX_BAND_NO_FORK",
         "VTX_BAND_NO_TIGHT", "VTX_DIAG_NO_TAIL", "VTX_DIAG_ABLATE", "VTX_BAND_LEGACY", "VTX_DIAG_WIDE", "VTX_BAND_NO_CORRIDOR", "VTX_DEBUG")
STAGE_DIAG_CERT, STAGE_SWEEP_DP, STAGE_GENERAL_DP, STAGE_DIAG_DP, STAGE_CORRIDOR_CERT = 1, 4, 5, 7, 11
N = len(RU.GPU_LABELS)

# argv[2] == "reuse": batch 2, batch 1 (an unlike one: other read lengths, another kernel build), batch 2 again on ONE context, stored as 0, 1, 2
CODE = r'''
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import recheck_util as RU
from vartrix_amd import lib
from vartrix_amd.abi import default_config
batches = RU.gpu_batches()
out = {}
def run(ctx, i, batch):
    ctx.submit(batch)
    ctx.run()
    out["ref%%d" %% i], out["alt%%d" %% i] = ctx.fetch_scores()
    out["stage%%d" %% i] = ctx.fetch_stage()
    t = ctx.timing()
    out["counts%%d" %% i] = np.array([int(t.swept_tasks), int(t.hard_tasks), int(t.diag_left)], np.int64)
def context():
    ctx = lib.Context(default_config(aligner="banded", scoring_mode="coverage", n_barcodes=RU.NB))
    ctx.set_stage_trace(True)
    return ctx
if len(sys.argv) > 2 and sys.argv[2] == "reuse":
    with context() as ctx:
        for i, b in enumerate((batches[2], batches[1], batches[2])):
            run(ctx, i, b)
else:
    for i, b in enumerate(batches):
        with context() as ctx:
            run(ctx, i, b)
np.savez(sys.argv[1], **out)
''' % (ROOT, os.path.join(ROOT, "tests"))


def run_dev(env_extra, mode="fresh"):
    """One process on libvtx_dev.so with the given hooks and VTX_DEBUG's statistics: its arrays, and per run (rechecked, cleared)."""
    env = dict(os.environ, VTX_LIB_VARIANT="dev")
    for k in HOOKS:
        env.pop(k, None)
    env.update(env_extra, VTX_DEBUG="1")
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "out.npz")
        p = subprocess.run([sys.executable, "-c", CODE, path, mode], env=env, timeout=300, stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0, p.stderr[-4000:]
        with np.load(path) as z:
            out = {k: z[k] for k in z.files}
    counts = [(int(a), int(b)) for a, b in re.findall(r"recheck: (\d+) tasks that failed band_diag_kernel's harmless test rechecked, (\d+) cleared", p.stderr)]
    return out, counts


_cache = {}


def cached(key, *args, **kw):
    if key not in _cache:
        _cache[key] = run_dev(*args, **kw)
    return _cache[key]


def on_run():
    return cached("on", {})


def off_run():
    return cached("off", {"VTX_DIAG_NO_RECHECK": "1"})


@pytest.fixture(scope="module")
def mirrored(tmp_path_factory):
    """The host mirror on the same batches: per batch (rc, score, why, route, pack)."""
    L = RU.load_mirror(tmp_path_factory.mktemp("recheck"))
    return [RU.mirror(L, b) for b in RU.gpu_batches()]


def tasks(a, i):
    t = np.empty(2 * a["ref%d" % i].size, np.int32)
    t[0::2], t[1::2] = a["ref%d" % i], a["alt%d" % i]
    return t


def assert_same_scores(a, b, what, pairs=None):
    for i, j in pairs or [(k, k) for k in range(N)]:
        assert tasks(a, i).tobytes() == tasks(b, j).tobytes(), "%s, %s: %d scores differ" % (what, RU.GPU_LABELS[i], int((tasks(a, i) != tasks(b, j)).sum()))


def test_batches_hold_tasks_for_the_recheck(mirrored):
    """Each batch with haplotypes of <= 255 bases has tasks that fail the coarse test; the real-sequence ones have tasks the tight test
    clears, decided outright and through the corridor; both builds of the kernels run (reads <= 192 and 193 - 256 bases)."""
    bs = RU.gpu_batches()
    assert int(bs[0].records["read_len"].max()) <= 192 and 192 < int(bs[2].records["read_len"].max()) <= 256
    assert max(int(bs[3].loci["ref_len"].max()), int(bs[3].loci["alt_len"].max())) > 255 and mirrored[3][0] == -1
    for i in range(3):
        rc, _, _, route, _ = mirrored[i]
        failed, cleared = int(((route & RU.LOOSE_FAILED) != 0).sum()), int(((route & RU.CLEARED) != 0).sum())
        print(RU.GPU_LABELS[i], "failed the coarse test:", failed, "cleared:", cleared)
        assert rc == 0 and failed >= 20, (RU.GPU_LABELS[i], failed)
        assert np.array_equal((route & RU.CLEARED) != 0, (route & RU.CLEARED_DIRECT) != 0)
    for i in (0, 2):
        route = mirrored[i][3]
        cl = (route & RU.CLEARED) != 0
        assert (cl & ((route & RU.DECIDED) != 0)).sum() >= 5 and (cl & ((route & RU.CORRIDOR) != 0)).sum() >= 5, RU.GPU_LABELS[i]


def test_scores_do_not_depend_on_the_recheck():
    on, off = on_run()[0], off_run()[0]
    assert_same_scores(on, off, "recheck on vs VTX_DIAG_NO_RECHECK=1")
    # swept_tasks and hard_tasks fall where the recheck clears tasks (the counts the change is about), and never rise
    for i in range(N):
        assert np.all(on["counts%d" % i][:2] <= off["counts%d" % i][:2]), (RU.GPU_LABELS[i], on["counts%d" % i], off["counts%d" % i])
    assert on["counts0"][0] < off["counts0"][0] and on["counts2"][0] < off["counts2"][0]


def test_device_counts_equal_the_mirror(mirrored):
    _, counts = on_run()
    assert len(counts) == N, counts
    for i in range(N):
        rc, _, _, route, _ = mirrored[i]
        want = (0, 0) if rc != 0 else (int(((route & RU.LOOSE_FAILED) != 0).sum()), int(((route & RU.CLEARED) != 0).sum()))
        assert counts[i] == want, (RU.GPU_LABELS[i], counts[i], want)
    assert off_run()[1] == [(0, 0)] * N


def test_a_cleared_task_is_decided_where_the_mirror_says(mirrored):
    on, off = on_run()[0], off_run()[0]
    for i in range(N):
        rc, score, _, route, _ = mirrored[i]
        sa, sb = on["stage%d" % i], off["stage%d" % i]
        cl = ((route & RU.CLEARED) != 0) if rc == 0 else np.zeros(sa.size, bool)
        assert np.array_equal(sa[~cl], sb[~cl]), "%s: stages differ at %d tasks the recheck does not clear" % (RU.GPU_LABELS[i], int((sa[~cl] != sb[~cl]).sum()))
        if rc != 0:
            continue
        want = np.where((route & RU.DECIDED) != 0, STAGE_DIAG_CERT, np.where((route & RU.CORRIDOR) != 0, STAGE_CORRIDOR_CERT, STAGE_DIAG_DP))
        assert np.array_equal(sa[cl], want[cl]), (RU.GPU_LABELS[i], sa[cl].tolist(), want[cl].tolist())
        assert np.all((sb[cl] == STAGE_SWEEP_DP) | (sb[cl] == STAGE_GENERAL_DP)), (RU.GPU_LABELS[i], sb[cl].tolist())
        # what the certificate stages decide for a cleared task is the mirror's score
        fin = cl & (((route & RU.DECIDED) != 0) | ((route & RU.CORRIDOR) != 0))
        assert np.array_equal(tasks(on, i)[fin], score[fin]), RU.GPU_LABELS[i]


def test_an_overflowing_buffer_keeps_the_scores(mirrored):
    """VTX_DIAG_RECHECK_CAP=8: eight records fit, the other tasks leave as they did before the recheck existed."""
    small, counts = cached("cap8", {"VTX_DIAG_RECHECK_CAP": "8"})
    on, off = on_run()[0], off_run()[0]
    assert_same_scores(small, on, "VTX_DIAG_RECHECK_CAP=8 vs default")
    for i in range(N):
        s, sa, sb = small["stage%d" % i], on["stage%d" % i], off["stage%d" % i]
        assert np.all((s == sa) | (s == sb)), RU.GPU_LABELS[i]
        if mirrored[i][0] == 0:
            assert int(((mirrored[i][3] & RU.LOOSE_FAILED) != 0).sum()) > 8 and counts[i][0] == 8 and counts[i][1] <= 8, (RU.GPU_LABELS[i], counts[i])
        else:
            assert counts[i] == (0, 0)


def test_long_haplotypes_run_without_the_recheck():
    """A batch with a haplotype above 255 bases takes four-byte match entries and round 3's path: no recheck record, no launch, and
    the scores of a run with the recheck switched off."""
    (on, counts), off = on_run(), off_run()[0]
    assert counts[3] == (0, 0)
    assert tasks(on, 3).tobytes() == tasks(off, 3).tobytes() and np.array_equal(on["stage3"], off["stage3"])


def test_context_reuse():
    """230-base reads, then 150-base reads at 3 % errors (another build of both kernels, other counts), then the first batch again, on one
    context: each run gives the bytes of the same batch on a fresh context."""
    reused, counts = cached("reuse", {}, mode="reuse")
    fresh, fcounts = on_run()
    for i, j in ((0, 2), (1, 1), (2, 2)):
        assert tasks(reused, i).tobytes() == tasks(fresh, j).tobytes(), (i, j)
        assert np.array_equal(reused["stage%d" % i], fresh["stage%d" % j]) and np.array_equal(reused["counts%d" % i], fresh["counts%d" % j]), (i, j)
    assert counts == [fcounts[2], fcounts[1], fcounts[2]], (counts, fcounts)
