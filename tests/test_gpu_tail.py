"""band_tail_kernel (vtx_band.hip): the tasks band_diag_kernel defers at the closure's first scan finish in a kernel of their own and
must end exactly as they did in their wavefront.  libvtx_dev.so with and without VTX_DIAG_NO_TAIL=1 (every task in its wavefront) on a
clean batch, one with 8 % substitution errors and an adversarial one: the same scores, the same stage byte per task, the same task
counts of every later stage.  Also with four-byte match entries (VTX_DIAG_WIDE=1) and with a record buffer that overflows
(VTX_DIAG_TAIL_CAP: the lanes that find no slot finish in their wavefront).  One process per run: some hooks are read once."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COUNTS = ("hard_tasks", "overflow_tasks", "diag_left", "checked_tasks", "swept_tasks", "resweep_tasks", "diag2_tasks", "diag2_scored",
          "diag2_streamed")

CODE = r'''
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import stress_batches as SB
from vartrix_amd import lib, synth
from vartrix_amd.abi import default_config
batches = [
    ("clean", synth.make_batch(synth.SynthSpec(n_loci=1500, n_barcodes=2000, reads_per_locus=128, seed=11)), 2000),
    ("8 %% errors", synth.make_batch(synth.SynthSpec(n_loci=800, n_barcodes=2000, reads_per_locus=128, sub_error=0.08, seed=12)), 2000),
    ("adversarial", SB.adversarial_batch(600, 32, seed=13), 500),
]
out = {}
for i, (label, batch, nb) in enumerate(batches):
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


def run_dev(env_extra, path):
    env = dict(os.environ, VTX_LIB_VARIANT="dev")                     # (the hooks exist in libvtx_dev.so only)
    for k in ("VTX_DIAG_NO_TAIL", "VTX_DIAG_WIDE", "VTX_DIAG_TAIL_CAP", "VTX_DIAG_ABLATE"):
        env.pop(k, None)
    env.update(env_extra)
    subprocess.check_call([sys.executable, "-c", CODE, path], env=env, timeout=600)
    return np.load(path)


@pytest.mark.parametrize("extra", [{}, {"VTX_DIAG_WIDE": "1"}, {"VTX_DIAG_TAIL_CAP": "700"}], ids=["narrow", "wide", "overflow"])
def test_tail_kernel_matches_in_wavefront_path(extra):
    with tempfile.TemporaryDirectory() as td:
        a = run_dev(dict(extra, VTX_DIAG_NO_TAIL="1"), os.path.join(td, "a.npz"))
        b = run_dev(dict(extra), os.path.join(td, "b.npz"))
        for i, label in enumerate(("clean", "8 % errors", "adversarial")):
            assert np.array_equal(a["ref%d" % i], b["ref%d" % i]) and np.array_equal(a["alt%d" % i], b["alt%d" % i]), "%s: scores differ" % label
            sa, sb = a["stage%d" % i], b["stage%d" % i]
            assert np.array_equal(sa, sb), "%s: stages differ at %d tasks" % (label, int((sa != sb).sum()))
            assert np.array_equal(a["counts%d" % i], b["counts%d" % i]), "%s: %s vs %s" % (
                label, dict(zip(COUNTS, a["counts%d" % i].tolist())), dict(zip(COUNTS, b["counts%d" % i].tolist())))
