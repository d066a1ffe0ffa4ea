"""Where the banded stage sends every task, pinned against the commit before the launchers took argument bundles
(vtx_device.h: vtx_task_arrays, vtx_band_shape, vtx_band_tables, vtx_diag_routes, vtx_rec_buf, vtx_band_out).  The A/B tests of the
suite compare a build with itself under hooks: a bundle field wired wrongly in EVERY configuration passes them, and since a null list
means "stage off" to most of these kernels such a mistake leaves correct scores by a slower route.  tests/golden/band_routes_parent.json
was recorded from the parent's libvtx_dev.so and must not change: per configuration and batch the sha256 of the scores, of the stage
bytes (vtx_fetch_stage: which stage decided each task) and of the triplets by bit pattern, and the task counts of vtx_timing.

Batches: the three of tests/test_gpu_tail_branch.py (300 loci x 64 reads; the same at 3 % substitution errors; a repeat-rich batch) and
one with 30 % indel loci, whose reads against the other allele lie on two diagonals (band_run_kernel's tasks).  The golden holds a
digest of every batch's arrays as well: a generator that changed fails as "inputs differ", not as a routing failure.

Configurations: sets of hooks vtx_api.hip reads, each steering other launchers (CONFIGS).  One process per configuration: the hooks
are read once.  The four batches overflow band_run_kernel's lists under VTX_BAND_LEGACY as they are (2 737 tasks of the repeat-rich
one, a handful of each other): no list is shrunk for the general kernel's path (band_coop_kernel / band_kernel).  The recorder
refuses to write a golden that does not reach the lists it claims to (record_checks), and test_golden_exercises_what_it_claims reads
the same off the committed file.

Re-record (with the tree of the commit to compare against built):  python tests/test_gpu_band_routes_pinned.py --record"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "band_routes_parent.json")

COUNTS = ("checked_tasks", "swept_tasks", "hard_tasks", "diag_left", "overflow_tasks")
COO = ("row", "col", "alt", "ref", "unk", "value", "ref_value")
LABELS = ("headline", "3 % errors", "repeat-rich", "indels")
CONFIGS = {
    "default": {},
    "no-fork": {"VTX_BAND_NO_FORK": "1"},
    "no-tight": {"VTX_BAND_NO_TIGHT": "1"},
    "no-corridor": {"VTX_BAND_NO_CORRIDOR": "1"},                      # band_refine_kernel
    "tail-inline": {"VTX_BAND_TAIL_INLINE": "1"},                      # band_tail_kernel launched from the diag launcher
    "check": {"VTX_BAND_CHECK": "1"},                                  # sw_check
    "diag2": {"VTX_BAND_DIAG2_MIN": "1"},                              # band_diag2_kernel, band_stream_kernel
    "chunks": {"VTX_BAND_CHUNK": "4096"},                              # several chunks
    "no-diag": {"VTX_BAND_NO_DIAG": "1"},                              # band_run_kernel in range mode
    "lds-tables": {"VTX_BAND_GT_MAX_TPL": "1"},                        # band_run_kernel with tables in LDS
    "legacy": {"VTX_BAND_LEGACY": "1"},                                # run, pending, expand, coop
    "legacy-no-coop": {"VTX_BAND_LEGACY": "1", "VTX_BAND_NO_COOP": "1"},   # band_kernel
}
HOOKS = sorted({k for env in CONFIGS.values() for k in env} |
               {"VTX_BAND_HARD_CAP", "VTX_BAND_SLOTS", "VTX_DIAG_TAIL_CAP", "VTX_DIAG_TAIL_GRID", "VTX_DIAG_REFINE_CAP", "VTX_DIAG_RECHECK_CAP",
                "VTX_DIAG_NO_TAIL", "VTX_DIAG_NO_RECHECK", "VTX_DIAG_ABLATE", "VTX_BAND_NO_STREAM", "VTX_BAND_NO_REFINE",
                "VTX_BAND_DENSE_MASK", "VTX_BAND_RUN_MIN", "VTX_DEBUG"})

# The child: the four batches, each on a fresh context with the stage trace on; one JSON object per batch.
CODE = r'''
import hashlib, json, sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import stress_batches as SB
from vartrix_amd import lib, synth
from vartrix_amd.abi import default_config
NB = 2000
batches = [
    synth.make_batch(synth.SynthSpec(n_loci=300, n_barcodes=NB, reads_per_locus=64)),
    synth.make_batch(synth.SynthSpec(n_loci=300, n_barcodes=NB, reads_per_locus=64, sub_error=0.03)),
    next(iter(SB.repeat_rich_batches(trials=1, loci=60, reads=24, pad_range=(30, 110))))[1],
    synth.make_batch(synth.SynthSpec(n_loci=300, n_barcodes=NB, reads_per_locus=64, indel_frac=0.3)),
]
def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%%s%%s;" %% (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())            # (bit patterns: a value may be NaN)
    return h.hexdigest()
out = []
for b in batches:
    with lib.Context(default_config(aligner="banded", scoring_mode="coverage", n_barcodes=NB)) as ctx:
        ctx.set_stage_trace(True)
        ctx.submit(b)
        ctx.run()
        ref, alt = ctx.fetch_scores()
        stage = ctx.fetch_stage()
        coo = ctx.fetch_coo()
        t = ctx.timing()
        out.append(dict(input=sha(b.loci, b.records, b.hap_arena, b.read_arena), scores=sha(ref, alt), stage=sha(stage),
                        coo=sha(*[coo[k] for k in %r]), counts={k: int(getattr(t, k)) for k in %r}))
json.dump(out, open(sys.argv[1], "w"))
''' % (ROOT, os.path.join(ROOT, "tests"), COO, COUNTS)


def run_config(name):
    """One process on libvtx_dev.so under the configuration's hooks: label -> the batch's digests and counts."""
    env = dict(os.environ, VTX_LIB_VARIANT="dev")                     # (the hooks exist in libvtx_dev.so only)
    for k in HOOKS:
        env.pop(k, None)
    env.update(CONFIGS[name])
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "out.json")
        p = subprocess.run([sys.executable, "-c", CODE, path], env=env, timeout=600, stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0, p.stderr[-4000:]
        return dict(zip(LABELS, json.load(open(path))))


def record_checks(configs):
    """What the recorded runs must show for the golden to pin what it claims to; a list of complaints."""
    bad = []
    d = configs["default"]
    if not d["repeat-rich"]["counts"]["swept_tasks"] > 0:
        bad.append("default, repeat-rich: nothing for band_sweep_kernel")
    if not d["3 % errors"]["counts"]["checked_tasks"] > 0:
        bad.append("default, 3 % errors: no task left the stage with a certificate")
    if not d["indels"]["counts"]["hard_tasks"] > 0:
        bad.append("default, indels: no hard task")
    for name in ("legacy", "legacy-no-coop"):
        if not any(configs[name][label]["counts"]["overflow_tasks"] > 0 for label in LABELS):
            bad.append("%s: no batch overflows band_run_kernel's lists" % name)
    for name in ("no-tight", "no-diag", "legacy"):
        if all(configs[name][label]["stage"] == d[label]["stage"] for label in LABELS):
            bad.append("%s: the stage bytes of every batch are the default's" % name)
    return bad


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def test_golden_exercises_what_it_claims(golden):
    assert sorted(golden["configs"]) == sorted(CONFIGS) and sorted(golden["inputs"]) == sorted(LABELS)
    for name, env in CONFIGS.items():
        assert golden["hooks"][name] == env, "%s: the golden was recorded under other hooks" % name
        assert sorted(golden["configs"][name]) == sorted(LABELS)
    assert record_checks(golden["configs"]) == []


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_routes_are_the_parents(golden, name):
    got = run_config(name)
    for label in LABELS:
        assert got[label]["input"] == golden["inputs"][label], "%s: inputs differ, re-record from the parent" % label
    for label in LABELS:
        g, want = got[label], golden["configs"][name][label]
        print(name, label, g["counts"])
        assert g["scores"] == want["scores"], "%s, %s: scores differ from the parent's" % (name, label)
        assert g["coo"] == want["coo"], "%s, %s: triplets differ from the parent's" % (name, label)
        assert g["counts"] == want["counts"], "%s, %s: task counts %s, the parent's %s" % (name, label, g["counts"], want["counts"])
        assert g["stage"] == want["stage"], "%s, %s: stage bytes differ from the parent's" % (name, label)


def record():
    configs = {name: run_config(name) for name in CONFIGS}
    inputs = {label: configs["default"][label]["input"] for label in LABELS}
    for name, by_label in configs.items():
        for label in LABELS:
            assert by_label[label].pop("input") == inputs[label], "the batches depend on the process: %s, %s" % (name, label)
            print(name, label, by_label[label]["counts"])
    bad = record_checks(configs)
    assert not bad, "not recorded: " + "; ".join(bad)
    with open(GOLDEN, "w") as f:
        json.dump(dict(inputs=inputs, hooks=CONFIGS, configs=configs), f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d configurations x %d batches" % (len(configs), len(LABELS)))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true")
    if ap.parse_args().record:
        record()
