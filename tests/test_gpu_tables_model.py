"""The device's k-mer tables against the plain model and against the host mirror (tests/tables_model.py, tests/tables_cases.py).

For every batch of the corpus, at a depth without t3[] and at one with: vtx_run with the banded aligner on the production library, the
tables it left in global memory (vtx_debug_tables), and then
  * every table through check_table — P1 .. P9, the expectation computed from the haplotype's bytes alone;
  * every table's defined bytes but t3[] equal to the mirror's (vtxt_build_tables: the builder all the CPU soundness evidence of the
    certificate stages stands on — tests/test_fastcore.py, tests/test_mutants.py);
  * every score equal to the oracle's.
The families with long chains, twin-list edges and odd bytes also run round 3's kernel (libvtx_dev.so, VTX_BAND_TABLES_V1=1) through the
same three checks: where device and model disagree, the record shows which builder is off.  One batch runs with 256 buckets
(libvtx_dev.so, VTX_BAND_HEADS=256): more HEAD_MULTI buckets, longer chains, more tag collisions.

Not covered, by construction: the tables band_run_kernel builds for itself in LDS cannot be dumped; scores alone pin those."""
import os

import numpy as np
import pytest

from oracle import oracle
from vartrix_amd import lib
from vartrix_amd.abi import default_config

import tables_cases as TC
import tables_model as TM

pytestmark = pytest.mark.gpu
HOOKS = ("VTX_BAND_TABLES_V1", "VTX_BAND_HEADS", "VTX_BAND_TABLES_GRID", "VTX_BAND_CHUNK", "VTX_BAND_GT_BYTES", "VTX_BAND_GT_MAX_TPL")
V1_TOO = ("one bucket, many entries", "twin-list edges", "alphabet")


@pytest.fixture(scope="module")
def mirror():
    return TM.load_mirror()


def run(batch, nb, variant=None, **env):
    """(tables, (ref, alt)) of one run on a fresh context; env: hooks of libvtx_dev.so, read at every launch."""
    assert not env or variant == "dev"
    for k in HOOKS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        with lib.Context(default_config(aligner="banded", scoring_mode="coverage", n_barcodes=nb), variant=variant) as ctx:
            ctx.submit(batch)
            ctx.run()
            return ctx.debug_tables(), ctx.fetch_scores()
    finally:
        for k in HOOKS:
            os.environ.pop(k, None)


_oracle = {}           # label -> the oracle's scores, computed once and left alone


def oracle_scores(label, batch, nb):
    if label not in _oracle:
        _oracle[label] = oracle.batch_scores(batch, default_config(aligner="banded", n_barcodes=nb), threads=min(os.cpu_count() or 8, 16))
    return _oracle[label]


def three_checks(mirror, label, batch, nb, got, n_heads=1024, n_tables=None):
    """The model, the mirror, the oracle; returns (tables checked, tables compared with the mirror)."""
    tables, (r, a) = got
    assert len(tables) > 0, "%s: no tables in global memory" % label
    n_tables = 2 * batch.n_loci if n_tables is None else n_tables
    checked, compared = TM.check_tables(tables, batch, n_heads, TC.uses_t3(batch), label, mirror=TM.mirror_tables(mirror, batch, n_heads))
    assert checked == compared == n_tables, (label, checked, compared, n_tables)
    oref, oalt = oracle_scores(batch_label(label), batch, nb)
    bad = np.nonzero((r != oref) | (a != oalt))[0]
    assert bad.size == 0, "%s: %d records differ from the oracle, first %d: device (%d, %d) oracle (%d, %d)" % (
        label, bad.size, bad[0], r[bad[0]], a[bad[0]], oref[bad[0]], oalt[bad[0]])
    return checked, compared


def batch_label(label):
    return label.split(" | ")[0]


@pytest.mark.parametrize("family", list(TC.FAMILIES))
def test_device_tables_against_model_and_mirror(mirror, family):
    built = checked = compared = 0
    for label, batch, nb in TC.cases(family):
        runs = [(label + " | production", run(batch, nb))]
        if family in V1_TOO:
            runs.append((label + " | round 3's kernel", run(batch, nb, "dev", VTX_BAND_TABLES_V1="1")))
        for name, got in runs:
            n_tables = 2 * len(TC.LONG_LENGTHS) + 2 if family == "a long batch" else None       # (the long batch states its own count)
            c, m = three_checks(mirror, name, batch, nb, got, n_tables=n_tables)
            built += 2 * batch.n_loci
            checked += c
            compared += m
    print("%s: %d tables built, %d checked against the model, %d compared with the mirror" % (family, built, checked, compared))
    assert built == checked == compared > 0


def test_device_tables_with_256_buckets(mirror):
    label, batch, nb = TC.ordinary_real(TC.DEEP)
    c, m = three_checks(mirror, label + " | 256 buckets", batch, nb, run(batch, nb, "dev", VTX_BAND_HEADS="256"), n_heads=256)
    print("256 buckets: %d tables built, %d checked against the model, %d compared with the mirror" % (2 * batch.n_loci, c, m))
    assert c == m == 2 * batch.n_loci
