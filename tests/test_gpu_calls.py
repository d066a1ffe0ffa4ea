"""The call stage on the device — group_heads_kernel, group_table_kernel, count_calls_kernel, umi_collapse_kernel, keep_flags_kernel,
emit_coo_kernel (vtx_kernels.hip), values_from_counts_kernel behind vtx_gather_coo, and the raw path's UMI grouping
(prep_resolve_kernel, prep_finalize_kernel; vtx_prep.hip) — against tests/call_model.py on the authored batches of
tests/call_cases.py.  tests/test_call_model.py shows on the CPU that those batches reach every class of the stage (every REF / ALT /
UNKNOWN / None boundary at five thresholds, every UMI-family composition up to 8 reads, every cell composition, repeated ids across
group boundaries, groups longer than a block, heads on block edges) and that every read scores what its construction promises.

Here: vtx_fetch_scores equals the oracle's scores, and vtx_fetch_coo equals the MODEL run on the ORACLE's scores, so that a wrong
score cannot hide a wrong call.  Every comparison is exact: integers, and bit patterns for the values (NaN included).

That the tests bite was checked once per one-token change of the device source (a scratch build each, this file run once):
  umi_collapse_kernel `>=` -> `>` (ALT's test; REF's)        test_calls_equal_the_model, every use_umi = 1 case
  count_calls_kernel  `&` -> `|` in the None test; `rs > as` -> `rs >= as`     test_calls_equal_the_model, every case
  group_heads_kernel  the rec_locus comparison dropped        test_calls_equal_the_model, every case
  group_heads_kernel  hu from the umi_id comparison alone      test_calls_equal_the_model, use_umi = 1 through vtx_submit (vtx_submit_raw
                                                               numbers its families itself), test_nothing_of_the_call_stage_survives_a_run
  keep_flags_kernel   keep ignoring the mode                   test_calls_equal_the_model, alt_frac and coverage
  emit_coo_kernel     k dropped from alt_frac's denominator    test_calls_equal_the_model, alt_frac
  values_from_counts_kernel  the same                          test_gathered_values_equal_the_model
  prep_finalize_kernel  umi_len left out of the comparison     test_a_ub_that_is_a_prefix_of_its_neighbour_is_another_family
  umi_collapse_kernel ALT and REF tested in the other order    nothing, and nothing can: 4r >= 3t and 4a >= 3t would need r + a >= 1.5 t"""
import os
import subprocess
import sys

import numpy as np
import pytest

import call_cases as CC
import call_model as CM
from oracle import prep
from vartrix_amd import lib
from vartrix_amd.abi import LOCUS_DTYPE, RAW_RECORD_DTYPE, RawBatch, default_config

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODES = ("consensus", "alt_frac", "coverage")
ALL_FIVE = {"full": "alt_frac", "banded": "coverage"}          # the mode in which an aligner runs all five thresholds


def config(aligner, mode, umi, m):
    return default_config(aligner=aligner, scoring_mode=mode, use_umi=umi, n_barcodes=CC.N_BARCODES, min_score=m)


def expected(case, aligner, mode, umi, m, path):
    """(ref, alt, entries as arrays, prepared batch) the device has to produce for `case`: the oracle's scores, the model's entries."""
    if path == "submit":
        packed = case.batch
        scores = case.oracle_scores(aligner)
    else:
        packed, _ = prep.prep_raw(CC.raw_form(case), CC.BARCODES, bool(umi))
        scores = case.scores_of(packed.records, aligner)
    entries, _ = CM.run(case.model_loci(packed), case.model_records(packed), scores[0], scores[1], m, umi, MODES.index(mode), case.n_barcodes)
    return scores, CM.as_arrays(entries), packed


def run_case(ctx, case, aligner, mode, umi, m, path):
    """One batch through one context: submit (or submit_raw), run, and everything it leaves against the oracle and the model."""
    label = "%s %s umi %d min_score %d %s, batch %s" % (aligner, mode, umi, m, path, case.name)
    scores, want, packed = expected(case, aligner, mode, umi, m, path)
    if path == "submit":
        ctx.submit(case.batch)
    else:
        stats = ctx.submit_raw(CC.raw_form(case))
        assert (int(stats.kept), int(stats.num_not_cell_bc), int(stats.num_non_umi)) == (case.n, 0, 0), label
        assert stats.hash_rounds == 1, label
        recs, begin, count = ctx.fetch_records()
        assert np.array_equal(begin, packed.loci["rec_begin"]) and np.array_equal(count, packed.loci["rec_count"]), label
        # the model's grouping, up to the order inside a family and the families' names
        assert prep.canonical_records(recs, begin, count) == prep.canonical_records(packed.records, begin, count), label
        scores = case.scores_of(recs, aligner)                 # (the device's own order inside a family)
    ctx.run()
    r, a = ctx.fetch_scores()
    bad = np.nonzero((r != scores[0]) | (a != scores[1]))[0]
    assert bad.size == 0, "%s: record %d scores %d / %d, the oracle %d / %d" % (label, bad[0], r[bad[0]], a[bad[0]], scores[0][bad[0]], scores[1][bad[0]])
    got = ctx.fetch_coo()
    CM.assert_same(got, want, label)
    return got


def thresholds(aligner, mode):
    return CC.MIN_SCORES if ALL_FIVE[aligner] == mode else (25, 26)


@pytest.mark.parametrize("path", ["submit", "submit_raw"])
@pytest.mark.parametrize("umi", [0, 1])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("aligner", ["full", "banded"])
def test_calls_equal_the_model(aligner, mode, umi, path):
    for m in thresholds(aligner, mode):
        with lib.Context(config(aligner, mode, umi, m)) as ctx:
            if path == "submit_raw":
                ctx.set_barcodes(CC.BARCODES)
            for case in CC.cases_for(umi):
                if path == "submit_raw" and case.name == "unsorted-umi":
                    continue                                   # (a raw batch has no umi_id to leave unsorted)
                run_case(ctx, case, aligner, mode, umi, m, path)


@pytest.mark.parametrize("aligner,mode,umi", [("full", "alt_frac", 1), ("banded", "consensus", 1), ("full", "coverage", 0)])
def test_nothing_of_the_call_stage_survives_a_run(aligner, mode, umi):
    """Five contexts, one per min_score, open together; the batches go through them in turn, so every context runs unlike batches
    one after the other (group tables, counters and keep flags of a 3 000-record batch, then of a 256-record one) while its
    neighbours run the same batches under another threshold."""
    ctxs = {m: lib.Context(config(aligner, mode, umi, m)) for m in CC.MIN_SCORES}
    try:
        first = {}
        order = CC.cases_for(umi)
        for case in order + order[::-1]:
            for m in CC.MIN_SCORES:
                got = run_case(ctxs[m], case, aligner, mode, umi, m, "submit")
                again = first.setdefault((case.name, m), got)
                for k in got:
                    assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), (case.name, m, k)
        # the thresholds really gave five different results (the reads that stand alone in their cells see to that)
        nnz = {m: len(first[("main", m)]["row"]) for m in CC.MIN_SCORES}
        assert len({b"".join(first[("main", m)][k].tobytes() for k in ("row", "col", "ref", "alt", "unk")) for m in CC.MIN_SCORES}) == 5
        assert nnz[151] == 0 if mode == "consensus" else len(set(nnz.values())) == 1, nnz
    finally:
        for c in ctxs.values():
            c.close()


GATHER_CHILD = r'''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import call_cases as CC
import call_model as CM
import test_gpu_calls as T
from vartrix_amd import lib
for mode, umi, m in (("alt_frac", 1, 25), ("consensus", 1, 26), ("alt_frac", 0, 151), ("coverage", 1, 25)):
    with lib.Context(T.config("full", mode, umi, m)) as ctx:
        ctx.comm_init(lib.comm_id(), 0, 1)
        for case in CC.cases_for(umi):
            T.run_case(ctx, case, "full", mode, umi, m, "submit")
            _, want, _ = T.expected(case, "full", mode, umi, m, "submit")
            d = ctx.gather_coo(0)
            assert d["nnz"] == len(want["row"]), (mode, case.name, d["nnz"])
            CM.assert_same(ctx.fetch_gathered(), want, "gathered, %%s umi %%d min_score %%d, batch %%s" %% (mode, umi, m, case.name))
            print(mode, umi, m, case.name, d["nnz"], int(np.isnan(want["value"]).sum()))
print("calls-gather-ok")
''' % (ROOT, HERE)


def test_gathered_values_equal_the_model():
    """vtx_gather_coo with world 1 after alt_frac, consensus and coverage runs: values_from_counts_kernel recomputes the values from
    the gathered counts; they equal the model's bit for bit, NaN included (min_score 151: every value is NaN).  (A child process, as
    tests/test_gpu_context_reuse.py runs its communicator.)"""
    p = subprocess.run([sys.executable, "-c", GATHER_CHILD], env=dict(os.environ), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "calls-gather-ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("alt_frac")]
    assert any(int(ln[-1]) > 0 for ln in lines if ln[2] == "25") and all(ln[-1] == ln[-2] for ln in lines if ln[2] == "151"), p.stdout


def prefix_batch():
    """Every cell's UBs, in record order, are each a prefix of the one before (down to the empty string): the only pairs of distinct
    UMIs the collision check of prep_finalize_kernel ever compares here are (longer, its prefix)."""
    ubs = [[b"ACGTACGTAC", b"ACGTACGT", b"ACGT", b""], [b"TTGCA", b"TTG"], [b"G", b""]]
    kinds = (CC.R, CC.A, CC.U, CC.R)
    tags, raw, arena = bytearray(), [], bytearray()
    for cell, chain in enumerate(ubs):
        for j, ub in enumerate(chain):
            for rep in range(2):
                seq, _ = kinds[j](3 * cell + rep)
                bc = CC.BARCODES[cell]
                raw.append((len(arena), len(seq), len(tags), len(tags) + len(bc), len(bc), len(ub)))
                arena += seq
                tags += bc + ub
    loci = np.array([(4, 0, len(raw), 0, len(CC.REF_HAP), len(CC.REF_HAP), len(CC.ALT_HAP), 0)], LOCUS_DTYPE)
    return RawBatch(loci, np.array(raw, RAW_RECORD_DTYPE), np.frombuffer(CC.REF_HAP + CC.ALT_HAP, np.uint8),
                    np.frombuffer(bytes(arena), np.uint8), np.frombuffer(bytes(tags) + b"A", np.uint8))


def test_a_ub_that_is_a_prefix_of_its_neighbour_is_another_family(monkeypatch):
    """The developer library's hook hashes every UB to 0 in the first round (tests/test_gpu_prep.py), so equal hashes meet the byte
    comparison: a UB and its prefix (the empty UB included) must be told apart there — a second round, and the grouping of
    oracle/prep.py.  Each family of a cell calls differently, so two families taken for one change the cell's counts."""
    monkeypatch.setenv("VTX_PREP_WEAK_ROUNDS", "1")
    raw = prefix_batch()
    packed, _ = prep.prep_raw(raw, CC.BARCODES, True)
    cfg = config("full", "coverage", 1, 25)
    with lib.Context(cfg, variant="dev") as ctx:
        ctx.set_barcodes(CC.BARCODES)
        stats = ctx.submit_raw(raw)
        recs, begin, count = ctx.fetch_records()
        ctx.run()
        r, a = ctx.fetch_scores()
        got = ctx.fetch_coo()
    assert stats.hash_rounds == 2 and int(stats.kept) == raw.n_records
    assert prep.canonical_records(recs, begin, count) == prep.canonical_records(packed.records, packed.loci["rec_begin"], packed.loci["rec_count"])
    assert len(np.unique(recs["umi_id"])) == 4 + 2 + 2
    entries, _ = CM.run([(4, 0, len(recs))], list(zip(recs["cell_index"].tolist(), recs["umi_id"].tolist())), r, a, 25, 1, CM.COVERAGE)
    assert [e[:5] for e in entries] == [(4, 0, 2, 1, 1), (4, 1, 1, 1, 0), (4, 2, 1, 1, 0)]
    CM.assert_same(got, CM.as_arrays(entries), "prefix UBs under a colliding hash")
