"""The call stage on the CPU: tests/call_model.py (written from reference src/main.rs:1019-1164) against the oracle's reduce
(vtxo_batch_reduce), on the authored batches of tests/call_cases.py, in all 3 modes x UMI on / off x 5 values of min_score.

  * every authored read has the score its construction promises (the oracle's aligners, full and banded);
  * the ledger of the model is complete: every class tests/call_cases.py lists for the configuration was passed through;
  * the oracle equals the model entry for entry, values as bit patterns;
  * the raw form (tag bytes, shuffled), prepared by oracle/prep.py, gives the same entries as the id form.
tests/test_gpu_calls.py holds the device to the same model."""
import numpy as np
import pytest

import call_cases as CC
import call_model as CM
from oracle import oracle, prep
from vartrix_amd.abi import default_config

MODES = ("consensus", "alt_frac", "coverage")
CONFIGS = [(mode, umi, m) for mode in MODES for umi in (0, 1) for m in CC.MIN_SCORES]
assert len(CONFIGS) == 30


def model_of(case, batch, scores, mode, umi, m):
    return CM.run(case.model_loci(batch), case.model_records(batch), scores[0], scores[1], m, umi, MODES.index(mode), case.n_barcodes)


@pytest.mark.parametrize("aligner", ["full", "banded"])
def test_every_authored_read_has_the_promised_scores(aligner):
    for case in CC.cases():
        r, a = case.oracle_scores(aligner)
        bad = np.nonzero((r != case.promise[:, 0]) | (a != case.promise[:, 1]))[0]
        assert bad.size == 0, "%s: record %d scores %d / %d, its construction promises %s" % (case.name, bad[0], r[bad[0]], a[bad[0]], case.promise[bad[0]])
        assert int(case.batch.records["read_len"].max()) <= 150


def test_batch_shapes():
    main, n256, n257, unsorted = CC.cases()
    assert (main.n % 256, n256.n, n257.n) == (2, 256, 257) and main.n < 5000
    assert set(CC.raw_ledger(CC.raw_form(main))) == set(CC.RAW_LEDGER)
    assert len(CC.LEDGER) == len({name for name, _ in CC.LEDGER}) == 5 + 164 + 2 + 27 + 10 + 2 + 12


@pytest.mark.parametrize("mode,umi,m", CONFIGS)
def test_ledger_is_complete_and_the_oracle_equals_the_model(mode, umi, m):
    cfg = default_config(aligner="full", scoring_mode=mode, use_umi=umi, n_barcodes=CC.N_BARCODES, min_score=m)
    ledger = set()
    for case in CC.cases_for(umi):
        scores = case.oracle_scores("full")
        entries, seen = model_of(case, case.batch, scores, mode, umi, m)
        ledger |= seen
        want = CM.as_arrays(entries)
        CM.assert_same(oracle.batch_reduce(case.batch, cfg, *scores), want, "oracle, %s" % case.name)
        if mode == "consensus":
            assert all(e[2] + e[3] > 0 for e in entries)
        else:
            assert len(entries) == len({(int(l), int(c)) for l, c in zip(
                np.repeat(np.arange(case.batch.n_loci), case.batch.loci["rec_count"]), case.batch.records["cell_index"])})
        # the raw form, prepared on the CPU: the same entries
        if case.name != "unsorted-umi":
            packed, stats = prep.prep_raw(CC.raw_form(case), CC.BARCODES, bool(umi))
            assert stats == {"num_not_cell_bc": 0, "num_non_umi": 0} and packed.n_records == case.n
            raw_entries, _ = model_of(case, packed, case.scores_of(packed.records, "full"), mode, umi, m)
            CM.assert_same(CM.as_arrays(raw_entries), want, "raw form, %s" % case.name)
    missing = CC.required(m, umi) - ledger
    assert not missing, "classes never reached at min_score %d, use_umi %d: %s" % (m, umi, sorted(missing))


def test_the_model_on_the_rule_itself():
    """The 0.75 rule where it is decided by equality, and the order of its two tests (ALT first cannot matter: both fractions
    cannot reach 0.75 at once)."""
    C = CM.collapse
    assert C([CM.REF] * 3 + [CM.ALT]) == CM.REF and C([CM.ALT] * 3 + [CM.REF]) == CM.ALT
    assert C([CM.REF] * 6 + [CM.ALT] * 2) == CM.REF and C([CM.REF] * 5 + [CM.ALT] * 3) == CM.UNKNOWN
    assert C([CM.REF] * 3 + [CM.UNKNOWN]) == CM.REF and C([CM.REF] * 2 + [CM.ALT, CM.UNKNOWN]) == CM.UNKNOWN
    assert C([CM.ALT] * 225 + [CM.REF] * 75) == CM.ALT and C([CM.ALT] * 224 + [CM.REF] * 76) == CM.UNKNOWN
    assert CM.evaluate(24, 25, 25) == CM.ALT and CM.evaluate(24, 24, 25) is None and CM.evaluate(25, 25, 25) == CM.UNKNOWN
    assert CM.evaluate(0, 0, 0) == CM.UNKNOWN and CM.evaluate(150, 144, 151) is None
