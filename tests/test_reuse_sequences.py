"""The sequences of tests/reuse_util.py are what tests/test_gpu_context_reuse.py assumes — checked without a device.

Record cap.  oracle.batch_scores(..., threads=8) over EVERY step of a sequence, banded and full flavour (the GPU test needs both for
a banded sequence: the scores and the stage invariant), measured on the build machine's CPU:
    unlike-banded-coverage-umi0   2.7 s  (31 338 records)
    unlike-banded-alt_frac-umi1   2.0 s  (31 338 records)
    unlike-full-consensus-umi0    1.0 s  (31 306 records; full flavour only)
    rare-paths                    1.1 s  (14 412 records)
10 s of oracle time per sequence is the budget; at the measured rate (11 500 records per second through both flavours) that is more
than 100 000 records, and RECORD_CAP = 60 000 keeps every sequence well inside it (the steps that repeat an earlier batch reuse its oracle result but count here)."""
import numpy as np
import pytest

import reuse_util as RU
from oracle import oracle
from vartrix_amd.abi import default_config

RECORD_CAP = 60_000


@pytest.fixture(scope="module")
def seqs(oracle_lib):
    return RU.sequences()


def test_every_step_is_a_valid_batch_under_one_barcode_count(seqs):
    assert set(seqs) == {"unlike-banded-coverage-umi0", "unlike-banded-alt_frac-umi1", "unlike-full-consensus-umi0", "rare-paths"}
    for name, seq in seqs.items():
        for label, batch in seq["steps"]:
            RU.validate_packed(batch, seq["n_barcodes"])
        total = sum(b.n_records for _, b in seq["steps"])
        assert 0 < total <= RECORD_CAP, (name, total)


@pytest.mark.parametrize("name", ["unlike-banded-coverage-umi0", "unlike-banded-alt_frac-umi1", "unlike-full-consensus-umi0"])
def test_unlike_steps_hold_what_they_are_there_for(seqs, name):
    seq = seqs[name]
    steps = dict(seq["steps"])
    labels = [l for l, _ in seq["steps"]]
    assert [l.split()[0] for l in labels] == ["1", "2a", "2b", "3", "4", "5", "6", "7", "8", "9"]
    sizes = [b.n_records for _, b in seq["steps"]]
    running = np.maximum.accumulate(sizes)
    # small after big: the tiny batch (twice), the empty one, the edge cases
    for k in (3, 4, 7, 8):
        assert sizes[k] * 50 < running[k - 1], (labels[k], sizes[k], running[k - 1])
    assert 10 <= sizes[3] <= 30 and steps["3 tiny clean"].n_loci == 4        # (4 loci x 5 reads: the depth is drawn per locus)
    assert sizes[4] == 0 and steps["4 empty"].n_loci == 0
    assert steps["8 tiny clean again"] is steps["3 tiny clean"] and steps["9 noisy indels again"] is steps["1 noisy indels"]
    assert 10_000 < sizes[0] == sizes[9]
    # step 1: ragged read lengths, and the band matters
    noisy = steps["1 noisy indels"]
    assert len(np.unique(noisy.records["read_len"])) > 20
    rb, ab = oracle.batch_scores(noisy, default_config(aligner="banded", n_barcodes=seq["n_barcodes"]), threads=8)
    rf, af = oracle.batch_scores(noisy, default_config(aligner="full", n_barcodes=seq["n_barcodes"]), threads=8)
    assert (rb != rf).any() or (ab != af).any()
    assert np.all(rb <= rf) and np.all(ab <= af)
    if seq["umi"]:
        assert len(np.unique(noisy.records["umi_id"])) > 100
    # step 5: long haplotypes first, in the middle, last — few enough for the two-pass split (vtx_run: n_long * 8 <= n_loci)
    mixed = steps["5 mixed with long haplotypes"]
    is_long = np.maximum(mixed.loci["ref_len"], mixed.loci["alt_len"]) > 255
    pos = np.nonzero(is_long)[0]
    assert len(pos) == 3 and pos[0] == 0 and pos[-1] == mixed.n_loci - 1 and 100 < pos[1] < 200
    assert 200 < mixed.n_loci and len(pos) * 8 <= mixed.n_loci
    # step 6: beyond the fast limits
    far = steps["6 beyond the fast limits"]
    assert int(far.records["read_len"].max()) == 3000 > 1024 and int(far.loci["alt_len"].max()) == 5400
    assert int((far.records["read_len"] <= 150).sum()) >= 8
    # step 7: a locus without reads, an empty read, a tie locus (REF == ALT)
    edge = steps["7 edge cases"]
    assert (edge.loci["rec_count"] == 0).any() and (edge.records["read_len"] == 0).any()
    l2 = edge.loci[2]
    assert bytes(edge.hap_arena[l2["ref_off"]:l2["ref_off"] + l2["ref_len"]]) == bytes(edge.hap_arena[l2["alt_off"]:l2["alt_off"] + l2["alt_len"]])
    # step 2: low-entropy sequence
    for label in ("2a repeat-rich", "2b poly-A / tandem"):
        b = steps[label]
        reads = [bytes(b.read_arena[r["read_off"]:r["read_off"] + r["read_len"]]) for r in b.records]
        assert any(b"AAAAAAAAAAAA" in x or b"ACACACACACAC" in x or b"ATATATATATAT" in x for x in reads), label


def test_rare_path_steps_alternate_big_and_small(seqs):
    sizes = [b.n_records for _, b in seqs["rare-paths"]["steps"]]
    assert len(sizes) == 4 and sizes[1] * 20 < sizes[0] and sizes[1] * 20 < sizes[2] and sizes[3] * 4 < sizes[1]
    big1 = seqs["rare-paths"]["steps"][0][1]
    assert (big1.hap_arena >= 0x80).any() or np.isin(big1.read_arena, np.frombuffer(b"N", np.uint8)).any()     # the sweep declines such tasks
