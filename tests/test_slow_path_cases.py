"""The premises of tests/slow_path_util.py, proved from the CPU oracle alone: what tests/test_gpu_slow_path.py feeds the exact slow
path (slow_align_kernel, run_slow) really has the match counts, rungs, empty seeds, band effects and lengths its cases are named
after — so that a pass on the device means what the test says."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import slow_path_util as U  # noqa: E402
from oracle import oracle  # noqa: E402
from vartrix_amd.abi import default_config  # noqa: E402


@pytest.mark.parametrize("target", sorted(U.MATCH_COUNT_AB))
def test_match_count_pair_has_exactly_the_target_matches(target):
    batch, info = U.match_count_pair(target)
    assert batch.n_records == 1 and info["slow"].all()
    assert U.match_counts(batch).tolist() == [target, target] == info["M"].tolist()
    a, b = U.MATCH_COUNT_AB[target]
    assert (a - 5) * (b - 5) == target
    # the pairs straddle the slab capacities of run_slow
    assert U.rung(target) == sum(target > c for c in (1024, 16384, 262144))


def test_match_count_targets_straddle_every_capacity():
    assert sorted(U.MATCH_COUNT_AB) == [c + d for c in U.SLAB_CAPS for d in (0, 1)]
    assert [U.rung(t) for t in sorted(U.MATCH_COUNT_AB)] == [0, 1, 1, 2, 2, 3]


@pytest.mark.parametrize("top_tasks", [2, 1])
def test_ladder_batch_rung_census(top_tasks):
    batch, info = U.ladder_batch(top_tasks)
    rungs = np.array([U.rung(m) for m in info["M"]])
    census = np.bincount(rungs, minlength=4)
    print("ladder: %d tasks, M %s, per rung %s" % (len(rungs), info["M"].tolist(), census.tolist()))
    assert info["slow"].all() and 20 <= len(rungs) <= 32
    assert (census[:3] >= 2).all() and census[3] == top_tasks
    assert batch.n_loci >= 4
    # no fast locus: the stages in front of run_slow count what they count for a one-record slow batch
    assert int(np.maximum(batch.loci["ref_len"], batch.loci["alt_len"]).min()) > U.FAST_HAP_LEN
    # rounds 2 and 3 each hold more than one task, and their lists are strict, non-contiguous subsets of the lists before them
    for r in (1, 2):
        todo = np.nonzero(rungs >= r)[0]
        before = np.nonzero(rungs >= r - 1)[0]
        assert 1 < len(todo) < len(before)
        assert (np.diff(todo) > 1).any()
    # some record has its two tasks on different rungs
    assert (rungs[0::2] != rungs[1::2]).any()
    # the exact capacities and their successors are all in the batch
    assert set(sorted(U.MATCH_COUNT_AB)[:5]) <= set(info["M"].tolist())


def test_edge_batch_labels_follow_the_rule():
    batch, info = U.edge_batch()
    assert np.array_equal(info["slow"], U.slow_rule(batch))
    tags = info["tags"]
    rl = batch.records["read_len"]
    for ln in (1023, 1024, 1025, 1026):
        rec = int(tags["len%d" % ln][0])
        assert rl[rec] == ln and bool(info["slow"][2 * rec]) == (ln > 1024)
    lens = sorted(zip(batch.loci["ref_len"].tolist(), batch.loci["alt_len"].tolist()))
    assert lens == [(3, 2503), (201, 201), (2400, 2400), (2400, 2401), (2401, 2400), (2401, 2401), (2401, 2401)]
    rec_locus = np.repeat(np.arange(batch.n_loci), batch.loci["rec_count"])
    for l in range(batch.n_loci):
        L = batch.loci[l]
        mine = rl[rec_locus == l]
        assert (mine == 150).sum() >= 2 or int(L["ref_len"]) == 3
        assert (mine == 1024).sum() >= 1
        over = max(int(L["ref_len"]), int(L["alt_len"])) > 2400
        assert info["slow"][np.repeat(rec_locus == l, 2)].all() == over or (mine > 1024).any()
    # both sides of the rule occur, on their own and together
    assert info["slow"].any() and not info["slow"].all()
    assert rl[int(tags["empty"][0])] == 0 and [int(rl[int(tags["len%d" % k][0])]) for k in (1, 5, 6)] == [1, 5, 6]
    for t in ("empty", "len1", "len5", "len6", "no_seed", "n_run", "lower", "iupac", "short_ref"):
        assert info["slow"][2 * tags[t]].all(), t
    x, _ = U.task_sequences(batch, 2 * int(tags["lower"][0]))
    assert x == x.lower() != x.upper()
    x, y = U.task_sequences(batch, 2 * int(tags["iupac"][0]))
    assert x.count(b"R") == 1
    x, y = U.task_sequences(batch, 2 * int(tags["n_run"][0]))
    assert b"N" * 10 in x and b"N" * 11 not in x and b"N" * 12 in y and b"N" * 13 not in y


def test_edge_batch_match_promises_and_empty_seeds():
    batch, info = U.edge_batch()
    M = U.match_counts(batch)
    promised = info["M"] >= 0
    assert promised.sum() == 8                 # (the empty read, the reads of 1 and 5 bases, the read without a shared 6-mer)
    assert np.array_equal(M[promised], info["M"][promised])
    assert info["no_seed"].sum() == 2
    for t in np.nonzero(info["no_seed"])[0]:
        x, y = U.task_sequences(batch, int(t))
        assert len(x) == 150 and M[t] == 0 and set(x) <= set(b"ACGT")
        assert oracle.sw_banded(x, y) == oracle.sw_full(x, y)
    # the N run: its k-mers match each other (5 in the read x 7 in the haplotype, besides the flanks' own)
    t = 2 * int(info["tags"]["n_run"][0])
    assert M[t] >= 35 + 100
    # the lower-case read shares nothing with the upper-case haplotypes either; the 3-base REF has no k-mer at all
    assert M[2 * int(info["tags"]["lower"][0])] == 0
    assert (M[2 * info["tags"]["short_ref"]] == 0).all() and (M[2 * info["tags"]["short_ref"] + 1] > 0).all()


def test_band_matters_batches_are_slow_and_the_band_changes_scores():
    batches = U.band_matters_batches()
    assert len(batches) == 2
    for batch, nb in batches:
        assert 2 * batch.n_records == 96
        assert int(np.minimum(batch.loci["ref_len"], batch.loci["alt_len"]).min()) > 2400 and U.slow_rule(batch).all()
        assert int(np.maximum(batch.loci["ref_len"], batch.loci["alt_len"]).max()) <= 2 * 1300 + 21
        bref, balt = oracle.batch_scores(batch, default_config(aligner="banded", n_barcodes=nb), threads=8)
        fref, falt = oracle.batch_scores(batch, default_config(aligner="full", n_barcodes=nb), threads=8)
        n_diff = int((bref != fref).sum() + (balt != falt).sum())
        print("band matters: %d of %d tasks differ" % (n_diff, 2 * batch.n_records))
        assert n_diff >= 4


def test_limit_batches_have_the_lengths_they_name():
    L = U.limit_batches()
    want = {"a": (30000, 30000, 30000), "a_small": (30000, 2401, 2401), "b": (30000, 201, 201), "c": (1025, 30000, 30000),
            "read_30001": (30001, 30000, 30000), "ref_30001": (30000, 30001, 30000), "alt_30001": (30000, 30000, 30001)}
    assert set(L) == set(want)
    for name, (rl, ref_len, alt_len) in want.items():
        batch, flavours = L[name]
        assert batch.n_records == 1 and batch.n_loci == 1
        assert (int(batch.records["read_len"][0]), int(batch.loci["ref_len"][0]), int(batch.loci["alt_len"][0])) == (rl, ref_len, alt_len)
        assert U.slow_rule(batch).all()
    assert L["a"][1] == ("banded",) and L["b"][1] == ("banded", "full") and L["c"][1] == ("banded",)
    assert U.MAX_LEN == 30000
    # (a): three rounds of the slab ladder; its fallback: two
    Ma, Ms = U.match_counts(L["a"][0]), U.match_counts(L["a_small"][0])
    print("limit (a): M %s; (a_small): M %s" % (Ma.tolist(), Ms.tolist()))
    assert all(U.rung(m) == 2 for m in Ma) and all(U.rung(m) == 2 for m in Ms)
    # the 40-base deletion and the substitutions are in the read: its score stays far below its length, far above a chance hit
    x, y = U.task_sequences(L["a"][0], 0)
    assert 20000 < oracle.sw_banded(x, y) < 29000


def test_even_offsets_keeps_the_batch():
    batch, info = U.edge_batch()
    keep = np.ones(batch.n_records, bool)
    keep[info["tags"]["lower"]] = False
    eb = U.even_offsets(batch, keep)
    assert eb.n_records == batch.n_records - 1 and not (eb.records["read_off"] & 1).any()
    kept = np.nonzero(keep)[0]
    for i in (0, 5, len(kept) - 1):
        assert U.task_sequences(eb, 2 * i + 1) == U.task_sequences(batch, 2 * int(kept[i]) + 1)
    assert int(eb.loci["rec_count"].sum()) == eb.n_records
    eb.to_nibbles()
