"""The exact slow path on the device (slow_align_kernel, run_slow: records with a read above 1 024 bases or a haplotype above 2 400)
against the CPU oracle: the edges of the classification rule, the slab regrowth loop at its exact capacities and with several rungs in
one batch, the band in the banded flavour, the hard limits (30 000 bases accepted, 30 001 refused) and the degenerate tasks.  The case
builders are tests/slow_path_util.py; tests/test_slow_path_cases.py proves their premises on the CPU.

Every run goes through lib.Context with the scores poisoned first and the stage trace on; every comparison is of all scores of both
haplotypes with oracle.batch_scores and of the triplets with oracle.batch_reduce, in coverage mode without UMIs and in alt_frac mode
with UMIs."""
import os
import sys

import numpy as np
import pytest

from oracle import oracle
from vartrix_amd import abi, lib, synth
from vartrix_amd.abi import default_config

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import slow_path_util as U  # noqa: E402

POISON = -4242
MODES = (("coverage", 0), ("alt_frac", 1))
ALIGNERS = ("banded", "full")
_oracle_cache = {}


def oracle_scores(key, batch, aligner, nb):
    """oracle.batch_scores, computed once per (case, flavour) and shared among the tests."""
    k = (key, aligner)
    if k not in _oracle_cache:
        r, a = oracle.batch_scores(batch, default_config(aligner=aligner, n_barcodes=nb), threads=8)
        r.setflags(write=False)
        a.setflags(write=False)
        _oracle_cache[k] = (r, a)
    return _oracle_cache[k]


def run_on(ctx, batch):
    ctx.set_stage_trace(True)
    ctx.set_poison(POISON)
    ctx.submit(batch)
    ctx.run()
    ref, alt = ctx.fetch_scores()
    return ref, alt, ctx.fetch_coo(), ctx.fetch_stage(), ctx.timing().sw_launches


def assert_scores(ref, alt, oref, oalt, what):
    assert not (ref == POISON).any() and not (alt == POISON).any(), "%s: a score was never written" % what
    bad = np.nonzero((ref != oref) | (alt != oalt))[0]
    assert bad.size == 0, "%s: %d mismatches, first at record %d: device (%d, %d) oracle (%d, %d)" % (
        what, bad.size, bad[0], ref[bad[0]], alt[bad[0]], oref[bad[0]], oalt[bad[0]])


def assert_coo(coo, batch, cfg, oref, oalt, what):
    ocoo = oracle.batch_reduce(batch, cfg, oref, oalt)
    for k in ("row", "col", "alt", "ref", "unk", "ref_value"):
        assert np.array_equal(coo[k], ocoo[k]), "%s: %s" % (what, k)
    assert np.array_equal(coo["value"].view(np.uint64), ocoo["value"].view(np.uint64)), what      # (alt_frac may hold NaN: bit patterns)


def check(key, batch, nb, aligner, ctxs=None, modes=MODES):
    """The batch in both modes of `modes` against the oracle -> (ref, alt, stage, sw_launches) of the last run.  ctxs: a dict of
    contexts to reuse, keyed by mode."""
    oref, oalt = oracle_scores(key, batch, aligner, nb)
    out = None
    for mode, umi in modes:
        cfg = default_config(aligner=aligner, scoring_mode=mode, use_umi=umi, n_barcodes=nb)
        what = "%s, %s, %s" % (key, aligner, mode)
        if ctxs is not None:
            if mode not in ctxs:
                ctxs[mode] = lib.Context(cfg)
            ref, alt, coo, stage, launches = run_on(ctxs[mode], batch)
        else:
            with lib.Context(cfg) as ctx:
                ref, alt, coo, stage, launches = run_on(ctx, batch)
        assert_scores(ref, alt, oref, oalt, what)
        assert_coo(coo, batch, cfg, oref, oalt, what)
        if out is not None:
            assert np.array_equal(out[2], stage) and out[3] == launches, what
        out = (ref, alt, stage, launches)
    return out


def close_all(ctxs):
    for c in ctxs.values():
        c.close()


def check_edge_batch(aligner, ctxs=None):
    batch, info = U.edge_batch()
    ref, alt, stage, _ = check("edge", batch, info["n_barcodes"], aligner, ctxs)
    assert np.array_equal(stage == abi.STAGE_SLOW, info["slow"]), "tasks on the slow path: %s, labelled slow: %s" % (
        np.nonzero(stage == abi.STAGE_SLOW)[0].tolist(), np.nonzero(info["slow"])[0].tolist())
    return ref, alt, stage


@pytest.mark.parametrize("aligner", ALIGNERS)
def test_fast_limit_edges(aligner):
    """edge_batch: reads of 1 023 .. 1 026 bases on a 201-base locus, haplotype pairs of 2 400 / 2 401 bases (both, REF only, ALT only),
    a 3-base REF beside a 2 503-base ALT, and on a 2 401-base locus the degenerate reads (empty, 1 / 5 / 6 bases, no shared 6-mer, an
    N run, lower case, an IUPAC byte).  Every score equals the oracle's, none is left at the poison, and the stage is STAGE_SLOW for
    exactly the tasks that `rl > 1024 || max(ref_len, alt_len) > 2400` names."""
    batch, info = U.edge_batch()
    ref, alt, stage = check_edge_batch(aligner)
    tags = info["tags"]
    assert ref[tags["empty"][0]] == 0 and alt[tags["empty"][0]] == 0
    assert ref[tags["len6"][0]] == 6 and ref[tags["len5"][0]] == 5 and ref[tags["len1"][0]] == 1
    assert ref[tags["lower"][0]] == 0                                # byte equality: lower case matches nothing
    assert ref[tags["len1024"][0]] > 150 and ref[tags["len1025"][0]] > 150


@pytest.mark.parametrize("aligner", ALIGNERS)
def test_fast_limit_edges_raw_and_nibbles(aligner):
    """The same batch through vtx_submit_raw (tag bytes, records in any order inside a locus) and with the read arena as nibbles,
    through both submits — without the lower-case read, which the nibble alphabet cannot hold.  Scores and stages are those of the
    byte submit; the raw path's, whose record order inside a (cell, UMI) group is its own, as multisets per locus.  (The full flavour's
    run of this batch is 0.6 s of device time: the byte submit runs in coverage mode, the nibble submit in both modes, the raw batch as
    bytes in coverage mode and as nibbles in alt_frac mode with UMIs.)"""
    full_batch, info = U.edge_batch()
    keep = np.ones(full_batch.n_records, bool)
    keep[info["tags"]["lower"]] = False
    batch = U.even_offsets(full_batch, keep)
    assert batch.n_records == full_batch.n_records - 1
    with pytest.raises(ValueError):
        abi.pack_nibbles(U.even_offsets(full_batch).read_arena)       # the lower-case read is what does not fit
    slow = U.slow_rule(batch)
    nb = info["n_barcodes"]
    want_ref, want_alt, want_stage, _ = check("edge_even", batch, nb, aligner, modes=MODES[:1])
    assert np.array_equal(want_stage == abi.STAGE_SLOW, slow)
    nib = batch.to_nibbles()
    assert nib.read_format == abi.READS_NIBBLES
    ref, alt, stage, _ = check("edge_even", nib, nb, aligner)
    assert np.array_equal(ref, want_ref) and np.array_equal(alt, want_alt) and np.array_equal(stage, want_stage)
    rec_locus = np.repeat(np.arange(batch.n_loci), batch.loci["rec_count"])

    def per_locus(r, a, st):
        rows = np.stack([rec_locus, r, a, st[0::2], st[1::2]], axis=1)
        return rows[np.lexsort(rows.T[::-1])]

    for mode, umi in MODES:
        cfg = default_config(aligner=aligner, scoring_mode=mode, use_umi=umi, n_barcodes=nb)
        raw, barcodes = synth.make_raw(batch, nb, use_umi=bool(umi), seed=5, frac_unlisted=0.0, frac_no_umi=0.0)
        raw_nib = abi.RawBatch(raw.loci, raw.records, raw.hap_arena, abi.pack_nibbles(raw.read_arena), raw.tag_arena, abi.READS_NIBBLES)
        oref, oalt = oracle_scores("edge_even", batch, aligner, nb)
        for rb in ((raw,) if umi == 0 else (raw_nib,)):                # (bytes in coverage mode, nibbles in alt_frac mode with UMIs)
            with lib.Context(cfg) as ctx:
                ctx.set_stage_trace(True)
                ctx.set_poison(POISON)
                ctx.set_barcodes(barcodes)
                stats = ctx.submit_raw(rb)
                assert int(stats.kept) == batch.n_records
                ctx.run()
                r, a = ctx.fetch_scores()
                coo, st = ctx.fetch_coo(), ctx.fetch_stage()
            assert not (r == POISON).any() and not (a == POISON).any()
            assert np.array_equal(per_locus(r, a, st), per_locus(want_ref, want_alt, want_stage))
            assert_coo(coo, batch, cfg, oref, oalt, "raw, %s, %s" % (aligner, mode))


# sw_launches of a batch whose every haplotype is above 2 400 bases, before run_slow's own rounds (vtx_api.hip).  Banded flavour:
# run_banded makes one BandPass over all tasks; max_hap_len, the longest FAST haplotype, is 0, so the pass is not on the sweep path:
# diag_stage -> diag_round3_path counts band_diag_kernel once (no refine record), run_stage counts band_run_kernel + masked DP once
# (both kernels skip the tasks of slow records): 2.  Full flavour: run_full_dp counts one per bucket of fast records: 0.  run_slow then
# adds one per round.  (A batch with fast loci beside slow records takes other stages in front, so its base differs.)
BASE_LAUNCHES = {"banded": 2, "full": 0}


def test_slab_regrowth_at_exact_capacity():
    """match_count_pair(cap) and (cap + 1) for the three slab capacities of run_slow (1 024, 16 384, 262 144 matches), banded flavour:
    M == cap fits the slab, M == cap + 1 is listed for the next round (band_task: `M > m_cap`).  Both equal the oracle;
    timing().sw_launches is BASE_LAUNCHES + 1 + rung: 3 / 4, 4 / 5, 5 / 6 for the three pairs, so the second of a pair is exactly one
    above the first, and the count never falls from rung to rung.  The full flavour has no match list: one round whatever M is."""
    seen = []
    for cap in U.SLAB_CAPS:
        pair = []
        for target in (cap, cap + 1):
            batch, info = U.match_count_pair(target)
            # (the 262 144 pair takes 0.8 - 0.9 s of one lane per run: coverage mode only; the triplets of a one-record batch in
            # alt_frac mode with UMIs are compared on the four smaller targets)
            ref, alt, stage, launches = check("M%d" % target, batch, info["n_barcodes"], "banded", modes=MODES if cap < U.SLAB_CAPS[2] else MODES[:1])
            assert (stage == abi.STAGE_SLOW).all()
            print("M = %d: sw_launches %d" % (target, launches))
            pair.append(launches)
            assert launches == BASE_LAUNCHES["banded"] + 1 + U.rung(target)
        assert pair[1] == pair[0] + 1
        seen += pair
    assert all(b >= a for a, b in zip(seen, seen[1:]))
    for target in (U.SLAB_CAPS[0], U.SLAB_CAPS[0] + 1, U.SLAB_CAPS[1] + 1):
        batch, info = U.match_count_pair(target)
        _, _, stage, launches = check("M%d" % target, batch, info["n_barcodes"], "full", modes=MODES[:1])
        assert (stage == abi.STAGE_SLOW).all() and launches == BASE_LAUNCHES["full"] + 1


def test_regrowth_ladder_in_one_batch():
    """ladder_batch, banded flavour: 26 slow tasks on all four rungs of the slab ladder in one batch, records of one locus on
    different rungs, REF and ALT of one record on different rungs — the retry list of every round is a strict, non-contiguous subset
    of the one before, in the other half of the retry buffer, and the slot of a task is its position in that list.  Task for task the
    oracle's scores; sw_launches is that of the deepest rung alone (BASE_LAUNCHES + 4 rounds); a second run on the same context (slab
    and retry buffer reused, at their largest) and a run on a fresh one give the same scores.  (One run is 1.75 s of device time, the
    M = 262 656 and 279 040 tasks through four rounds: three runs — coverage mode twice on one context, alt_frac with UMIs on the
    fresh one.)"""
    batch, info = U.ladder_batch()
    nb = info["n_barcodes"]
    deepest = max(U.rung(m) for m in info["M"])
    assert deepest == 3
    ctxs = {}
    try:
        first = check("ladder", batch, nb, "banded", ctxs, modes=MODES[:1])
        assert (first[2] == abi.STAGE_SLOW).all()
        assert first[3] == BASE_LAUNCHES["banded"] + 1 + deepest
        again = check("ladder", batch, nb, "banded", ctxs, modes=MODES[:1])
    finally:
        close_all(ctxs)
    fresh = check("ladder", batch, nb, "banded", modes=MODES[1:])
    for other in (again, fresh):
        assert np.array_equal(first[0], other[0]) and np.array_equal(first[1], other[1]) and np.array_equal(first[2], other[2])
        assert first[3] == other[3]


def test_band_is_honoured_on_the_slow_path():
    """band_matters_batches: repeat-rich loci whose every haplotype is above 2 400 bases, so every task is slow, and on which the band
    lowers a few scores below the full matrix's.  Each flavour equals its own oracle, and the device's banded and full scores differ
    on exactly the tasks where the oracle's do (slow_align_kernel scoring the whole matrix in the banded flavour would pass every
    other slow-path test of this suite)."""
    for i, (batch, nb) in enumerate(U.band_matters_batches()):
        got = {}
        for aligner in ALIGNERS:
            ref, alt, stage, _ = check("band%d" % i, batch, nb, aligner)
            assert (stage == abi.STAGE_SLOW).all()
            got[aligner] = np.stack([ref, alt])
        want = {al: np.stack(oracle_scores("band%d" % i, batch, al, nb)) for al in ALIGNERS}
        dev_diff, ora_diff = got["banded"] != got["full"], want["banded"] != want["full"]
        print("batch %d: banded != full on %d tasks" % (i, int(dev_diff.sum())))
        assert ora_diff.sum() >= 4 and np.array_equal(dev_diff, ora_diff)
        assert (got["banded"] <= got["full"]).all()


@pytest.mark.parametrize("case,aligner", [("a", "banded"), ("a_small", "banded"), ("b", "banded"), ("b", "full"), ("c", "banded")])
def test_hard_limits_accepted(case, aligner):
    """30 000 bases, the longest read and the longest haplotype the library takes (kMaxReadLen, kMaxHapLen: the 16-bit chain, range and
    band arrays, the i << 16 | j match words and the 0xffff / 0x7fff sentinels of the slow path are sized by it): (a) read and both
    haplotypes at the limit, banded, three rounds of the slab ladder; (b) the read at the limit on a 201-base locus, both flavours;
    (c) the haplotypes at the limit under a 1 025-base read, banded.  (a) is 3.1 s of one lane per run (M = 2.5e5 matches through the
    chaining, 30 000 columns of band): it runs in coverage mode only, and (a_small), the same read on 2 401-base haplotypes, in both."""
    batch, flavours = U.limit_batches()[case]
    assert aligner in flavours
    ref, alt, stage, launches = check("limit_" + case, batch, 2, aligner, modes=MODES[:1] if case == "a" else MODES)
    assert (stage == abi.STAGE_SLOW).all()
    print("limit (%s), %s: scores (%d, %d), sw_launches %d" % (case, aligner, ref[0], alt[0], launches))
    if case == "a":
        assert launches == BASE_LAUNCHES["banded"] + 3 and ref[0] > 20000
    if case == "b":
        assert ref[0] > 150


def test_hard_limits_refused():
    """30 001 bases: vtx_submit refuses the batch with VTX_E_UNSUPPORTED and names the record (a read) or the locus (a haplotype, REF
    or ALT); vtx_submit_raw refuses the read with VTX_E_INVAL.  After each refusal the same context takes edge_batch and gives the
    oracle's scores (banded contexts in both modes after every refusal; a full-flavour one, whose edge_batch is 0.6 s of device time,
    after all four)."""
    L = U.limit_batches()
    nb = U.edge_batch()[1]["n_barcodes"]
    raw, barcodes = synth.make_raw(L["read_30001"][0], nb, use_umi=False, frac_unlisted=0.0, frac_no_umi=0.0)

    def refuse(ctx, name, word):
        with pytest.raises(lib.VtxError) as e:
            ctx.submit(L[name][0])
        assert e.value.status == abi.VTX_E_UNSUPPORTED, str(e.value)
        assert word in str(e.value) and "30000" in str(e.value), str(e.value)

    def refuse_raw(ctx):
        ctx.set_barcodes(barcodes)
        with pytest.raises(lib.VtxError) as e:
            ctx.submit_raw(raw)
        assert e.value.status == abi.VTX_E_INVAL and "30000" in str(e.value), str(e.value)

    cases = (("read_30001", "record 0"), ("ref_30001", "locus 0"), ("alt_30001", "locus 0"))
    ctxs = {}
    try:
        check_edge_batch("banded", ctxs)                                  # (creates the contexts: one per mode)
        for name, word in cases:
            for ctx in ctxs.values():
                refuse(ctx, name, word)
            check_edge_batch("banded", ctxs)
        for ctx in ctxs.values():
            refuse_raw(ctx)
        check_edge_batch("banded", ctxs)
    finally:
        close_all(ctxs)
    ctxs = {}
    try:
        ctxs["coverage"] = lib.Context(default_config(aligner="full", scoring_mode="coverage", use_umi=0, n_barcodes=nb))
        for name, word in cases:
            refuse(ctxs["coverage"], name, word)
        refuse_raw(ctxs["coverage"])
        batch, info = U.edge_batch()
        _, _, stage, _ = check("edge", batch, nb, "full", ctxs, modes=MODES[:1])
        assert np.array_equal(stage == abi.STAGE_SLOW, info["slow"])
    finally:
        close_all(ctxs)
