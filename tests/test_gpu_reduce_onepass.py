"""The call reduction in one pass over the scores — reduce_count_kernel, the scan of its per-block counts, reduce_emit_kernel
(vtx_kernels.hip; one thread per (row, cell) group, vtx_call_core.h) — against the histogram kernels it stands in for on batches of
short groups (count_calls_kernel .. emit_coo_kernel; VTX_REDUCE_LEGACY=1 in the developer library) and against tests/call_model.py
run on the oracle's scores.  Every comparison is exact: integers, and bit patterns for the values (NaN included).

The kernels cut the GROUPS into blocks of 256 (the histogram kernels cut the records), so the block edges here are group counts:
1, 255, 256, 257 and 513 groups (1, 2 and 3 words for the scan), blocks that keep 0, 1 and all 256 of their groups.  The batches of
tests/call_cases.py bring the record-index edges (heads and the last record on 255 / 256 / 257), the 600-record group and the 300-read
family.  Which path a run took is read from the developer library (vtx_dev_reduce_path: 1 histogram, 2 one pass), never timed."""
import ctypes as C

import numpy as np
import pytest
import torch

import call_cases as CC
import call_model as CM
from vartrix_amd import lib, shard
from vartrix_amd.abi import LOCUS_DTYPE, RECORD_DTYPE, PackedBatch, default_config

pytestmark = pytest.mark.gpu
MODES = ("consensus", "alt_frac", "coverage")
LEGACY, ONEPASS = 1, 2
BLOCK = 256
MEAN_MAX = 4                       # kReduceMeanGroupMax (vtx_api.hip)
FORCE = "1000000000"               # VTX_REDUCE_THRESHOLD that sends every batch through the one-pass kernels


def context(mode, umi, m):
    return lib.Context(default_config(aligner="full", scoring_mode=mode, use_umi=umi, n_barcodes=CC.N_BARCODES, min_score=m), variant="dev")


def path_of(ctx):
    f = ctx._L.vtx_dev_reduce_path
    f.restype, f.argtypes = C.c_int, [C.c_void_p]
    return f(ctx._h)


def model(case, mode, umi, m):
    r, a = case.oracle_scores("full")
    entries, _ = CM.run(case.model_loci(), case.model_records(case.batch), r, a, m, umi, MODES.index(mode), case.n_barcodes)
    return entries


def run_both(ctx, monkeypatch, case, mode, umi, m, threshold=FORCE):
    """The resident batch through the one-pass kernels and through the histogram kernels of the same context; both against the model.
    -> the model's entries"""
    label = "%s umi %d min_score %d, batch %s" % (mode, umi, m, case.name)
    want = model(case, mode, umi, m)
    ctx.submit(case.batch)
    got = {}
    for name, env, path in (("one pass", {"VTX_REDUCE_THRESHOLD": threshold}, ONEPASS), ("histogram", {"VTX_REDUCE_LEGACY": "1"}, LEGACY)):
        monkeypatch.delenv("VTX_REDUCE_THRESHOLD", raising=False)
        monkeypatch.delenv("VTX_REDUCE_LEGACY", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx.run()
        assert path_of(ctx) == path, (label, name)
        got[name] = ctx.fetch_coo()
        assert ctx.device_coo()["nnz"] == len(want), (label, name)
        CM.assert_same(got[name], CM.as_arrays(want), "%s, %s" % (label, name))
    for k in got["one pass"]:
        assert np.array_equal(got["one pass"][k].view(np.uint8), got["histogram"][k].view(np.uint8)), (label, k)
    return want


@pytest.mark.parametrize("umi", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_one_pass_equals_the_histogram_kernels_and_the_model(mode, umi, monkeypatch):
    for m in (0, 26, 151):
        with context(mode, umi, m) as ctx:
            for case in CC.cases_for(umi):
                want = run_both(ctx, monkeypatch, case, mode, umi, m)
                if mode == "alt_frac" and m == 151:
                    assert want and all(np.isnan(e[5]) for e in want)          # 0 / 0 in every entry


# ---- block edges of the group index ----
KEPT = (lambda i: [CC.R(i)], lambda i: [CC.A(i)], lambda i: [CC.U(i), CC.A(i)], lambda i: [CC.NONE(0), CC.R(i), CC.R(i + 1)])
DROPPED = (lambda i: [CC.U(i)], lambda i: [CC.NONE(0)], lambda i: [CC.U(i), CC.NONE(2)])      # (consensus, min_score 26: no REF / ALT call)


def flags_case(name, keep):
    """One (row, cell) group per flag, 100 cells to a locus; kept groups hold a REF or ALT call, the others none.  Every record is a
    UMI family of its own."""
    loci = []
    for g, kept in enumerate(keep):
        if g % 100 == 0:
            loci.append([])
        reads = (KEPT[g % len(KEPT)] if kept else DROPPED[g % len(DROPPED)])(g)
        loci[-1] += [(g % 100, 10 * g + j, rd) for j, rd in enumerate(reads)]
    return CC.Case(name, [(2 * i + 1, reads) for i, reads in enumerate(loci)])


def edge_patterns():
    out = []
    for ng in (1, 255, 256, 257, 513):
        out.append(("all-%d" % ng, [1] * ng))
        out.append(("none-%d" % ng, [0] * ng))
        out.append(("every-third-%d" % ng, [int(g % 3 == 0) for g in range(ng)]))
    full_none_one = [1] * BLOCK + [0] * BLOCK + [1]                      # block totals 256, 0, 1
    none_last_full = [0] * BLOCK + [0] * (BLOCK - 1) + [1] + [1]         # 0, 1 (its last lane), 1
    first_only = [1] + [0] * (BLOCK - 1) + [0] + [1] * (BLOCK - 1) + [0]  # 1 (its first lane), 255, 0
    out += [("256-0-1", full_none_one), ("0-1-1", none_last_full), ("1-255-0", first_only)]
    return out


_edge_cases = {}


def edge_case(name, keep):
    if name not in _edge_cases:
        _edge_cases[name] = flags_case(name, keep)
    return _edge_cases[name]


@pytest.mark.parametrize("umi", [0, 1])
def test_block_edges_of_the_group_index(umi, monkeypatch):
    totals, words = set(), set()
    with context("consensus", umi, 26) as ctx:
        for name, keep in edge_patterns():
            case = edge_case(name, keep)
            want = run_both(ctx, monkeypatch, case, "consensus", umi, 26)
            # the batch is what it was authored to be: the model keeps exactly the flagged groups
            assert [(e[0], e[1]) for e in want] == [(2 * (g // 100) + 1, g % 100) for g, k in enumerate(keep) if k], name
            per_block = [sum(keep[b:b + BLOCK]) for b in range(0, len(keep), BLOCK)]
            totals |= set(per_block)
            words.add(len(per_block))
    assert {0, 1, BLOCK} <= totals and words == {1, 2, 3}
    with context("alt_frac", umi, 26) as ctx:                            # every group kept, whatever it holds: offset = group index
        for name, keep in edge_patterns():
            if name in ("none-513", "256-0-1", "every-third-257"):
                assert len(run_both(ctx, monkeypatch, edge_case(name, keep), "alt_frac", umi, 26)) == len(keep)


def test_nothing_kept_writes_nothing(monkeypatch):
    """Consensus over a batch whose every read is None, after a batch that left entries: nnz is 0 and no element of the seven output
    arrays is written (they are filled with a pattern before the run that is checked)."""
    monkeypatch.setenv("VTX_REDUCE_THRESHOLD", FORCE)
    first = edge_case("every-third-513", [int(g % 3 == 0) for g in range(513)])
    none = CC.Case("all-none", [(i, [(c, 5, CC.NONE(2 * c + i)) for c in range(100)] + [(100, 6, CC.NONE(0)), (100, 6, CC.NONE(1))]) for i in range(6)])
    assert none.n <= first.n
    for umi in (0, 1):
        with context("consensus", umi, 26) as ctx:
            ctx.submit(first.batch)
            ctx.run()
            assert ctx.device_coo()["nnz"] == len(model(first, "consensus", umi, 26)) > 0
            ctx.submit(none.batch)
            ctx.run()
            d = ctx.device_coo()                                         # (the arrays as they are after this submit)
            assert d["nnz"] == 0
            views = {k: torch.as_tensor(shard._DevArray(d[k], none.n * (1 if dt is np.uint32 else 2), "<i4"), device="cuda:%d" % ctx.cfg.device)
                     for k, dt in shard.COO_FIELDS}
            for v in views.values():
                v.fill_(0x5A5A5A5A)
            torch.cuda.synchronize()
            ctx.run()
            assert path_of(ctx) == ONEPASS
            after = ctx.device_coo()
            assert after["nnz"] == 0 and len(ctx.fetch_coo()["row"]) == 0
            assert model(none, "consensus", umi, 26) == []
            for k, v in views.items():
                assert after[k] == d[k], k                               # (the arrays were not moved: the views are the outputs)
                assert bool((v == 0x5A5A5A5A).all().item()), "output array %s was written" % k


SOLO = 40                          # one-record groups on each side of the deep group: 83 groups, 682 records, mean 8.2


def deep_case():
    """call_cases.main_case's 600-record cell group — its first 300 records one UMI family that is ALT by exactly 0.75 (225 : 75) —
    between one-record groups."""
    big = [(30, 1, CC.A(j) if j % 4 else CC.R(j)) for j in range(300)]
    big += [(30, 2 + j // 3, (CC.R, CC.R, CC.A)[j % 3](j)) for j in range(150)]
    big += [(30, 100 + j // 4, (CC.A, CC.A, CC.A, CC.U)[j % 4](j)) for j in range(150)]
    solo = lambda i: [(c, 7, (CC.R, CC.A, CC.U, CC.NONE)[(c + i) % 4](c)) for c in range(SOLO)]
    return CC.Case("deep", [(0, solo(0)), (1, [(29, 1, CC.R(0))] + big + [(31, 1, CC.R(1))]), (2, solo(1))])


def test_a_deep_group_among_short_ones_on_the_one_pass_path(monkeypatch):
    case = deep_case()
    assert case.n > MEAN_MAX * (2 * SOLO + 3)                            # (the batch's mean alone would send it to the histogram kernels)
    for mode, umi in (("coverage", 1), ("coverage", 0), ("consensus", 1)):
        with context(mode, umi, 26) as ctx:
            want = run_both(ctx, monkeypatch, case, mode, umi, 26)
        big = [e for e in want if (e[0], e[1]) == (1, 30)]
        # the 300-read family is ONE ALT call; 50 families 2 : 1 are UNKNOWN; 37 families 3 : 1 and one 2 : 0 are ALT
        assert [e[2:5] for e in big] == ([(0, 39, 50)] if umi else [(175, 388, 37)]), big


def threshold_cases():
    """50 groups: four records each (mean 4.0), and the same with one None read more in the last group (mean 4.02)."""
    reads = [(c, 10 * c + j, (CC.R, CC.A, CC.U, CC.A)[(c + j) % 4](c + j)) for c in range(50) for j in range(4)]
    return CC.Case("mean-4", [(3, reads)]), CC.Case("mean-over-4", [(3, reads + [(49, 10 * 49 + 3, CC.NONE(0))])])


@pytest.mark.parametrize("mode,umi", [("consensus", 0), ("coverage", 1)])
def test_the_threshold_picks_the_path_and_not_the_result(mode, umi, monkeypatch):
    monkeypatch.delenv("VTX_REDUCE_THRESHOLD", raising=False)
    monkeypatch.delenv("VTX_REDUCE_LEGACY", raising=False)
    under, over = threshold_cases()
    assert under.n == MEAN_MAX * 50 and over.n == MEAN_MAX * 50 + 1
    got = {}
    with context(mode, umi, 26) as ctx:
        for case, path in ((under, ONEPASS), (over, LEGACY), (under, ONEPASS)):
            ctx.submit(case.batch)
            ctx.run()
            assert path_of(ctx) == path, case.name
            got[case.name] = ctx.fetch_coo()
            CM.assert_same(got[case.name], CM.as_arrays(model(case, mode, umi, 26)), case.name)
    for k in got["mean-4"]:
        assert np.array_equal(got["mean-4"][k].view(np.uint8), got["mean-over-4"][k].view(np.uint8)), k
    assert len(got["mean-4"]["row"]) == 50


def test_an_empty_batch_after_a_full_one_has_no_entries(monkeypatch):
    monkeypatch.setenv("VTX_REDUCE_THRESHOLD", FORCE)
    empty = PackedBatch(np.zeros(0, LOCUS_DTYPE), np.zeros(0, RECORD_DTYPE), np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    case = edge_case("all-257", [1] * 257)
    with context("coverage", 1, 26) as ctx:
        for _ in range(2):
            ctx.submit(case.batch)
            ctx.run()
            assert path_of(ctx) == ONEPASS and ctx.device_coo()["nnz"] == 257
            ctx.submit(empty)
            ctx.run()
            assert path_of(ctx) == 0 and ctx.device_coo()["nnz"] == 0 and len(ctx.fetch_coo()["row"]) == 0
