"""An independent model of the call stage — two scores per read in, matrix entries out — for tests/test_call_model.py and
tests/test_gpu_calls.py.

The device (group_heads_kernel .. emit_coo_kernel, values_from_counts_kernel; vartrix_amd/csrc/vtx_kernels.hip) and the oracle
(vtxo_batch_reduce) both restate reference src/main.rs:1019-1164 as passes over flat arrays with head flags and integer
comparisons, so agreement between them proves little.  This file is written from the reference's text alone and differently on
purpose:

  * a locus is cut into runs of equal cell_index (itertools group_by over the sorted scores, :1044);
  * inside a run, calls are collected in a dict keyed by the UMI, as the reference's HashMap (:1047-1057) — the order of the records
    inside a run therefore cannot matter, and neither can the UMI when use_umi is off;
  * the 0.75 rule is two float divisions compared with 0.75, in the order the reference writes them (:1070-1081);
  * values are Python floats; 0 / 0 is the machine's own double division, as it is in the reference's binary.

run() also returns a LEDGER: the set of classes the input made it pass through (tests/call_cases.py lists the ones a batch has to
reach).  The ledger is how a test knows that a composition it means to pin was really there once the scores were what they were.
"""
import itertools

import numpy as np

REF, ALT, UNKNOWN = 1, 2, -1              # REF_VALUE, ALT_VALUE, UNKNOWN_VALUE (src/main.rs:27-31)
REF_ALT = 3                               # REF_ALT_VALUE
THRESHOLD = 0.75                          # CONSENSUS_THRESHOLD (:32)
CONSENSUS, ALT_FRAC, COVERAGE = 0, 1, 2   # vtx_scoring_mode
BLOCK = 256                               # the device's kernels run one record per thread in blocks of this many
EDGE_NAMES = {BLOCK - 1: "255", 0: "256", 1: "257"}      # a record index modulo BLOCK -> the name of the block-edge position


def evaluate(ref_score, alt_score, min_score):
    """evaluate_scores (:1019-1030): None, or REF / ALT / UNKNOWN."""
    if (ref_score < min_score) & (alt_score < min_score):
        return None
    elif ref_score > alt_score:
        return REF
    elif alt_score > ref_score:
        return ALT
    return UNKNOWN


def counts(calls):
    """convert_to_counts (:1032-1039) -> (ref, alt, unk)"""
    return (sum(1 for c in calls if c == REF), sum(1 for c in calls if c == ALT), sum(1 for c in calls if c == UNKNOWN))


def collapse(calls):
    """One UMI's calls -> its consensus call (:1061-1081).  `calls` is never empty: a UMI enters the map with its first call."""
    r, a, k = counts(calls)
    ref_frac = float(r) / (float(a) + float(r) + float(k))
    alt_frac = float(a) / (float(a) + float(r) + float(k))
    if (ref_frac < THRESHOLD) & (alt_frac < THRESHOLD):
        return UNKNOWN
    elif alt_frac >= THRESHOLD:
        return ALT
    assert ref_frac >= THRESHOLD
    return REF


def divide(a, b):
    """a as f64 / b as f64 with IEEE semantics (Python's own `/` raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def run(loci, records, ref_score, alt_score, min_score, use_umi, mode, n_barcodes=None):
    """loci: (row, rec_begin, rec_count) per locus; records: (cell_index, umi_id) per record; the two score arrays; cfg.min_score,
    cfg.use_umi, cfg.scoring_mode.  -> (entries, ledger): entries = [(row, col, ref, alt, unk, value, ref_value)] in locus order,
    then cell-run order; ledger = a set of class names."""
    ledger = set()
    entries = []
    n = len(records)
    prev = None                            # the last non-empty locus: (locus index, its last record)
    seen_rows = []
    for li, (row, begin, count) in enumerate(loci):
        seen_rows.append((li, row, count))
        if not count:
            continue
        if prev is not None:
            if li - prev[0] > 1:
                ledger.add("edge:empty-locus-between")
            if begin % BLOCK in EDGE_NAMES:
                ledger.add("block:locus-head@" + EDGE_NAMES[begin % BLOCK])
            if records[prev[1]][0] == records[begin][0]:
                ledger.add("edge:cell-across-loci:" + ("same-umi" if records[prev[1]][1] == records[begin][1] else "other-umi"))
        prev = (li, begin + count - 1)
        if row != li:
            ledger.add("edge:row-is-not-the-index")
        at = begin
        prev_run_umis = None
        for cell, run_ in itertools.groupby(range(begin, begin + count), key=lambda i: records[i][0]):
            idx = list(run_)
            if at != begin and at % BLOCK in EDGE_NAMES:
                ledger.add("block:cell-head@" + EDGE_NAMES[at % BLOCK])
            at += len(idx)
            if len(idx) > 2 * BLOCK:
                ledger.add("block:cell-group-over-two-blocks")
            if cell == 0:
                ledger.add("edge:cell-0")
            if n_barcodes is not None and cell == n_barcodes - 1:
                ledger.add("edge:cell-last")
            umis = [records[i][1] for i in idx]
            if prev_run_umis is not None and set(umis) & prev_run_umis:
                ledger.add("edge:umi-in-adjacent-cells")
            prev_run_umis = set(umis)
            if 0 in prev_run_umis:
                ledger.add("edge:umi-0")
            if 2 ** 31 - 1 in prev_run_umis:
                ledger.add("edge:umi-2^31-1")
            if not use_umi and any(x > y for x, y in zip(umis, umis[1:])):
                ledger.add("edge:unsorted-umi-without-umis")
            for i, j in zip(idx, idx[1:]):
                if records[i][1] != records[j][1] and j % BLOCK in EDGE_NAMES:
                    ledger.add("block:umi-head@" + EDGE_NAMES[j % BLOCK])
            # ---- parse_scores (:1041-1109) for this run ----
            evals = []
            for i in idx:
                rs, as_ = int(ref_score[i]), int(alt_score[i])
                e = evaluate(rs, as_, min_score)
                evals.append(e)
                if e is None:
                    ledger.add("call:none")
                else:
                    ledger.add({REF: "call:ref", ALT: "call:alt", UNKNOWN: "call:unknown"}[e])
                    if min(rs, as_) < min_score:
                        ledger.add("call:one-side-under")
            if use_umi:
                by_umi = {}
                members = {}
                for i, e in zip(idx, evals):
                    members[records[i][1]] = members.get(records[i][1], 0) + 1
                    if e is None:
                        continue
                    by_umi.setdefault(records[i][1], []).append(e)
                calls = []
                for umi, n_reads in members.items():
                    if n_reads > BLOCK:
                        ledger.add("block:family-over-one-block")
                    if umi not in by_umi:
                        ledger.add("family:none-only")
                        continue
                    v = by_umi[umi]
                    ledger.add("family:%d,%d,%d" % counts(v))
                    if len(v) < n_reads:
                        ledger.add("family:with-none-reads")
                    calls.append(collapse(v))
            else:
                calls = [e for e in evals if e is not None]
            # ---- consensus_scoring / alt_frac / coverage (:1111-1164) ----
            r, a, k = counts(calls)
            ledger.add("cell:%d,%d,%d" % (min(r, 3), min(a, 3), min(k, 3)))          # (3 stands for "3 or more")
            if mode == CONSENSUS:
                if (r > 0) & (a > 0):
                    entries.append((row, cell, r, a, k, float(REF_ALT), 0.0))
                elif a > 0:
                    entries.append((row, cell, r, a, k, float(ALT), 0.0))
                elif r > 0:
                    entries.append((row, cell, r, a, k, float(REF), 0.0))
            elif mode == ALT_FRAC:
                entries.append((row, cell, r, a, k, divide(a, float(r) + float(a) + float(k)), 0.0))
            else:
                entries.append((row, cell, r, a, k, float(a), float(r)))
    if n and (n - 1) % BLOCK in EDGE_NAMES:
        ledger.add("block:last-record@" + EDGE_NAMES[(n - 1) % BLOCK])
    return entries, ledger


def as_arrays(entries):
    """entries -> the dict of arrays vtx_fetch_coo / oracle.batch_reduce give"""
    cols = list(zip(*entries)) if entries else [()] * 7
    out = {k: np.array(cols[i], np.uint32) for i, k in enumerate(("row", "col"))}
    out["ref"], out["alt"], out["unk"] = (np.array(cols[i], np.uint32) for i in (2, 3, 4))
    out["value"], out["ref_value"] = np.array(cols[5], np.float64), np.array(cols[6], np.float64)
    return out


def assert_same(got, want, label):
    """Entry for entry: counts exact, values as bit patterns (NaN included)."""
    for k in ("row", "col", "ref", "alt", "unk"):
        assert got[k].shape == want[k].shape, "%s: %d entries, the model has %d" % (label, len(got[k]), len(want[k]))
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, "%s: field %s differs at entry %d (row %d col %d): %d, the model has %d" % (
            label, k, bad[0], want["row"][bad[0]], want["col"][bad[0]], got[k][bad[0]], want[k][bad[0]])
    for k in ("value", "ref_value"):
        g, w = got[k].view(np.uint64), want[k].view(np.uint64)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, "%s: field %s differs at entry %d (row %d col %d): %r (%016x), the model has %r (%016x)" % (
            label, k, bad[0], want["row"][bad[0]], want["col"][bad[0]], got[k][bad[0]], g[bad[0]], want[k][bad[0]], w[bad[0]])
