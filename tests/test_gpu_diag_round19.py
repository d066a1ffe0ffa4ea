"""Whole constructed batches through band_diag_kernel, aimed at the code round 19 rewrote (closure_scan's skip mask, packed nearest
match and split counters; pass 1's membership bits and the walk-list append; harmless_item4) and at the paths around it.  Scores are
held to the oracle; what the first stage decides — its verdict, its score, the stage byte, the list a task leaves on — to the CPU build
of the same header (tests/fastcore/recheck_host.cpp through recheck_util.mirror, as tests/test_gpu_recheck.py does).  Every task the
mirror decides must be decided by the first stage on the device.

Two batches: reads of at most 192 bases (the three-word build of the kernel) and one with reads of 193 - 256 bases (the four-word
build); haplotypes of at most 255 bases (two-byte match entries).  One to three loci per case, at most 64 reads each.

Cases (every locus list below names its own):
  twins      haplotypes with 0, 2, 12, 14, 44 and more than 60 twin-list entries (the list holds a pair in both orders, so its length is
             even: 12 fills the head the kernel loads ahead, 14 is the first length with an entry behind it, above 60 there is no
             list), reads at every offset: twin rows in every mask word and below row 0
  overhang   reads of 70, 130, 150 (and 200, 256) bases hanging over the window on either side
  append     a wavefront whose overhangs are copies of haplotype sequence: their rows hit in both haplotypes (counted on the host: more
             than 36 a read), so the hits of one trip pass the walk list's 224 entries (its retry); that a lane gets six blocks with
             all 36 append bits set follows from the construction but is not observed
  short      the batch ends in a wavefront with fewer than 64 tasks
  stub       an ALT of three bases beside a full REF: one lane of every pair never reaches a table
  far        exactly E read k-mers matching D = 3 .. 40 diagonals off the main one, on one side, none on the other and none nearer, with
             E = bound - 1, bound, bound + 1 for the bound of D's bin (E = 1 at D = 3, where any match breaks it): within condition (*)
             and broken by a single match.  The counts are asserted from the batch's bytes.  (A task that breaks the condition is still
             decided as a rule — the repeat joins the generic set —; what the scan answers is pinned by tests/test_gpu_maskops.py.)
  pieces     reads of one to four main pieces with an off-diagonal match (sx, sy) at harmless_item4's equalities: min(sx, sy - d) at,
             one below and one above pu + K; max(sx, sy - d) at, one below and one above pv - 5 - K, for every piece; asserted from the
             batch's bytes"""
import os

import numpy as np
import pytest

import recheck_util as RU
from stress_batches import manual_batch

pytestmark = pytest.mark.gpu
NB = 64
K = 6
STAGE_DIAG_CERT, STAGE_DIAG_DP, STAGE_CORRIDOR_CERT = 1, 7, 11
ACGT = np.frombuffer(b"ACGT", np.uint8)


def twin_entries(h):
    pos = {}
    for y in range(len(h) - K + 1):
        pos.setdefault(bytes(h[y:y + K]), []).append(y)
    return sum(len(v) * (len(v) - 1) for v in pos.values())


def twin_free(rng, n):
    """iid-like bases in which no 6-mer occurs twice: a base that would repeat one is drawn again"""
    while True:
        h, seen = bytearray(), set()
        while len(h) < n:
            for b in rng.permutation(4):
                k = bytes(h[len(h) - K + 1:]) + bytes([ACGT[b]])
                if len(k) < K or k not in seen:
                    h.append(ACGT[b]); seen.add(k)
                    break
            else:
                break                                  # (all four bases repeat a 6-mer: start again)
        if len(h) == n:
            return h


def hap_with_twins(rng, n, want):
    """no twins but `want` twin-list entries exactly (want > 60: at least that many), the copies planted away from the centre"""
    while True:
        h = twin_free(rng, n)
        for _ in range(200):
            if twin_entries(h) >= want:
                break
            a, b = int(rng.integers(0, n // 2 - 10)), int(rng.integers(n // 2 + 10, n - K))
            h[b:b + K] = h[a:a + K]
        if twin_entries(h) == want or (want > 60 and twin_entries(h) > 60):
            return bytes(h)


def other(b, step=1):
    return ACGT[(list(ACGT).index(b) + step) % 4]


def matches_at(read, hap, d, delta):
    """read k-mers (rows) that equal the haplotype's `delta` diagonals off the diagonal d"""
    return [r for r in range(len(read) - K + 1) if 0 <= r + d + delta <= len(hap) - K and read[r:r + K] == hap[r + d + delta:r + d + delta + K]]


def pieces_of(read, hap, d):
    """runs of >= 6 matching bases on diagonal d as (first base, last base)"""
    eq = [0 <= r + d < len(hap) and read[r] == hap[r + d] for r in range(len(read))] + [False]
    out, start = [], None
    for r, e in enumerate(eq):
        if e and start is None:
            start = r
        if not e and start is not None:
            if r - start >= K:
                out.append((start, r - 1))
            start = None
    return out


def snv(h):
    c = len(h) // 2
    return h[:c] + bytes([ACGT[(list(ACGT).index(h[c]) + 1) % 4]]) + h[c + 1:]


def mutate(rng, s, rows):
    s = bytearray(s)
    for r in rows:
        s[r] = ACGT[(list(ACGT).index(s[r]) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(s)


def rand(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def build(four_words):
    """(batch, case name per locus)"""
    rng = np.random.default_rng(1919 + int(four_words))
    n = 251 if four_words else 201                    # haplotype bases
    m = 230 if four_words else 150                    # the usual read
    haps, reads, names = [], [], []
    cell = [0]

    def rd(seq):
        cell[0] += 1
        return (cell[0] % NB, cell[0], seq)

    def locus(name, ref, alt, seqs):
        assert len(seqs) <= 64 and len(ref) <= 255 and len(alt) <= 255
        haps.append((ref, alt)); reads.append([rd(s) for s in seqs]); names.append(name)

    # ---- twins
    for want in (0, 2, 12, 14, 44, 62):
        ref = hap_with_twins(rng, n, want)
        seqs = []
        for off in range(0, n - m + 1, max(1, (n - m) // 10)):
            s = ref[off:off + m]
            seqs += [mutate(rng, s, [int(rng.integers(10, m - 10))]), mutate(rng, snv(ref)[off:off + m], [int(rng.integers(10, m - 10)), int(rng.integers(10, m - 10))])]
        for sl in (70, 100):                         # short reads far into the window: the twins of the first half lie below row 0
            seqs.append(mutate(rng, ref[n - sl:], [sl // 2]))
        locus("twins %d" % want, ref, snv(ref), seqs[:64])
    # ---- overhang
    for ln in ((70, 130, 150, 200, 256) if four_words else (70, 130, 150)):
        ref = hap_with_twins(rng, n, 4)
        seqs = []
        for over in (1, 5, 6, 7, 20, 49, ln // 2):
            body = ln - over
            if body < 30 or body > n:
                continue
            seqs += [rand(rng, over) + ref[:body], ref[n - body:] + rand(rng, over), rand(rng, over) + mutate(rng, snv(ref)[:body], [body // 2]),
                     mutate(rng, ref[n - body:], [body // 3]) + rand(rng, over)]
        locus("overhang %d" % ln, ref, snv(ref), seqs)
    # ---- append / retry: 64 reads (one or two whole wavefronts of tasks) whose overhang is a copy of haplotype sequence
    ref = hap_with_twins(rng, n, 0)
    seqs = []
    for i in range(64):
        over = 48 + (i % 3)
        seqs.append(ref[n - (m - over):] + ref[10 + i % 7:10 + i % 7 + over])
    locus("append", ref, snv(ref), seqs)
    # ---- stub: an ALT of three bases
    ref = hap_with_twins(rng, n, 2)
    locus("stub", ref, b"ACG", [mutate(rng, ref[o:o + m], [40 + o]) for o in range(0, min(n - m, 40), 3)] + [ref[:m]])
    # ---- far matches at chosen distances, either side: exactly E read k-mers match the haplotype D diagonals off the main one, on the
    #      named side and on no other (counted below, and again by test_batches_are_what_they_claim).  A run of E consecutive rows at the
    #      read's end (its start) whose bases recur D further on (before), beyond the read: a stretch of period D; E = D + 1 — one more
    #      than a stretch beyond the read can hold without matching from the other side as well — takes one more 6-mer elsewhere, whose
    #      mirror image a substitution in the read removes
    lims = {4: 2, 6: 6, 8: 8, 12: 12, 16: 16, 24: 24, 32: 32}      # bound(lower edge of D's bin)
    mf = 200 if four_words else 150                                # (n - mf = 51 bases of window beside the read: room for D = 40)
    for D in (3, 4, 5, 6, 7, 8, 11, 12, 15, 16, 23, 24, 31, 32, 39, 40):
        lim = lims[max([e for e in lims if e <= D], default=4)]
        for side in (+1, -1):
            for E in ([1] if D == 3 else [lim - 1, lim, lim + 1]):
                run = min(E, D)                                    # matches of the stretch; E - run (0 or 1) elsewhere
                ln = K - 1 + run
                for attempt in range(50):
                    h = twin_free(rng, n)
                    cuts = [mf // 2]
                    if side > 0:
                        off = n - mf - D
                        y0 = off + mf - ln
                        for i in range(ln):
                            h[y0 + D + i] = h[y0 + i]
                        h[y0 - 1] = other(h[y0 - 1 + D])           # the stretch does not go on to the left
                        if E > run:
                            r1 = 20
                            h[off + r1 + D:off + r1 + D + K] = h[off + r1:off + r1 + K]
                            cuts.append(r1 + D + 2)
                    else:
                        off = y0 = 45
                        for i in reversed(range(ln)):
                            h[y0 - D + i] = h[y0 + i]
                        h[y0 + ln] = other(h[y0 - D + ln])         # ... nor to the right
                        if E > run:
                            r1 = mf - 60
                            h[off + r1 - D:off + r1 - D + K] = h[off + r1:off + r1 + K]
                            cuts.append(r1 - D + 2)
                    ref = bytes(h)
                    read = mutate(rng, ref[off:off + mf], cuts)
                    if len(matches_at(read, ref, off, side * D)) == E and not matches_at(read, ref, off, -side * D) and \
                            all(not matches_at(read, ref, off, x) for x in range(-D + 1, D) if x != 0):
                        break
                else:
                    raise AssertionError("no far case for D %d side %d E %d" % (D, side, E))
                locus("far D %d side %+d E %d" % (D, side, E), ref, snv(ref), [read])
    # ---- pieces: one to four main pieces (a substitution ends a piece, the next starts behind it) and an off-diagonal match (sx, sy) at
    #      the equalities of harmless_item4's two conditions: a = min(sx, sy - d) at pu + K + e, the other coordinate 31 .. 40 above it;
    #      b = max(sx, sy - d) at pv - 5 - K + e, the other coordinate as far below.  The READ's own k-mer is written into the
    #      haplotype (and into the read's rows on the main diagonal there, which so stays whole).
    for r in (1, 2, 3, 4):
        cuts = [30 + 28 * i for i in range(r - 1)]
        for e in (-1, 0, 1):
            for which in range(r):
                pu = 0 if which == 0 else cuts[which - 1] + 1
                pv = (cuts[which] - 1) if which < r - 1 else m - 1
                for cond, sx in (("a", pu + K + e), ("b", pv - 5 - K + e)):
                    for gap in (35, 33, 37, 31, 39, 40):
                        t = sx + gap if cond == "a" else sx - gap     # sy - d
                        if sx >= 0 and sx + K <= m and t >= 0 and t + K <= m and not any(t - 1 <= c <= t + K for c in cuts):
                            break
                    else:
                        continue
                    off = 10
                    h = twin_free(rng, n)
                    read = bytearray(mutate(rng, bytes(h[off:off + m]), cuts))
                    read[t:t + K] = read[sx:sx + K]
                    h[off + t:off + t + K] = read[sx:sx + K]
                    ref = bytes(h)
                    locus("pieces %d e %+d %s pu %d pv %d sx %d sy %d" % (r, e, cond, pu, pv, sx, off + t), ref, snv(ref), [bytes(read)])
    # ---- short: the last locus leaves the last wavefront with fewer than 64 tasks
    ref = hap_with_twins(rng, n, 6)
    locus("short", ref, snv(ref), [mutate(rng, ref[3:3 + m], [77])] * 1)
    batch = manual_batch(haps, reads, NB)
    if (2 * batch.n_records) % 64 == 0:
        raise AssertionError("the batch must end in a short wavefront")
    return batch, names


_cache = {}


def case(four_words, tmp_dir):
    """(batch, names, locus of every task, device scores per task, device stage bytes, oracle scores per task, the mirror's arrays)"""
    if four_words not in _cache:
        from oracle import oracle
        from vartrix_amd import lib
        from vartrix_amd.abi import default_config
        batch, names = build(four_words)
        cfg = default_config(aligner="banded", scoring_mode="coverage", n_barcodes=NB)
        with lib.Context(cfg) as ctx:
            ctx.set_stage_trace(True)
            ctx.submit(batch)
            ctx.run()
            ref, alt = ctx.fetch_scores()
            stage = np.asarray(ctx.fetch_stage()).copy()
        oref, oalt = oracle.batch_scores(batch, cfg, threads=8)

        def tasks(a, b):
            t = np.empty(2 * len(a), np.int64)
            t[0::2], t[1::2] = a, b
            return t
        mir = RU.mirror(RU.load_mirror(tmp_dir), batch)
        loc = np.repeat(np.repeat(np.arange(batch.n_loci), batch.loci["rec_count"]), 2)
        _cache[four_words] = (batch, names, loc, tasks(ref, alt), stage, tasks(oref, oalt), mir)
    return _cache[four_words]


@pytest.fixture(scope="module")
def tmp_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("diag19")


@pytest.mark.parametrize("four_words", [False, True], ids=["three-words", "four-words"])
def test_batches_are_what_they_claim(four_words, tmp_dir):
    batch, names, loc, _, _, _, (rc, score, why, route, _) = case(four_words, tmp_dir)
    rl = batch.records["read_len"]
    assert rc == 0 and (192 < int(rl.max()) <= 256 if four_words else int(rl.max()) <= 192)
    assert int(batch.loci["rec_count"].max()) <= 64 and max(int(batch.loci["ref_len"].max()), int(batch.loci["alt_len"].max())) <= 255
    decided = (route & RU.DECIDED) != 0
    by = {}
    for l, nm in enumerate(names):
        key = nm.split(" ")[0]
        sel = loc == l
        d = by.setdefault(key, [0, 0, set()])
        d[0] += int(decided[sel].sum()); d[1] += int((~decided[sel]).sum()); d[2] |= set(why[sel].tolist())
    print({k: (v[0], v[1], sorted(v[2])) for k, v in by.items()})
    ref_of = lambda l: bytes(batch.hap_arena[int(batch.loci["ref_off"][l]):int(batch.loci["ref_off"][l]) + int(batch.loci["ref_len"][l])])
    alt_of = lambda l: bytes(batch.hap_arena[int(batch.loci["alt_off"][l]):int(batch.loci["alt_off"][l]) + int(batch.loci["alt_len"][l])])

    def reads_of(l):
        out = []
        for r in range(int(batch.loci["rec_begin"][l]), int(batch.loci["rec_begin"][l]) + int(batch.loci["rec_count"][l])):
            o, n_ = int(batch.records["read_off"][r]), int(batch.records["read_len"][r])
            out.append(bytes(batch.read_arena[o:o + n_]))
        return out
    # far: counted here from the batch's own bytes — exactly E read k-mers D diagonals off the main one on the named side, none on the
    # other side, none nearer; every distance and side with the E below, at and above the bound of D's bin
    seen = set()
    mf = 200 if four_words else 150
    nh = 251 if four_words else 201
    for l, nm in enumerate(names):
        if not nm.startswith("far "):
            continue
        _, _, D, _, side, _, E = nm.split(" ")
        D, side, E = int(D), int(side), int(E)
        d = (nh - mf - D) if side > 0 else 45
        (read,), ref = reads_of(l), ref_of(l)
        assert pieces_of(read, ref, d), nm
        assert len(matches_at(read, ref, d, side * D)) == E, (nm, matches_at(read, ref, d, side * D))
        assert not matches_at(read, ref, d, -side * D) and all(not matches_at(read, ref, d, x) for x in range(-D + 1, D) if x != 0), nm
        seen.add((D, side, E))
    lims = {3: None, 4: 2, 5: 2, 6: 6, 7: 6, 8: 8, 11: 8, 12: 12, 15: 12, 16: 16, 23: 16, 24: 24, 31: 24, 32: 32, 39: 32, 40: 32}
    for D, lim in lims.items():
        for side in (1, -1):
            for E in ([1] if lim is None else [lim - 1, lim, lim + 1]):
                assert (D, side, E) in seen, (D, side, E)
    # pieces: the planted match exists and sits at the stated equality of the stated piece
    conds = set()
    for l, nm in enumerate(names):
        if not nm.startswith("pieces "):
            continue
        f = nm.split(" ")
        r, e, cond, pu, pv, sx, sy = int(f[1]), int(f[3]), f[4], int(f[6]), int(f[8]), int(f[10]), int(f[12])
        (read,), ref, d = reads_of(l), ref_of(l), 10
        assert read[sx:sx + K] == ref[sy:sy + K] and sy - sx != d, nm
        ps = pieces_of(read, ref, d)
        assert len(ps) == r and (pu, pv) in ps, (nm, ps)
        a, b = min(sx, sy - d), max(sx, sy - d)
        assert (a == pu + K + e and sx == a) if cond == "a" else (b == pv - 5 - K + e and sx == b), nm
        conds.add((r, e, cond))
    assert conds == {(r, e, c) for r in (1, 2, 3, 4) for e in (-1, 0, 1) for c in "ab"}
    # append: the rows of the overhangs that are k-mers of BOTH haplotypes, counted here.  A pair's rows are probed in blocks of three;
    # one trip of pass 1 takes 6 x 64 blocks, each hit row two walk entries: the wavefront's first trip passes the list's 224 entries
    # when the pairs hold more than 112 such rows between them.  (That one LANE gets six blocks of three such rows — all 36 append bits —
    # follows from nearly every block being one, and is not observed: the kernel has no counter for it.)
    l = names.index("append")
    ref, alt = ref_of(l), alt_of(l)
    both = []
    for read in reads_of(l):
        body_d = [x for x in range(-len(read), len(ref)) if len(pieces_of(read, ref, x)) and max(b_ - a_ for a_, b_ in pieces_of(read, ref, x)) > 60]
        assert len(body_d) == 1
        rows = [r_ for r_ in range(len(read) - K + 1) if read[r_:r_ + K] != ref[r_ + body_d[0]:r_ + body_d[0] + K]]
        both.append(sum(1 for r_ in rows if read[r_:r_ + K] in ref and read[r_:r_ + K] in alt))
    print("append: rows per read that hit in both haplotypes: min %d, any 32 reads in a row at least %d" % (min(both), min(sum(both[i:i + 32]) for i in range(33))))
    assert min(both) >= 36 and min(sum(both[i:i + 16]) for i in range(49)) > 224
    for key in ("twins", "overhang", "pieces", "far"):
        assert by[key][0] > 0, key                       # the first stage decides tasks of every family
    assert by["append"][1] > 0 and by["stub"][0] > 0


@pytest.mark.parametrize("four_words", [False, True], ids=["three-words", "four-words"])
def test_scores_are_the_oracles(four_words, tmp_dir):
    _, names, loc, got, _, want, _ = case(four_words, tmp_dir)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%d scores differ from the oracle; first: task %d of locus '%s': %d, oracle %d" % (
        len(bad), bad[0], names[loc[bad[0]]], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("four_words", [False, True], ids=["three-words", "four-words"])
def test_first_stage_decides_what_the_mirror_decides(four_words, tmp_dir):
    """Verdict, score, stage byte and list: a task the mirror decides carries the diag certificate's stage and the mirror's score, one it
    hands to the corridor bound the corridor's stage and score, one that keeps only its one-diagonal band the band's DP stage; every
    other task is decided by none of the three."""
    _, names, loc, got, stage, _, (rc, score, why, route, _) = case(four_words, tmp_dir)
    decided, corridor, band = (route & RU.DECIDED) != 0, (route & RU.CORRIDOR) != 0, (route & RU.BAND) != 0
    want = np.where(decided, STAGE_DIAG_CERT, np.where(corridor, STAGE_CORRIDOR_CERT, np.where(band, STAGE_DIAG_DP, 0)))
    known = want != 0
    bad = np.nonzero(known & (stage != want))[0]
    assert len(bad) == 0, "%d tasks decided elsewhere than the mirror says; first: task %d of '%s': stage %d, mirror %d (why %d)" % (
        len(bad), bad[0], names[loc[bad[0]]], stage[bad[0]], want[bad[0]], why[bad[0]])
    left = ~known & (why != 1)                                     # (W_SHAPE: a haplotype below six bases, scored without a table)
    assert not np.isin(stage[left], (STAGE_DIAG_CERT, STAGE_CORRIDOR_CERT, STAGE_DIAG_DP)).any(), "the device decided a task the mirror leaves"
    fin = decided | corridor
    assert np.array_equal(got[fin], score[fin].astype(np.int64))
