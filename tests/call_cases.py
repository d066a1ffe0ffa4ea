"""Authored batches that reach every class of the call stage (tests/call_model.py names the classes): REF / ALT / UNKNOWN / None at
every threshold boundary, every UMI-family composition up to 8 reads, every cell composition, repeated cell and UMI ids across
group boundaries, groups longer than a 256-thread block and group heads on block edges.  Built from READS, not from injected
scores, so that the production path (aligner, call, collapse, emit) runs end to end.

How a read reaches a score class.  ONE SNV haplotype pair, PAD bases on each side of the site.  Reads are exact substrings, so with
match = 1, mismatch = -5, gap open = -5 a score is a length:
  avoid(L)        a read of L bases next to the site: L on both haplotypes        (a tie: UNKNOWN when L >= m, None when L < m)
  cover(REF, L)   L bases of REF over the site, >= 7 bases on each side: L on REF, L - 6 on ALT  (the mismatch costs 1 + 5)
  cover(ALT, L)   the mirror image
  the one-base read "T": the flanks are drawn from A, C, G and the REF allele is T, so T occurs once in REF and never in ALT: 1 / 0
  the read "NNNNNNNN" shares no base with either haplotype: 0 / 0; the empty read: 0 / 0
Every read carries the scores its construction promises; tests/test_call_model.py asserts them against the oracle's aligner, which
is what makes the ledger mean something.  The reads and haplotypes are the same in every run; only cfg.min_score, cfg.use_umi,
cfg.scoring_mode and the entry path change.
"""
import itertools

import numpy as np

from vartrix_amd.abi import LOCUS_DTYPE, RAW_RECORD_DTYPE, RECORD_DTYPE, PackedBatch, RawBatch

PAD = 100
N_BARCODES = 400
MIN_SCORES = (0, 1, 25, 26, 151)
UMI_MAX = 2 ** 31 - 1
BLOCK = 256


def _haplotypes():
    rng = np.random.default_rng(20261017)
    flank = bytes(rng.choice(list(b"ACG"), 2 * PAD).tolist())
    return flank[:PAD] + b"T" + flank[PAD:], flank[:PAD] + b"A" + flank[PAD:]


REF_HAP, ALT_HAP = _haplotypes()


# ---- reads: (bases, (promised REF score, promised ALT score)) ----
def cover(alt, L, i=0):
    assert 15 <= L <= 150
    lo, hi = max(7, L - 1 - PAD), min(PAD, L - 8)      # bases in front of the site; the rest, L - 1 - left >= 7, behind it
    left = lo + i % (hi - lo + 1)
    hap = ALT_HAP if alt else REF_HAP
    return hap[PAD - left:PAD - left + L], ((L - 6, L) if alt else (L, L - 6))


def avoid(L, i=0):
    assert 0 <= L <= PAD
    start = i % (PAD - L + 1) + (PAD + 1 if i & 1 else 0)
    return REF_HAP[start:start + L], (L, L)


def R(i=0):
    return cover(False, 40, i)


def A(i=0):
    return cover(True, 40, i)


def U(i=0):
    return avoid(40, i)


def NONE(i=0):
    """None at every threshold from 11 up (i odd; UNKNOWN below) or from 1 up (i even: the empty read)."""
    return avoid(10, i) if i & 1 else avoid(0)


T_READ = (b"T", (1, 0))
N_READ = (b"N" * 8, (0, 0))


class Case:
    """One batch: loci = [(row, [(cell, umi, (bases, promise))])], records in the order given (sorted by (cell, umi) unless `unsorted`)."""

    def __init__(self, name, loci, umi_modes=(0, 1), unsorted=False):
        self.name, self.umi_modes, self.n_barcodes = name, umi_modes, N_BARCODES
        lo, rec, arena, promise = [], [], bytearray(), []
        hap = REF_HAP + ALT_HAP
        for row, reads in loci:
            if not unsorted:
                assert reads == sorted(reads, key=lambda t: (t[0], t[1])), (name, row)
            lo.append((row, len(rec), len(reads), 0, len(REF_HAP), len(REF_HAP), len(ALT_HAP), 0))
            for cell, umi, (seq, p) in reads:
                assert 0 <= cell < N_BARCODES and 0 <= umi <= UMI_MAX and len(seq) <= 150
                rec.append((len(arena), len(seq), cell, umi))
                arena += seq
                promise.append(p)
        self.batch = PackedBatch(np.array(lo, LOCUS_DTYPE).reshape(-1), np.array(rec, RECORD_DTYPE).reshape(-1),
                                 np.frombuffer(hap, np.uint8), np.frombuffer(bytes(arena) + b"A", np.uint8))
        self.promise = np.array(promise, np.int32).reshape(-1, 2)
        self._scores = {}

    @property
    def n(self):
        return self.batch.n_records

    def model_loci(self, batch=None):
        b = self.batch if batch is None else batch
        return [(int(r), int(s), int(c)) for r, s, c in zip(b.loci["row"], b.loci["rec_begin"], b.loci["rec_count"])]

    @staticmethod
    def model_records(batch):
        return list(zip(batch.records["cell_index"].tolist(), batch.records["umi_id"].tolist()))

    def oracle_scores(self, aligner):
        """(ref, alt) of the oracle's aligner for the id form, once per aligner."""
        if aligner not in self._scores:
            from oracle import oracle
            from vartrix_amd.abi import default_config
            self._scores[aligner] = oracle.batch_scores(self.batch, default_config(aligner=aligner, n_barcodes=N_BARCODES), threads=8)
        return self._scores[aligner]

    def scores_of(self, records, aligner):
        """The oracle's scores for records that name this case's reads in another order (the raw path's prepared records)."""
        r, a = self.oracle_scores(aligner)
        table = {}
        for k, (off, ln) in enumerate(zip(self.batch.records["read_off"].tolist(), self.batch.records["read_len"].tolist())):
            assert table.setdefault((off, ln), (r[k], a[k])) == (r[k], a[k])      # (empty reads share an offset: the same 0 / 0)
            table[(off, ln)] = (r[k], a[k])
        got = [table[(o, l)] for o, l in zip(records["read_off"].tolist(), records["read_len"].tolist())]
        out = np.array(got, np.int32).reshape(-1, 2)
        return out[:, 0].copy(), out[:, 1].copy()


# ---- the raw form: barcode and UB bytes instead of ids ----
BARCODES = [b"%s-1" % "".join("ACGT"[(j >> (2 * d)) & 3] for d in range(16)).encode() for j in range(N_BARCODES)]
# UMI ids whose bytes are special (the raw-only locus of main_case uses them); every other id is 16 bases spelling the id
UB_EMPTY, UB_SHORT, UB_LONG, UB_LAST = 1000, 1001, 1002, 1003
UB_SPECIAL = {UB_EMPTY: b"", UB_SHORT: b"ACGTACGT", UB_LONG: b"ACGTACGTAC", UB_LAST: b"ACGTACGTAA"}


def ub_bytes(umi):
    if umi in UB_SPECIAL:
        return UB_SPECIAL[umi]
    return "".join("ACGT"[(umi >> (2 * d)) & 3] for d in range(16)).encode()


def raw_form(case, seed=5):
    """vtx_submit_raw's view of `case`: the same reads, shuffled inside their locus, cell and UMI as tag bytes.  UB bytes are a
    function of the UMI id alone, so the same bytes recur wherever the id form repeats an id: in other cells, in other loci."""
    rng = np.random.default_rng(seed)
    b = case.batch
    raw = np.zeros(b.n_records, RAW_RECORD_DTYPE)
    tags = bytearray()
    order = np.concatenate([s + rng.permutation(c) for s, c in zip(b.loci["rec_begin"].astype(np.int64), b.loci["rec_count"])] +
                           [np.zeros(0, np.int64)]).astype(np.int64)
    for j, i in enumerate(order):
        r = b.records[i]
        bc, ub = BARCODES[int(r["cell_index"])], ub_bytes(int(r["umi_id"]))
        raw[j] = (r["read_off"], r["read_len"], len(tags), len(tags) + len(bc), len(bc), len(ub))
        tags += bc + ub
    return RawBatch(b.loci.copy(), raw, b.hap_arena, b.read_arena, np.frombuffer(bytes(tags) + b"A", np.uint8))


def raw_ledger(raw):
    """The classes only the raw path has, read off the tag bytes."""
    out = set()
    t = raw.tag_arena.tobytes()
    where = {}                                 # UB bytes -> {(locus, barcode bytes)}
    for li in range(raw.n_loci):
        s, c = int(raw.loci["rec_begin"][li]), int(raw.loci["rec_count"][li])
        by_cell = {}
        for r in raw.records[s:s + c]:
            bc = t[int(r["bc_off"]):int(r["bc_off"]) + int(r["bc_len"])]
            ub = t[int(r["umi_off"]):int(r["umi_off"]) + int(r["umi_len"])]
            by_cell.setdefault(bc, set()).add(ub)
            where.setdefault(ub, set()).add((li, bc))
        for ubs in by_cell.values():
            if b"" in ubs:
                out.add("raw:zero-length-ub")
            for x, y in itertools.permutations(ubs, 2):
                if x and len(x) < len(y) and y.startswith(x):
                    out.add("raw:ub-prefix-of-another-in-one-cell")
                if x and len(x) == len(y) and x[:-1] == y[:-1] and x[-1] != y[-1]:
                    out.add("raw:ubs-differ-in-the-last-byte-in-one-cell")
    for places in where.values():
        if len({bc for _, bc in places}) > 1:
            out.add("raw:same-ub-in-different-cells")
        if len({li for li, _ in places}) > 1:
            out.add("raw:same-ub-in-different-loci")
    return out


# ---- the batches ----
FAMILIES = [(r, a, t - r - a) for t in range(1, 9) for r in range(t + 1) for a in range(t + 1 - r)]
assert len(FAMILIES) == 164
CELLS = list(itertools.product(range(3), repeat=3))


def family_reads(r, a, k, i):
    """r REF, a ALT, k UNKNOWN reads, interleaved (the order inside a family is free)."""
    reads = [R(i + j) for j in range(r)] + [A(i + j) for j in range(a)] + [U(i + j) for j in range(k)]
    return reads[i % len(reads):] + reads[:i % len(reads)]


class _Filler:
    """Ordinary records — a few cells per locus, families of 1 .. 4 reads, every kind of read — to put what follows at a chosen
    record index."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.umi = 5000

    def reads(self, n):
        kinds = (R, A, U, NONE, lambda i: cover(False, 25, i), lambda i: cover(True, 26, i), lambda i: avoid(25, i), lambda i: avoid(24, i))
        out, cell = [], int(self.rng.integers(0, 20))
        while len(out) < n:
            cell += int(self.rng.integers(1, 4))
            for _ in range(int(self.rng.integers(1, 4))):
                self.umi += 1
                for _ in range(int(self.rng.integers(1, 5))):
                    if len(out) < n:
                        out.append((cell % N_BARCODES, self.umi, kinds[int(self.rng.integers(0, len(kinds)))](int(self.rng.integers(0, 90)))))
        return sorted(out, key=lambda t: (t[0], t[1]))

    def loci(self, n, per_locus=48):
        out = []
        while n > 0:
            out.append(self.reads(min(n, per_locus)))
            n -= len(out[-1])
        return out


def main_case():
    """Every class but the ones that need a batch of their own (see LEDGER)."""
    loci = []                                  # lists of reads; rows are given at the end
    count = lambda: sum(len(l) for l in loci)
    fill = _Filler(1)

    def pad_to(residue):
        loci.extend(fill.loci((residue - count()) % BLOCK))

    # -- call boundaries: every read in a cell of its own, so each call shows in the entries by itself
    lengths = (15, 18, 19, 20, 24, 25, 26, 30, 31, 32, 33, 40, 144, 145, 150)
    solo = [avoid(L, L) for L in (0, 1, 2, 10, 18, 19, 24, 25, 26, 27, 31, 32, 40, PAD)] + [T_READ, N_READ]
    solo += [cover(alt, L, L) for L in lengths for alt in (False, True)]
    loci.append([(c, 100 + c, rd) for c, rd in enumerate(solo)])
    # -- UMI families: one composition each, one family per cell (the collapse shows in the entry by itself) ...
    loci.append([(c, 7, rd) for c, (r, a, k) in enumerate(FAMILIES) for rd in family_reads(r, a, k, c)])
    # ... every second one again with None reads mixed in (they must not count toward t), and families of None reads only
    mixed = []
    for c, (r, a, k) in enumerate(FAMILIES[::2]):
        reads = family_reads(r, a, k, c + 1)
        for j in range(1 + c % 3):
            reads.insert((c + 2 * j) % (len(reads) + 1), NONE(c + j))
        mixed += [(c, 300 + c, rd) for rd in reads]
    mixed += [(200, 1, NONE(0)), (200, 1, NONE(2)), (201, 1, NONE(0)), (201, 2, R(3)), (202, 5, A(1)), (202, 6, NONE(4)), (202, 6, NONE(6))]
    loci.append(mixed)
    # -- cells after collapse: every (R, A, K) in {0, 1, 2}^3, every read a UMI of its own (the same cell with and without UMIs)
    cells = []
    for c, (r, a, k) in enumerate(CELLS):
        reads = family_reads(r, a, k, c) if r + a + k else [NONE(0)]
        cells += [(2 * c, 10 * c + j, rd) for j, rd in enumerate(reads)]
        if c % 2:                              # the same again with a None read in it
            cells += [(2 * c + 1, 10 * c + j, rd) for j, rd in enumerate(reads + [NONE(2 * c)])]
    loci.append(cells)
    # -- identity edges
    last = N_BARCODES - 1
    loci.append([(0, 0, R(1)), (0, 0, R(2)), (0, UMI_MAX, A(3)), (5, 7, R(4))])                 # cell 0; UMI 0 and 2^31 - 1; ends in (5, 7)
    loci.append([(5, 7, A(5)), (5, 7, A(6)), (5, 7, A(7)), (9, 3, R(8))])                       # begins with the same cell and UMI; ends in (9, 3)
    loci.append([(9, 4, A(9)), (10, 42, R(1)), (10, 42, R(2)), (11, 42, A(3)), (12, 42, U(4)), (last, 42, R(5))])   # same cell, other UMI; UMI 42 in adjacent cells
    loci.append([])                                                                               # a locus without records between two with
    loci.append([(last, 42, A(6)), (last, 43, A(7))])
    # -- raw path only: UB bytes that are empty, a prefix of another, equal up to the last byte (UB_SPECIAL); one family each, and
    #    every family with another call, so that two of them taken for one changes the cell's counts
    loci.append([(20, UB_EMPTY, R(1)), (20, UB_EMPTY, R(2)), (20, UB_SHORT, A(1)), (20, UB_SHORT, A(2)), (20, UB_LONG, U(1)),
                 (20, UB_LAST, R(3)), (20, UB_LAST, R(4)), (21, UB_LONG, A(5)), (21, UB_LAST, U(6))])
    # -- longer than a block: one cell group of 600 records; in it one UMI family of 300 that is ALT by exactly 0.75 (225 : 75)
    big = [(30, 1, A(j) if j % 4 else R(j)) for j in range(300)]
    big += [(30, 2 + j // 3, (R, R, A)[j % 3](j)) for j in range(150)]                          # 50 families, 2 : 1 -> UNKNOWN
    big += [(30, 100 + j // 4, (A, A, A, U)[j % 4](j)) for j in range(150)]                     # 3 : 1 -> ALT (the last one 2 : 0)
    loci.append([(29, 1, R(0))] + big + [(31, 1, R(1))])
    # -- block edges: a cell-group head (not its locus's first record) on record index 255, 256 and 257 modulo 256 ...
    pad_to(BLOCK - 3)
    loci.append([(40, 1, R(1)), (40, 2, A(1)), (41, 2, A(2)), (42, 2, R(2)), (43, 2, U(1)), (43, 3, A(3))])
    # ... a UMI-family head inside a cell group on each of them ...
    pad_to(BLOCK - 3)
    loci.append([(50, 1, R(1)), (50, 1, R(2)), (50, 2, A(1)), (50, 3, U(1)), (50, 4, A(2)), (50, 4, A(3)), (50, 5, R(3))])
    # ... a locus boundary on each of them, between loci that end and begin with the same cell and UMI
    pad_to(BLOCK - 2)
    loci += [[(60, 9, R(1))], [(60, 9, A(1))], [(60, 9, U(1))], [(60, 9, A(2)), (61, 9, R(2))]]
    # -- and the last record of the batch on index 257 (call_256 / call_257 have theirs on 255 and 256)
    pad_to(2)
    assert count() % BLOCK == 2
    return Case("main", [(3 * i + 2, reads) for i, reads in enumerate(loci)])                   # rows with gaps: never the locus index


def sized_case(n):
    """Exactly n records of ordinary material."""
    f = _Filler(n)
    c = Case("n%d" % n, list(enumerate(f.loci(n, per_locus=60))))
    assert c.n == n
    return c


def unsorted_case():
    """use_umi = 0 only: arbitrary, unsorted umi_id inside a cell (include/vtx.h: "any value when !use_umi")."""
    reads = [(3, 5, R(1)), (3, 2, A(1)), (3, 9, R(2)), (3, 2, U(1)), (3, 0, NONE(1)), (3, UMI_MAX, R(3)), (3, 0, A(2)),
             (4, 7, A(3)), (4, 1, A(4)), (4, 7, R(4)), (6, 2, U(2))]
    return Case("unsorted-umi", [(0, reads), (1, [(6, 1, R(5)), (6, 0, A(5))])], umi_modes=(0,), unsorted=True)


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = [main_case(), sized_case(256), sized_case(257), unsorted_case()]
    return _cases


def cases_for(use_umi):
    return [c for c in cases() if use_umi in c.umi_modes]


# ---- the ledger: every class, and in which configurations it has to be reached ----
# Scores are never negative, so at min_score 0 no read is None and no side of a call is under the threshold; no read is longer than
# 150 bases, so at min_score 151 every read is None, every family is made of None reads only and every cell is (0, 0, 0).  The
# one-base read "T" (1 / 0) and the empty read are what reach "one side under" and None at min_score 1.  Everything else is reached at
# every threshold up to 26: the reads of the families and cells are 40 bases long (40 / 34, 34 / 40, 40 / 40).
def _calls(m):
    return m <= 26


LEDGER = [
    # the five call outcomes
    ("call:none", lambda m, umi: m >= 1),
    ("call:ref", lambda m, umi: _calls(m)),
    ("call:alt", lambda m, umi: _calls(m)),
    ("call:unknown", lambda m, umi: _calls(m)),
    ("call:one-side-under", lambda m, umi: 1 <= m <= 26),
    # UMI families
    *[("family:%d,%d,%d" % f, lambda m, umi: umi and _calls(m)) for f in FAMILIES],
    ("family:none-only", lambda m, umi: umi and m >= 1),
    ("family:with-none-reads", lambda m, umi: umi and 1 <= m <= 26),
    # cells after collapse, per UMI mode (the test runs both)
    *[("cell:%d,%d,%d" % c, (lambda m, umi: m >= 1) if c == (0, 0, 0) else (lambda m, umi: _calls(m))) for c in CELLS],
    # identity edges
    ("edge:cell-across-loci:same-umi", lambda m, umi: True),
    ("edge:cell-across-loci:other-umi", lambda m, umi: True),
    ("edge:umi-in-adjacent-cells", lambda m, umi: True),
    ("edge:umi-0", lambda m, umi: True),
    ("edge:umi-2^31-1", lambda m, umi: True),
    ("edge:unsorted-umi-without-umis", lambda m, umi: not umi),
    ("edge:empty-locus-between", lambda m, umi: True),
    ("edge:row-is-not-the-index", lambda m, umi: True),
    ("edge:cell-0", lambda m, umi: True),
    ("edge:cell-last", lambda m, umi: True),
    # block edges
    ("block:cell-group-over-two-blocks", lambda m, umi: True),
    ("block:family-over-one-block", lambda m, umi: bool(umi)),
    *[("block:%s@%s" % (what, at), lambda m, umi: True) for what in ("cell-head", "umi-head", "locus-head", "last-record")
      for at in ("255", "256", "257")],
]
RAW_LEDGER = ["raw:same-ub-in-different-cells", "raw:same-ub-in-different-loci", "raw:ub-prefix-of-another-in-one-cell",
              "raw:zero-length-ub", "raw:ubs-differ-in-the-last-byte-in-one-cell"]


def required(min_score, use_umi):
    return {name for name, when in LEDGER if when(min_score, use_umi)}
