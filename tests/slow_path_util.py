"""Case builders for the exact slow path (slow_align_kernel / run_slow: records with a read above 1 024 bases or a haplotype above
2 400).  Pure Python and numpy, fixed seeds; tests/test_slow_path_cases.py proves what the builders promise from the CPU oracle alone,
tests/test_gpu_slow_path.py runs them on the device.

Every builder returns (batch, info).  `info` holds one entry per TASK (2 * record + haplotype, the order of vtx_fetch_stage):
  slow     the record is on the slow list: read_len > FAST_READ_LEN or max(ref_len, alt_len) > FAST_HAP_LEN (both prep kernels)
  M        the number of 6-mer matches the case promises (find_kmer_matches of the oracle), -1 where the case promises none
  no_seed  the case promises that the read shares no 6-mer with the haplotype (Band::full_matrix: the whole matrix in both flavours)
and `n_barcodes`, plus per-builder keys named in the builder's docstring."""
import functools

import numpy as np

import stress_batches as SB
from oracle import oracle
from vartrix_amd.abi import PackedBatch

FAST_READ_LEN, FAST_HAP_LEN = 1024, 2400          # vtx_prep.hip: c_fast_limit
MAX_LEN = 30000                                   # vtx_api.hip: kMaxReadLen, kMaxHapLen
KMER = 6
SLAB_CAPS = (1024, 16384, 262144)                 # run_slow: the match capacity of rounds 1, 2, 3 (x 16 per round)
ACGT = b"ACGT"

# (a, b) of match_count_pair: M = (a - 5) * (b - 5)
MATCH_COUNT_AB = {1024: (37, 37), 1025: (30, 46), 16384: (133, 133), 16385: (150, 118), 262144: (517, 517), 262145: (550, 486)}


def rung(M):
    """The round of run_slow (0-based) in which a banded task with M matches fits its slab."""
    return int(sum(M > c for c in SLAB_CAPS))


def _rand(rng, n, alphabet=ACGT):
    return bytes(rng.choice(list(alphabet), n).tolist()) if n else b""


def _other(base, step=1):
    return bytes([ACGT[(ACGT.index(base) + step) % 4]])


def _mutate(rng, seq, rate):
    b = bytearray(seq)
    for e in np.nonzero(rng.random(len(b)) < rate)[0]:
        b[e] = ACGT[int(rng.integers(0, 4))]
    return bytes(b)


class _Cases:
    """Loci and reads with what each read promises; build() lays them out as stress_batches.manual_batch does (reads sorted by
    (cell, umi) inside a locus, a stable sort) and carries the promises along."""

    def __init__(self, n_barcodes, seed):
        self.nb, self.rng, self.haps, self.reads = n_barcodes, np.random.default_rng(seed), [], []

    def locus(self, ref, alt):
        self.haps.append((ref, alt))
        self.reads.append([])
        return len(self.haps) - 1

    def read(self, locus, seq, M=(-1, -1), no_seed=False, tag=None, cell=None):
        cell = int(self.rng.integers(0, self.nb)) if cell is None else cell
        self.reads[locus].append((cell, int(self.rng.integers(0, 3)), seq, M, no_seed, tag))

    def build(self):
        batch = SB.manual_batch(self.haps, [[r[:3] for r in rl] for rl in self.reads], self.nb)
        slow, M, no_seed, tags = [], [], [], {}
        for (ref, alt), rl in zip(self.haps, self.reads):
            for r in sorted(rl, key=lambda t: (t[0], t[1])):
                rec = len(slow) // 2
                s = len(r[2]) > FAST_READ_LEN or max(len(ref), len(alt)) > FAST_HAP_LEN
                slow += [s, s]
                M += [r[3][0], r[3][1]]
                no_seed += [r[4], r[4]]
                if r[5] is not None:
                    tags.setdefault(r[5], []).append(rec)
                assert bytes(batch.read_arena[int(batch.records["read_off"][rec]):][:len(r[2])]) == r[2]
        info = dict(slow=np.array(slow, bool), M=np.array(M, np.int64), no_seed=np.array(no_seed, bool), n_barcodes=self.nb,
                    tags={k: np.array(v) for k, v in tags.items()})
        assert len(slow) == 2 * batch.n_records
        return batch, info


def task_sequences(batch, task):
    """(read, haplotype) bytes of task 2 * record + hap."""
    rec, hap = task >> 1, task & 1
    r = batch.records[rec]
    loc = batch.loci[int(np.searchsorted(batch.loci["rec_begin"].astype(np.int64) + batch.loci["rec_count"], rec, side="right"))]
    off, ln = (int(loc["alt_off"]), int(loc["alt_len"])) if hap else (int(loc["ref_off"]), int(loc["ref_len"]))
    return bytes(batch.read_arena[int(r["read_off"]):int(r["read_off"]) + int(r["read_len"])]), bytes(batch.hap_arena[off:off + ln])


def match_counts(batch):
    """M of every task, from the oracle's find_kmer_matches."""
    out = np.zeros(2 * batch.n_records, np.int64)
    for t in range(len(out)):
        x, y = task_sequences(batch, t)
        out[t] = len(oracle.kmer_matches(x, y))
    return out


def slow_rule(batch):
    """The classification rule of both prep kernels, per task."""
    rec_locus = np.repeat(np.arange(batch.n_loci), batch.loci["rec_count"])
    hmax = np.maximum(batch.loci["ref_len"], batch.loci["alt_len"])[rec_locus]
    return np.repeat((batch.records["read_len"] > FAST_READ_LEN) | (hmax > FAST_HAP_LEN), 2)


def _no_shared_kmer_read(rng, haps, n):
    """n bases over ACGT none of whose 6-mers occurs in any of `haps` (depth-first, the next base in random order)."""
    seen = set()
    for h in haps:
        seen.update(h[i:i + KMER] for i in range(len(h) - KMER + 1))
    out = bytearray(_rand(rng, KMER - 1))
    order = [list(rng.permutation(4)) for _ in range(n)]
    pos = [0] * n
    i = KMER - 1
    while i < n:
        while pos[i] < 4:
            c = ACGT[order[i][pos[i]]]
            pos[i] += 1
            if bytes(out[i - KMER + 1:i]) + bytes([c]) not in seen:
                out.append(c)
                break
        else:
            pos[i] = 0
            i -= 1
            assert i >= KMER - 1, "no read without a shared 6-mer"
            out.pop()
            continue
        i += 1
    return bytes(out)


@functools.lru_cache(maxsize=None)
def edge_batch():
    """One batch at every edge of the classification rule, with the degenerate tasks on the slow list.  info["tags"] names records:
    len1023 / len1024 / len1025 / len1026 (the 201-base locus), empty, len1, len5, len6, no_seed, n_run, lower, iupac (the
    2 401-base locus), short_ref (the locus whose REF is 3 bases)."""
    c = _Cases(12, 20241)
    rng = c.rng
    g = _rand(rng, 60000)

    def reads_around(locus, p, lens, tagged=False):
        for ln in lens:
            s = p - int(rng.integers(50, ln - 20))           # (the read covers the variant at p)
            c.read(locus, _mutate(rng, g[s:s + ln], 0.01), tag=("len%d" % ln) if tagged else None)

    # 1. a 201-base locus: reads of 1 023 .. 1 026 bases decide alone
    p = 3000
    l0 = c.locus(g[p - 100:p + 101], g[p - 100:p] + _other(g[p:p + 1]) + g[p + 1:p + 101])
    reads_around(l0, p, (1023, 1024, 1025, 1026), tagged=True)
    reads_around(l0, p, (150, 150, 150))
    # 2. haplotypes of 2 400 / 2 401 bases: both equal, and one of the two over (an insertion, a deletion)
    for k, (rlen, alen) in enumerate(((2400, 2400), (2401, 2401), (2400, 2401), (2401, 2400))):
        p = 8000 + 4000 * k
        left = g[p - 1200:p]
        if rlen == alen:
            ref = left + g[p:p + rlen - 1200]
            alt = left + _other(g[p:p + 1]) + ref[1201:]
        elif alen > rlen:                           # one-base insertion behind base p
            ref = left + g[p:p + 1200]
            alt = left + g[p:p + 1] + _other(g[p + 1:p + 2]) + g[p + 1:p + 1200]
        else:                                       # one-base deletion
            ref = left + g[p:p + 1201]
            alt = left + g[p:p + 1] + g[p + 2:p + 1201]
        assert (len(ref), len(alt)) == (rlen, alen)
        lk = c.locus(ref, alt)
        reads_around(lk, p, (150, 150, 150, 1024))
    # 3. a 2 401-base locus (every record slow) with the degenerate tasks; its haplotypes carry a run of 12 N
    p = 30000
    ref = bytearray(g[p - 1200:p + 1201])
    ref[300:312] = b"N" * 12
    ref = bytes(ref)
    alt = ref[:1200] + _other(ref[1200:1201]) + ref[1201:]
    ld = c.locus(ref, alt)
    reads_around(ld, p, (150, 150, 1024))
    c.read(ld, b"", M=(0, 0), tag="empty")
    for ln in (1, 5, 6):
        c.read(ld, ref[1198:1198 + ln], M=(0, 0) if ln < KMER else (-1, -1), tag="len%d" % ln)
    c.read(ld, _no_shared_kmer_read(rng, (ref, alt), 150), M=(0, 0), no_seed=True, tag="no_seed")
    c.read(ld, ref[230:300] + b"N" * 10 + ref[312:382], tag="n_run")
    c.read(ld, ref[1130:1280].lower(), tag="lower")
    c.read(ld, ref[1120:1200] + b"R" + ref[1201:1270], tag="iupac")
    # 4. REF below k, ALT a 2 500-base insertion
    p = 40000
    ins = _rand(rng, 2500)
    ref3 = g[p:p + 3]
    alt3 = ref3[:1] + ins + ref3[1:]
    ls = c.locus(ref3, alt3)
    for s, ln in ((0, 150), (1200, 150), (2380, 123), (700, 1024)):
        c.read(ls, _mutate(rng, alt3[s:s + ln], 0.01), tag="short_ref")
    return c.build()


def _match_count_seqs(target, rng):
    a, b = MATCH_COUNT_AB[target]
    body = bytearray(_rand(rng, 1030, b"CG"))
    body[-1] = ord("G")                              # (a C there would add the stray match CAAAAA)
    read = bytes(body) + b"A" * a
    ref = b"T" * 100 + b"T" + b"T" * 100 + b"C" + b"A" * b + b"C" + b"T" * (2401 - 203 - b)
    alt = ref[:100] + b"G" + ref[101:]
    assert len(ref) == len(alt) == 2401
    return read, ref, alt


@functools.lru_cache(maxsize=None)
def match_count_pair(target):
    """One locus, one read; both tasks have exactly `target` k-mer matches (asserted here with the oracle)."""
    read, ref, alt = _match_count_seqs(target, np.random.default_rng(target))
    for hap in (ref, alt):
        M = len(oracle.kmer_matches(read, hap))
        assert M == target, "match_count_pair(%d): the oracle counts %d" % (target, M)
    c = _Cases(4, target)
    c.read(c.locus(ref, alt), read, M=(target, target))
    return c.build()


@functools.lru_cache(maxsize=None)
def ladder_batch(top_tasks=2):
    """About 24 slow tasks on every rung of run_slow's slab ladder, the records of a locus in shuffled order (their cells are drawn
    at random), on several loci.  `top_tasks`: how many tasks need the fourth slab (M > 262 144).  info["M"] holds the oracle's
    count of every task."""
    c = _Cases(16, 777)
    rng = c.rng
    g = _rand(rng, 30000)

    def cg_read(a):
        body = bytearray(_rand(rng, 1030, b"CG"))
        body[-1] = ord("G")
        return bytes(body) + b"A" * a

    # locus 0: the poly-A haplotype of match_count_pair with a run of 517 A in REF and of 37 A in ALT (a 480-base deletion): M is
    # (a - 5) * 512 against REF and (a - 5) * 32 against ALT, so the two tasks of one record sit on different rungs and the retry
    # list takes one task of a record without the other.  a = 37: 16 384 / 1 024; 133: 65 536 / 4 096; 517: 262 144 / 16 384;
    # 518: 262 656 / 16 416; 550: 279 040 / 17 440
    ref = b"T" * 201 + b"C" + b"A" * 517 + b"C" + b"T" * (2401 - 203 - 517)
    alt = ref[:202 + 37] + ref[202 + 517:]
    l0 = c.locus(ref, alt)
    for a in {1: (37, 133, 517, 518), 2: (37, 133, 517, 518, 550)}[top_tasks]:
        c.read(l0, cg_read(a), M=((a - 5) * 512, (a - 5) * 32))
    # four loci: the exact-capacity pairs of the first two slabs
    for t in (1024, 16385, 1025, 16384):
        a, b = MATCH_COUNT_AB[t]
        ref = b"T" * 201 + b"C" + b"A" * b + b"C" + b"T" * (2401 - 203 - b)
        c.read(c.locus(ref, ref[:100] + b"G" + ref[101:]), cg_read(a), M=(t, t))
    # locus: tandem repeats, 140 copies in the read against 20 (REF) and 40 (ALT)
    unit = b"ACGTTGCA"
    fl, fr = g[100:1300], g[2000:3200]
    lt = c.locus(fl + unit * 20 + fr, fl + unit * 40 + fr)
    c.read(lt, unit * 140)
    c.read(lt, _mutate(rng, unit * 140, 0.01))
    # ordinary 1 100-base reads against a 2 401-base locus (second slab).  (Every locus of this batch is above 2 400 bases, so the
    # banded stages in front of run_slow see no fast locus and sw_launches is that of a one-record slow batch.)
    p = 12000
    ll = c.locus(g[p - 1200:p + 1201], g[p - 1200:p] + _other(g[p:p + 1]) + g[p + 1:p + 1201])
    for k in range(2):
        c.read(ll, _mutate(rng, g[p - 500 - 50 * k:p + 600 - 50 * k], 0.01))
    batch, info = c.build()
    measured = match_counts(batch)
    promised = info["M"] >= 0
    assert np.array_equal(measured[promised], info["M"][promised]), "ladder_batch: the oracle counts other matches than the construction promises"
    info["M"] = measured
    assert info["slow"].all()
    return batch, info


def band_matters_batches():
    """Two repeat-rich batches whose every haplotype is above 2 400 bases (all slow) and on which the band changes some scores."""
    return [(b, nb) for _, b, nb in SB.repeat_rich_batches(trials=2, loci=6, reads=8, pad_range=(1210, 1300), seed=51)]


def _one_record(ref, alt, read):
    return SB.manual_batch([(ref, alt)], [[(0, 0, read)]], 2)


@functools.lru_cache(maxsize=None)
def limit_batches():
    """name -> (batch, flavours): the hard limits (30 000 bases accepted, 30 001 refused).
      a            a 30 000-base read (1 % substitutions, one 40-base deletion) against 30 000-base haplotypes; banded
      a_small      the same read against 2 401-base haplotypes; banded (the fallback of (a) when its time is too long)
      b            a 30 000-base read against a 201-base locus; both flavours
      c            a 1 025-base read against 30 000-base haplotypes; banded
      read_30001 / ref_30001 / alt_30001   (a)'s inputs with one of them a base longer: refused"""
    rng = np.random.default_rng(30000)
    g = _rand(rng, 30100)
    ref = g[:MAX_LEN]
    alt = ref[:15000] + _other(ref[15000:15001]) + ref[15001:]
    read = _mutate(rng, g[:9000] + g[9040:MAX_LEN + 40], 0.01)
    read1 = read + g[MAX_LEN + 40:MAX_LEN + 41]
    ref1 = g[:MAX_LEN + 1]
    alt1 = alt + g[MAX_LEN:MAX_LEN + 1]
    p = 15000
    out = {
        "a": (_one_record(ref, alt, read), ("banded",)),
        "a_small": (_one_record(g[p - 1200:p + 1201], g[p - 1200:p] + _other(g[p:p + 1]) + g[p + 1:p + 1201], read), ("banded",)),
        "b": (_one_record(g[p - 100:p + 101], g[p - 100:p] + _other(g[p:p + 1]) + g[p + 1:p + 101], read), ("banded", "full")),
        "c": (_one_record(ref, alt, _mutate(rng, g[p - 500:p + 525], 0.01)), ("banded",)),
        "read_30001": (_one_record(ref, alt, read1), ()),
        "ref_30001": (_one_record(ref1, alt, read), ()),
        "alt_30001": (_one_record(ref, alt1, read), ()),
    }
    return out


def even_offsets(batch, keep=None):
    """The batch without the records where keep is False, every read at an even offset of the arena (what to_nibbles needs)."""
    keep = np.ones(batch.n_records, bool) if keep is None else np.asarray(keep, bool)
    recs = batch.records[keep].copy()
    arena = bytearray()
    for i, r in enumerate(batch.records[keep]):
        if len(arena) & 1:
            arena += b"N"
        recs["read_off"][i] = len(arena)
        arena += bytes(batch.read_arena[int(r["read_off"]):int(r["read_off"]) + int(r["read_len"])])
    loci = batch.loci.copy()
    rec_locus = np.repeat(np.arange(batch.n_loci), batch.loci["rec_count"])
    cnt = np.bincount(rec_locus[keep], minlength=batch.n_loci)
    loci["rec_count"] = cnt
    loci["rec_begin"] = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    return PackedBatch(loci, recs, batch.hap_arena, np.frombuffer(bytes(arena), np.uint8))
