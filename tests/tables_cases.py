"""The haplotype corpus of the table checks (tests/tables_model.py): one function per family, each returning (label, batch, n_barcodes)
for a number of reads per locus.  Every family comes at SHALLOW and at DEEP reads per locus: vtx_band.hip's band_use_t3 switches at 16
tasks (8 reads) per locus, and with t3[] band_tables_kernel has another LDS layout and zeroes more words.

What a case is meant to hold is stated here as data (the *_PREMISES tables, the named haplotypes) and proven from the bytes alone by
tests/test_tables_model.py; nothing here asks a table builder.  Cases found by search were searched on the CPU with numpy's
default_rng at the seeds written next to them; the found bytes are rebuilt from the seed (or stand here as bytes).

Two cases of the list this corpus was written to cannot exist, and stand here in their nearest possible form:
  * a haplotype with exactly 61 ordered pairs of equal k-mers: a k-mer with c occurrences gives c (c - 1) ordered pairs, an even number,
    so the count is even.  The smallest count above TW_MAX = 60 is 62 (TWINS_62).
  * 65 or more buckets on one of the 128 link slots within one round of 64 positions: a round links 64 positions, and with 1 024 buckets a
    slot (bucket & 127) serves 8 buckets.  SLOT_CROWD puts ALL 64 positions of a round on one slot, over three distinct buckets: every
    trip of the link retires one position, and buckets that share the slot wait for each other.

A batch must stay in ONE banded pass for its dump to hold every table (vtx_api.hip, run_banded: two passes when the loci above 255 bases
are at most an eighth of the loci): one_pass() says so, and every family keeps to it.
"""
import os

import numpy as np

from vartrix_amd import synth

import stress_batches as SB

SHALLOW, DEEP = 4, 9            # reads per locus: 8 and 18 tasks, either side of band_use_t3's 16
HERE = os.path.dirname(os.path.abspath(__file__))
FILLER_READ = b"ACGTTGCAAGGCTTAC"          # for a locus whose REF is too short to cut a read from


def rnd(seed, n):
    return bytes(np.random.default_rng(seed).choice(list(b"ACGT"), n).tolist())


def one_pass(batch):
    hl = np.maximum(batch.loci["ref_len"], batch.loci["alt_len"])
    n_long = int((hl > 255).sum())
    return not (n_long and int((hl <= 255).sum()) and 8 * n_long <= batch.n_loci)


def uses_t3(batch):
    return (2 * batch.n_records) // max(batch.n_loci, 1) >= 16


def reads_of(ref, alt, reads):
    """`reads` reads of up to 150 bases cut from REF at spread starts (from ALT, or a fixed read, when REF is shorter than 16 bases)."""
    src = ref if len(ref) >= 16 else (alt if len(alt) >= 16 else FILLER_READ)
    ln = min(150, len(src))
    return [(k, 0, src[(k * max(len(src) - ln, 0)) // max(reads - 1, 1):][:ln]) for k in range(reads)]


def batch_of(haps, reads, nb=16):
    b = SB.manual_batch(haps, [reads_of(r, a, reads) for r, a in haps], nb)
    assert one_pass(b) and uses_t3(b) == (reads >= 8)
    return b, nb


# ---- lengths --------------------------------------------------------------------------------------------------------------------------
# 63 + 5, 64 + 5, 65 + 5, 128 + 5, 129 + 5: one, two and three rounds of 64 positions in the link and flag loops; 255 / 256 / 257: the edge of
# the two-byte match entries and of the twin list.  Four of the eleven loci are above 255 bases: one pass.
LENGTHS = (0, 1, 5, 6, 7, 68, 69, 70, 133, 134, 255, 256, 257)
LENGTH_PAIRS = ((0, 68), (1, 69), (5, 70), (6, 133), (7, 134), (255, 6), (68, 0), (256, 5), (257, 1), (7, 256), (134, 257))


def lengths(reads):
    haps = [(rnd(300 + 2 * i, a), rnd(301 + 2 * i, b)) for i, (a, b) in enumerate(LENGTH_PAIRS)]
    b, nb = batch_of(haps, reads)
    return "lengths, %d reads per locus" % reads, b, nb


# ---- one bucket, many entries ------------------------------------------------------------------------------------------------------------
# A repeat of a primitive unit of u bases has u distinct k-mers; at u (c - 1) + 6 bases the one at phase 0 occurs c times, the others c - 1.
REPEAT_UNITS = (b"A", b"AC", b"ACG", b"ACGT", b"AACGTC", b"ACGTTGCATGGA")
REPEAT_COUNTS = (63, 64, 65, 128, 129)


def repeat_haps():
    """[(unit, c, haplotype)]: the bucket of the phase-0 k-mer holds c entries."""
    return [(u, c, (u * (c + 6))[:len(u) * (c - 1) + 6]) for u in REPEAT_UNITS for c in REPEAT_COUNTS]


def one_bucket(reads):
    haps = []
    for u, c, h in repeat_haps():
        mid = len(h) // 2
        haps.append((h, h[:mid] + (b"T" if h[mid:mid + 1] != b"T" else b"G") + h[mid + 1:]))     # ALT: the repeat broken in the middle
    b, nb = batch_of(haps, reads)
    return "one bucket, many entries, %d reads per locus" % reads, b, nb


# ---- a long batch ---------------------------------------------------------------------------------------------------------------------
LONG_LENGTHS = ((300, 280), (256, 512), (601, 600), (257, 30), (1000, 999), (420, 421))
LONG_LIMIT = 2400                # the fast path's limit (vtx_device.h: VTX_FAST_HAP_LEN)


def long_batch(reads):
    """Every locus above 255 bases; the last one a pair at the fast path's limit, REF random (the reads are cut from it), ALT a homopolymer: a
    chain of 2 395 entries."""
    haps = [(rnd(500 + 2 * i, a), rnd(501 + 2 * i, b)) for i, (a, b) in enumerate(LONG_LENGTHS)]
    haps.append((rnd(599, LONG_LIMIT), b"A" * LONG_LIMIT))
    b, nb = batch_of(haps, reads)
    return "long haplotypes, %d reads per locus" % reads, b, nb


# ---- twin-list edges ------------------------------------------------------------------------------------------------------------------
def _plant(base, src, dst, n):
    """base with base[src:src + n] copied to dst."""
    return base[:dst] + base[src:src + n] + base[dst + n:]


_Z200, _Z256, _Z257 = rnd(155, 200), rnd(234, 256), rnd(234, 257)          # seeds searched from 100 on: no k-mer twice; the plant offsets below searched from 95 on for the exact counts
TWINS_60 = _plant(_Z200, 10, 120, 35)                                        # 30 k-mers twice
TWINS_62 = _plant(_Z200, 10, 120, 36)                                        # 31 k-mers twice: the smallest count above TW_MAX
TWINS_60_TRIPLE = _plant(_plant(_Z200, 10, 100, 6), 10, 154, 33)             # one k-mer three times (6 pairs), 27 twice (54)
TWINS_60_AT_256 = _plant(_Z256, 10, 100, 35)
TWINS_2_AT_257 = _plant(_Z257, 10, 102, 6)
TWINS_2_7F = _plant(_Z200, 10, 100, 6)[:60] + b"\x7f" + _plant(_Z200, 10, 100, 6)[61:]
TWINS_2_80 = TWINS_2_7F[:60] + b"\x80" + TWINS_2_7F[61:]
# haplotype -> (ordered pairs, tw[0] the header promises; None: TW_NONE)
TWIN_PREMISES = ((TWINS_60, 60, 60), (TWINS_62, 62, None), (TWINS_60_TRIPLE, 60, 60), (TWINS_60_AT_256, 60, 60), (TWINS_2_AT_257, 2, None),
                 (TWINS_2_7F, 2, 2), (TWINS_2_80, 2, None))


def twin_edges(reads):
    haps = [(h, _Z200) for h, _, _ in TWIN_PREMISES[:4]] + [(_Z200[:150], TWINS_2_AT_257), (TWINS_2_7F, TWINS_2_80), (TWINS_2_80, TWINS_60)]
    b, nb = batch_of(haps, reads)
    return "twin-list edges, %d reads per locus" % reads, b, nb


# ---- tags and buckets (1 024 buckets) -------------------------------------------------------------------------------------------------------
SHARED_TAG = rnd(22, 200)           # seed searched from 1 on: no k-mer twice; CGGTCG and GCTTAT share the bucket AND the hash's top nibble
SHARED_TAG_KMERS = (b"CGGTCG", b"GCTTAT")
SHARED_BUCKET = rnd(23, 200)        # two distinct k-mers in one bucket (any 200 random bases have some; proven by the test)
SLOT_CROWD = b"QXz" * 43            # the three k-mers of this repeat: buckets 548, 164, 420 = link slot 36, all of them


def tags_and_buckets(reads):
    haps = [(SHARED_TAG, SHARED_BUCKET), (SLOT_CROWD, SLOT_CROWD[:64] + b"A" + SLOT_CROWD[65:]), (SHARED_BUCKET, SHARED_TAG[:100])]
    b, nb = batch_of(haps, reads)
    return "tags and buckets, %d reads per locus" % reads, b, nb


# ---- alphabet -------------------------------------------------------------------------------------------------------------------------
_A = rnd(700, 180)
ALPHABET = {
    "N runs": _A[:40] + b"N" * 3 + _A[43:90] + b"N" * 14 + _A[104:],
    "lower case": _A[:50] + _A[50:120].lower() + _A[120:],
    "IUPAC": _A[:30] + b"RYKMSWBDHVN" + _A[41:100] + b"acgtn" + _A[105:],
    "a byte >= 0x80 first": b"\x90" + _A[1:],
    "a byte >= 0x80 in the middle": _A[:90] + b"\xc1" + _A[91:],
    "a byte >= 0x80 last": _A[:-1] + b"\xff",
    "NNNNNN next to GGGGGG": _A[:60] + b"NNNNNN" + b"GGGGGG" + _A[72:],
}


def alphabet(reads):
    names = list(ALPHABET)
    haps = [(ALPHABET[n], ALPHABET[names[(i + 3) % len(names)]][:170 - 7 * i]) for i, n in enumerate(names)]
    b, nb = batch_of(haps, reads)
    return "alphabet, %d reads per locus" % reads, b, nb


# ---- ordinary ---------------------------------------------------------------------------------------------------------------------------
def ordinary_synth(reads):
    """The generator of bench.py with every read kept: 6 reads per locus (no t3[]) or 12 (t3[] built)."""
    n = 6 if reads < 8 else 12
    b = synth.make_batch(synth.SynthSpec(n_loci=48, n_barcodes=100, reads_per_locus=n, unlisted_frac=0.0, seed=4100 + n))
    assert one_pass(b) and uses_t3(b) == (n >= 8)
    return "ordinary, synthetic, %d reads per locus" % n, b, 100


def ordinary_real(reads):
    n = 6 if reads < 8 else 12
    b = synth.make_batch(synth.SynthSpec(n_loci=48, n_barcodes=100, reads_per_locus=n, unlisted_frac=0.0, seed=4200 + n,
                                         genome_fasta=os.path.join(HERE, "golden", "test_dna.fa")))
    assert one_pass(b) and uses_t3(b) == (n >= 8)
    return "ordinary, test_dna.fa, %d reads per locus" % n, b, 100


FAMILIES = {"lengths": (lengths,), "one bucket, many entries": (one_bucket,), "a long batch": (long_batch,), "twin-list edges": (twin_edges,),
            "tags and buckets": (tags_and_buckets,), "alphabet": (alphabet,), "ordinary": (ordinary_synth, ordinary_real)}


def cases(family, depths=(SHALLOW, DEEP)):
    """[(label, batch, n_barcodes)] of one family: every batch of it at every depth."""
    return [f(reads) for f in FAMILIES[family] for reads in depths]
