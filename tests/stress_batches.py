"""Batches shared by the stress tests (CPU: tests/test_certify_stress.py, tests/test_fastcore.py; GPU: tests/test_gpu_stress.py)
and by tools/certify_stress.py / tools/gpu_parity_stress.py, which run the same generators at full size.

  synthetic_batches   config-3 generator from clean to 30 % substitution errors, with indel loci, ragged read lengths and paddings
  repeat_rich_batches tandem-repeat genomes over 2- to 4-letter alphabets: hundreds of k-mer pieces per alignment
  near_repeat_batches iid genomes with short words copied a few bases further on (period 4-40, 6-12 bases): chance-like off-diagonal
                      matches AT CHOSEN DISTANCES from the main diagonal — the adversary of band_diag_kernel's far-piece condition
  far_apart_batches   reads whose two matching ends sit 100 - 170 bases apart on one diagonal (main or off-diagonal)
  real_sequence_batches loci at random positions of tests/golden/test_dna.fa (181 kb of real sequence: 2-3 x the chance 6-mer
                      matches of iid bases, satellite repeats in the tail)
  real_shape_batches  what real 10x reads add to `150M`: soft-clipped ends (the clip is random sequence), adapter tails, spliced
                      reads (the read skips an intron of the reference: CIGAR N), lower-case / N bases
  adversarial_batches shapes aimed at the certificate bounds (excursions over far pieces, tandem repeats, indel errors in reads, edge
                      bytes and lengths), built as numpy arrays: the GPU audit (tests/audit_util.py) runs 10 M alignments of them
"""
import numpy as np

from vartrix_amd import synth
from vartrix_amd.abi import LOCUS_DTYPE, RECORD_DTYPE, PackedBatch

ERROR_MODELS = [(0.005, 0, 0, 150, 100), (0.02, 0.3, 40, 150, 100), (0.05, 0.5, 60, 120, 60), (0.1, 0.2, 30, 100, 150),
                (0.15, 0.6, 50, 80, 40), (0.01, 0.8, 70, 150, 200), (0.3, 0.1, 0, 150, 100)]


def manual_batch(haps, reads_per_locus, n_barcodes):
    loci, recs, hb, rb = [], [], bytearray(), bytearray()
    for i, ((ref, alt), reads) in enumerate(zip(haps, reads_per_locus)):
        begin = len(recs)
        for cell, umi, seq in sorted(reads, key=lambda t: (t[0], t[1])):
            recs.append((len(rb), len(seq), cell, umi))
            rb += seq
        loci.append((i, begin, len(recs) - begin, len(hb), len(ref), len(hb) + len(ref), len(alt), 0))
        hb += ref + alt
    return PackedBatch(np.array(loci, LOCUS_DTYPE).reshape(-1), np.array(recs, RECORD_DTYPE).reshape(-1),
                       np.frombuffer(bytes(hb), np.uint8), np.frombuffer(bytes(rb), np.uint8))


def synthetic_batches(per_model=3, n_loci=150, reads=48):
    seed = 1000
    for (sub, indel, jitter, rl, pad) in ERROR_MODELS:
        for _ in range(per_model):
            seed += 1
            spec = synth.SynthSpec(n_loci=n_loci, n_barcodes=500, reads_per_locus=reads, indel_frac=indel, sub_error=sub,
                                   read_len_jitter=jitter, read_len=rl, padding=pad, seed=seed)
            yield ("sub %.3f indel %.1f jitter %d len %d pad %d" % (sub, indel, jitter, rl, pad), synth.make_batch(spec), 500)


def repeat_rich_batches(trials=12, loci=60, reads=24, pad_range=(30, 160), seed=2024):
    rng = np.random.default_rng(seed)
    for trial in range(trials):
        alpha = [b"ACGT", b"AC", b"AT", b"ACG"][trial % 4]
        units = [b"A", b"AC", b"AAT", b"ACGT", b"AAAAC", b"AG", b"T", b"CAG", b"ACACAT", b"GATTACA"]
        g = bytearray()
        while len(g) < 40000:
            g += units[int(rng.integers(0, len(units)))] * int(rng.integers(2, 40))
            g += bytes(rng.choice(list(alpha), int(rng.integers(0, 30))).tolist())
        g = bytes(g)
        haps, rds = [], []
        for _ in range(loci):
            p = int(rng.integers(pad_range[1] + 250, len(g) - pad_range[1] - 400))
            pad = int(rng.integers(pad_range[0], pad_range[1]))
            ref = g[p - pad:p + pad + 1]
            kind = rng.random()
            if kind < 0.5:
                alt = ref[:pad] + bytes([b"ACGT"[(b"ACGT".index(ref[pad:pad + 1]) + 1) % 4]]) + ref[pad + 1:]
            elif kind < 0.75:
                alt = ref[:pad + 1] + bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, 21))).tolist()) + ref[pad + 1:]
            else:
                alt = ref[:pad + 1] + ref[pad + 1 + int(rng.integers(1, min(20, pad - 1))):]
            haps.append((ref, alt))
            rl = []
            for _k in range(reads):
                ln = int(rng.integers(40, 200))
                s = max(p - int(rng.integers(0, ln)), 0)
                rd = bytearray(g[s:s + ln])
                for e in np.nonzero(rng.random(len(rd)) < rng.choice([0.0, 0.02, 0.08]))[0]:
                    rd[e] = b"ACGT"[int(rng.integers(0, 4))]
                if len(rd) >= 10:
                    rl.append((int(rng.integers(0, 30)), 0, bytes(rd)))
            rds.append(rl)
        yield ("repeat-rich, alphabet %s" % alpha.decode(), manual_batch(haps, rds, 30), 30)


def near_repeat_batches(trials=8, loci=80, reads=32, seed=4242):
    rng = np.random.default_rng(seed)
    for trial in range(trials):
        n_plant = [1, 2, 4, 8, 12, 3, 6, 16][trial % 8]
        haps, rds = [], []
        for _ in range(loci):
            pad = 100
            g = bytearray(rng.choice(list(b"ACGT"), 2 * pad + 1 + 400).tolist())
            for _p in range(n_plant):
                ln = int(rng.integers(6, 13))
                per = int(rng.integers(4, 41)) if rng.random() < 0.8 else int(rng.integers(1, 4))
                y0 = int(rng.integers(150, 150 + 2 * pad - ln - per))
                g[y0 + per:y0 + per + ln] = g[y0:y0 + ln]
            g = bytes(g)
            p = 200 + pad
            ref = g[p - pad:p + pad + 1]
            alt = ref[:pad] + bytes([b"ACGT"[(b"ACGT".index(ref[pad:pad + 1]) + 1) % 4]]) + ref[pad + 1:]
            haps.append((ref, alt))
            rl = []
            for _k in range(reads):
                ln = int(rng.integers(100, 151))
                s0 = p - int(rng.integers(0, ln))
                rd = bytearray(g[s0:s0 + ln])
                if s0 <= p < s0 + ln and rng.random() < 0.5:
                    rd[p - s0] = alt[pad]
                for e in np.nonzero(rng.random(len(rd)) < rng.choice([0.0, 0.005, 0.02]))[0]:
                    rd[e] = b"ACGT"[int(rng.integers(0, 4))]
                rl.append((int(rng.integers(0, 30)), 0, bytes(rd)))
            rds.append(rl)
        yield ("near repeats, %d planted per locus" % n_plant, manual_batch(haps, rds, 30), 30)


def far_apart_batches(trials=4, loci=60, reads=24, seed=515):
    """Reads whose two ends match the haplotype on ONE diagonal, 100 - 170 bases apart, with a middle that does not (random bases,
    or the haplotype's own bases at 30 - 60 % errors): same-diagonal joins at the long end of their range (the closed forms of the
    run bound are periodic in D: a division by 6 that is only right for short D goes unnoticed on ordinary reads), and the same
    construction copied onto an off-diagonal (the read's ends taken 7 - 40 bases further along the haplotype)."""
    rng = np.random.default_rng(seed)
    for trial in range(trials):
        haps, rds = [], []
        for _ in range(loci):
            pad = int(rng.integers(100, 140))
            g = bytes(rng.choice(list(b"ACGT"), 2 * pad + 1 + 500).tolist())
            p = 250 + pad
            ref = g[p - pad:p + pad + 1]
            alt = ref[:pad] + bytes([b"ACGT"[(b"ACGT".index(ref[pad:pad + 1]) + 1) % 4]]) + ref[pad + 1:]
            haps.append((ref, alt))
            rl = []
            for _k in range(reads):
                ln = int(rng.integers(150, 193))
                s0 = p - int(rng.integers(20, ln - 20))
                rd = bytearray(g[s0:s0 + ln])
                la, lb = int(rng.integers(6, 25)), int(rng.integers(6, 25))
                mid = slice(la, ln - lb)
                if trial % 2 == 0:
                    rd[mid] = bytes(rng.choice(list(b"ACGT"), ln - la - lb).tolist())
                else:
                    for e in np.nonzero(rng.random(ln - la - lb) < rng.choice([0.3, 0.45, 0.6]))[0]:
                        rd[la + int(e)] = b"ACGT"[int(rng.integers(0, 4))]
                if trial >= 2:                                   # the ends from another diagonal
                    sh = int(rng.integers(7, 41))
                    rd[:la] = g[s0 + sh:s0 + sh + la]
                    rd[ln - lb:] = g[s0 + sh + ln - lb:s0 + sh + ln]
                rl.append((int(rng.integers(0, 30)), 0, bytes(rd)))
            rds.append(rl)
        yield ("two ends far apart on one diagonal, variant %d" % trial, manual_batch(haps, rds, 30), 30)


def real_sequence_batches(trials=3, n_loci=300, reads=24, seed=9000):
    import os
    fasta = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_dna.fa")
    for trial in range(trials):
        err = [0.002, 0.01, 0.03][trial % 3]
        spec = synth.SynthSpec(n_loci=n_loci, n_barcodes=500, reads_per_locus=reads, sub_error=err, genome_fasta=fasta, seed=seed + trial)
        yield ("real sequence (test_dna.fa), %.1f %% errors" % (100 * err), synth.make_batch(spec), 500)


def real_shape_batches(trials=4, loci=80, reads=40, seed=77):
    """Reads as an aligner reports them for 10x libraries, against the haplotypes of SNV / indel loci at padding 100.  A read
    reaches the aligner with ALL its bases (`rec.seq()`, src/main.rs:896): soft clips included, introns excluded."""
    rng = np.random.default_rng(seed)
    acgt = list(b"ACGT")
    for trial in range(trials):
        g = bytes(rng.choice(acgt, 1000 * loci + 3000).tolist())
        haps, rds = [], []
        for i in range(loci):
            p = 1500 + 1000 * i
            pad = 100
            kind = rng.random()
            if kind < 0.6:
                ref_al, alt_al = g[p:p + 1], bytes([b"ACGT"[(b"ACGT".index(g[p:p + 1]) + 1 + int(rng.integers(0, 3))) % 4]])
            elif kind < 0.8:
                ref_al, alt_al = g[p:p + 1], g[p:p + 1] + bytes(rng.choice(acgt, int(rng.integers(1, 21))).tolist())
            else:
                k = int(rng.integers(1, 21))
                ref_al, alt_al = g[p:p + 1 + k], g[p:p + 1]
            ref = g[p - pad:p] + ref_al + g[p + len(ref_al):p + len(ref_al) + pad]
            alt = g[p - pad:p] + alt_al + g[p + len(ref_al):p + len(ref_al) + pad]
            haps.append((ref, alt))
            rl = []
            for _k in range(reads):
                ln = int(rng.choice([91, 98, 124, 150, 151]))
                allele_alt = rng.random() < 0.5
                # the "chromosome" this molecule came from: with the ALT allele spliced in, or not
                chrom = g[:p] + (alt_al if allele_alt else ref_al) + g[p + len(ref_al):]
                vpos = p
                shape = rng.random()
                if shape < 0.35:                                    # plain
                    s = vpos - int(rng.integers(0, ln))
                    rd = bytearray(chrom[s:s + ln])
                elif shape < 0.6:                                   # soft clip / adapter at the 3' end: random tail (111M13S and the like)
                    clip = int(rng.integers(4, 60))
                    s = vpos - int(rng.integers(0, ln - clip))
                    rd = bytearray(chrom[s:s + ln - clip]) + bytearray(rng.choice(acgt, clip).tolist())
                elif shape < 0.75:                                  # soft clip at the 5' end (template-switch oligo)
                    clip = int(rng.integers(4, 40))
                    s = vpos - int(rng.integers(0, ln - clip))
                    rd = bytearray(rng.choice(acgt, clip).tolist()) + bytearray(chrom[s:s + ln - clip])
                elif shape < 0.9:                                   # spliced: the read skips an intron right or left of the variant
                    intron = int(rng.integers(60, 2000))
                    a = int(rng.integers(20, ln - 20))              # bases before the junction
                    if rng.random() < 0.5:                          # variant in the first exon
                        s = vpos - int(rng.integers(0, a))
                        rd = bytearray(chrom[s:s + a]) + bytearray(chrom[s + a + intron:s + a + intron + ln - a])
                    else:                                           # variant in the second exon
                        s2 = vpos - int(rng.integers(0, ln - a))
                        rd = bytearray(chrom[max(s2 - intron - a, 0):max(s2 - intron - a, 0) + a]) + bytearray(chrom[s2:s2 + ln - a])
                else:                                               # poly-A tail + N bases
                    tail = int(rng.integers(5, 50))
                    s = vpos - int(rng.integers(0, ln - tail))
                    rd = bytearray(chrom[s:s + ln - tail]) + bytearray(b"A" * tail)
                    for e in rng.integers(0, len(rd), 2):
                        rd[int(e)] = ord("N")
                for e in np.nonzero(rng.random(len(rd)) < 0.006)[0]:
                    rd[e] = b"ACGT"[int(rng.integers(0, 4))]
                rl.append((int(rng.integers(0, 30)), int(rng.integers(0, 5)), bytes(rd)))
            rds.append(rl)
        yield ("real-read shapes (clips, adapters, splices, poly-A, N), trial %d" % trial, manual_batch(haps, rds, 30), 30)


# ---- adversarial batches: shapes aimed at the certificate bounds (vtx_fast_core.h, vtx_band_trim.h), built as arrays ----
#   excursion    a read copies its haplotype; inside a gap of D = 12 - 21 bases 6 - 9 bases are overwritten with haplotype bases taken
#                1 - 6 diagonals away (an exact off-diagonal run between two main runs: the shape of the round-6 join_gap3 bug), plus
#                0 - 3 more errors in the gap and 0 - 3 % substitutions elsewhere
#   repeats      tandem repeats (unit 1 - 12 bases) and homopolymers in haplotype and read, one across the variant (an indel there
#                is a unit expansion / contraction), others where read ends fall
#   read_indels  indel ERRORS in the reads, 1 - 4 bases at 0.2 - 2 % per base, with substitutions: the read leaves its diagonal part-way
#   edges        N runs in reads and flanks, lower-case and IUPAC bytes in REF / ALT, a few haplotypes with a byte >= 0x80 (the
#                kernel's `hib` path, no twin lists), reads longer than the window overhanging both ends, read lengths at the
#                mask-word edges (63/64/65 ... 255/256) and shorter than a k-mer
ADV_FAMILIES = ("excursion", "repeats", "read_indels", "edges")
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_IUPAC = np.frombuffer(b"RYKMSWBDHVNacgtn", np.uint8)
_EDGE_LENS = np.array([63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256])
_ADV_OV, _ADV_MAXIND, _ADV_LMAX = 300, 20, 300


def _pieces(M, lo, hi):
    """M[i, lo[i]:hi[i]] of every row, concatenated."""
    cols = np.arange(M.shape[1])[None, :]
    return M[(cols >= lo[:, None]) & (cols < hi[:, None])]


def _plant_repeats(rng, g, rows, starts, lens, max_unit=12):
    """Overwrite g[rows, starts:starts + lens] with a tandem repeat of a random unit of 1 - max_unit bases; returns (unit, u)."""
    n = len(rows)
    u = rng.integers(1, max_unit + 1, n)
    u = np.where(rng.random(n) < 0.3, 1, u)                      # homopolymers
    unit = _ACGT[rng.integers(0, 4, (n, max_unit))]
    j = np.arange(g.shape[1])[None, :] - starts[:, None]
    inr = (j >= 0) & (j < lens[:, None])
    rep = np.take_along_axis(unit, np.mod(np.maximum(j, 0), u[:, None]), axis=1)
    g[rows] = np.where(inr, rep, g[rows])
    return unit, u


def _adversarial_chunk(rng, fam, reads, pads):
    """One chunk of loci (fam[i]: index into ADV_FAMILIES): haplotype bytes (REF, ALT of each locus in turn), their lengths, read
    bytes, read lengths."""
    nl = len(fam)
    pmax = pads[1]
    C = _ADV_OV + pmax                                            # molecule column of the variant
    GW = C + pmax + 1 + 2 * _ADV_MAXIND + _ADV_OV + 8
    ex, rp, ri, ed = (fam == k for k in range(4))
    g = _ACGT[rng.integers(0, 4, (nl, GW), dtype=np.uint8)]
    pad = rng.integers(pads[0], pmax + 1, nl)
    pad = np.where(ex | ri, np.maximum(pad, 60), pad)
    # repeats: one across the variant, two more anywhere in the window or just outside it
    unit, u = np.zeros((nl, 12), np.uint8), np.ones(nl, np.int64)
    r = np.nonzero(rp)[0]
    if len(r):
        ln = rng.integers(8, 60, len(r))
        unit[r], u[r] = _plant_repeats(rng, g, r, C - rng.integers(0, ln), ln)
        for _ in range(2):
            ln = rng.integers(6, 40, len(r))
            _plant_repeats(rng, g, r, C + rng.integers(-pmax - 150, pmax + 150, len(r)), ln)
    # edges: N runs in the flanks (reads copy them)
    e = np.nonzero(ed & (rng.random(nl) < 0.4))[0]
    if len(e):
        s = C + rng.integers(-pmax, pmax, len(e))
        j = np.arange(GW)[None, :] - s[:, None]
        g[e] = np.where((j >= 0) & (j < rng.integers(1, 13, len(e))[:, None]), ord("N"), g[e])
    # the variant: SNV, insertion or deletion of 1 - 20 bases (the alt molecule through an index map)
    kind = rng.choice(3, nl, p=[0.5, 0.25, 0.25])
    k = rng.integers(1, _ADV_MAXIND + 1, nl)
    k = np.where(kind == 0, 0, k)
    cols = np.arange(GW)[None, :]
    src = np.where(cols <= C, cols, np.where((kind == 1)[:, None], cols - k[:, None], cols + k[:, None]))
    alt = np.take_along_axis(g, np.clip(src, 0, GW - 1), axis=1)
    ins = (kind == 1)[:, None] & (cols > C) & (cols <= C + k[:, None])
    ins_base = np.where(rp[:, None], np.take_along_axis(unit, np.mod(cols - C - 1, u[:, None]), axis=1),
                        _ACGT[rng.integers(0, 4, (nl, GW), dtype=np.uint8)])
    alt = np.where(ins, ins_base, alt)
    snv = np.nonzero(kind == 0)[0]
    alt[snv, C] = _ACGT[(np.searchsorted(_ACGT, g[snv, C]) % 4 + rng.integers(1, 4, len(snv))) % 4]
    mol = np.stack([g, alt], axis=1).reshape(2 * nl, GW)
    ref_len = 2 * pad + 1
    alt_len = ref_len + np.where(kind == 1, k, -k)
    # reads
    n = nl * reads
    loc = np.repeat(np.arange(nl), reads)
    a = rng.integers(0, 2, n)
    hl = np.where(a == 1, alt_len[loc], ref_len[loc])
    L = 150 - rng.integers(0, 51, n)
    red = ed[loc]
    pick = rng.random(n)
    L = np.where(red & (pick < 0.6), _EDGE_LENS[rng.integers(0, len(_EDGE_LENS), n)], L)
    L = np.where(red & (pick >= 0.6) & (pick < 0.7), rng.integers(1, 6, n), L)                     # shorter than a k-mer
    over = red & (pick >= 0.7)                                                                     # longer than the window
    L = np.where(over, np.minimum(hl + rng.integers(2, 60, n), _ADV_LMAX), L)
    s = C - rng.integers(0, np.maximum(L, 1))
    s = np.where(over, C - pad[loc] - rng.integers(1, np.maximum(L - hl, 2)), s)
    s = np.clip(s, 0, GW - _ADV_LMAX - 2 * _ADV_MAXIND - 8)
    # the reads as one flat array: base t of read r at roff[r] + t
    roff = np.cumsum(L) - L
    rec = np.repeat(np.arange(n), L)
    tpos = (np.arange(len(rec)) - roff[rec]).astype(np.int32)
    src = s[rec].astype(np.int32) + tpos
    # read indels: the source position of base t shifts by the indels before it; inserted bases are random
    rir = np.nonzero(ri[loc])[0]
    insm = None
    if len(rir):
        lmax = int(L[rir].max())
        valid = np.arange(lmax)[None, :] < L[rir, None]
        rate = rng.uniform(0.002, 0.02, len(rir))
        ev = (rng.random((len(rir), lmax), dtype=np.float32) < rate[:, None]) & valid
        elen = rng.integers(1, 5, (len(rir), lmax), dtype=np.int32)
        eins = rng.random((len(rir), lmax), dtype=np.float32) < 0.5
        shift = np.cumsum(np.where(ev, np.where(eins, -elen, elen), 0), axis=1, dtype=np.int32)
        insm = np.zeros((len(rir), lmax), bool)
        for q in range(4):
            m = ev & eins & (elen > q)
            insm[:, q:] |= m[:, :lmax - q]
        at = (roff[rir, None] + np.arange(lmax)[None, :])[valid]
        src[at] += shift[valid]
        insm = at[insm[valid]]
    np.clip(src, 0, GW - 1, out=src)
    molrow = (2 * loc + a) * GW
    rd = mol.reshape(-1)[molrow[rec] + src]
    if insm is not None:
        rd[insm] = _ACGT[rng.integers(0, 4, len(insm))]
    # excursions: 6 - 9 bases of a D = 12 - 21 gap taken from 1 - 6 diagonals away, 0 - 3 more errors in the gap.  A quarter of them
    # over D = 23 - 30 (join_gap3's floor of 11 above D = 22); half of the reads get a second one anywhere
    xr = np.nonzero(ex[loc] & (L >= 60))[0]
    for second in (False, True):
        if second:
            xr = xr[rng.random(len(xr)) < 0.5]
        if not len(xr):
            break
        D = np.where(rng.random(len(xr)) < 0.25, rng.integers(23, 31, len(xr)), rng.integers(12, 22, len(xr)))
        gs = rng.integers(5, L[xr] - D - 4)
        if not second:
            # half of them leave a run of 8 - 20 bases between the gap and a read end: joined, that run is worth about a join (the
            # round-6 task: the longer run alone was the certificate, the join priced one too high cost the excursion's score)
            near = rng.random(len(xr)) < 0.5
            endrun = rng.integers(8, 21, len(xr))
            gs = np.where(near, np.where(rng.random(len(xr)) < 0.5, endrun, L[xr] - D - endrun), gs)
        ne = rng.integers(6, 10, len(xr))
        o = rng.integers(0, D - ne + 1)
        # (4 - 6 diagonals, 70 %: far pieces that condition (*) still admits; 1 - 3: the corridor and the edge of the far-piece condition)
        dl = np.where(rng.random(len(xr)) < 0.7, rng.integers(4, 7, len(xr)), rng.integers(1, 4, len(xr))) * rng.choice([-1, 1], len(xr))
        for q in range(9):
            on = q < ne
            p = gs[on] + o[on] + q
            rd[roff[xr[on]] + p] = mol.reshape(-1)[molrow[xr[on]] + s[xr[on]] + p + dl[on]]
        for q in range(3):
            on = rng.integers(0, 4, len(xr)) > q
            rd[roff[xr[on]] + (gs + rng.integers(0, D))[on]] = _ACGT[rng.integers(0, 4, int(on.sum()))]
    # background substitutions (a random base: the same one now and then)
    bg = np.select([ex[loc], rp[loc], ri[loc]], [rng.choice([0.0, 0.005, 0.01, 0.03], n), rng.choice([0.0, 0.005, 0.02], n), rng.uniform(0, 0.01, n)], 0.005)
    ns = rng.binomial(L, bg)
    rows = np.repeat(np.arange(n), ns)
    rd[roff[rows] + (rng.random(len(rows)) * L[rows]).astype(np.int64)] = _ACGT[rng.integers(0, 4, len(rows))]
    # edges: N runs of 1 - 8 bases in reads
    nr = np.nonzero(red & (rng.random(n) < 0.2) & (L > 0))[0]
    if len(nr):
        st = rng.integers(0, L[nr])
        nl_ = rng.integers(1, 9, len(nr))
        for q in range(8):
            on = (q < nl_) & (st + q < L[nr])
            rd[roff[nr[on]] + st[on] + q] = ord("N")
    # edges: lower-case / IUPAC bytes in REF and ALT (after the reads were copied), bytes >= 0x80 in a few haplotypes
    eh = np.nonzero(ed)[0]
    if len(eh):
        w = np.abs(cols - C) <= pad[eh, None] + _ADV_MAXIND
        sub = mol[2 * eh[:, None] + np.arange(2)[None, :]]                       # (ne, 2, GW)
        hit = (rng.random(sub.shape) < 0.02) & w[:, None, :] & (rng.random(len(eh))[:, None, None] < 0.5)
        lowc = np.where(np.isin(sub, _ACGT), sub | 0x20, sub)
        sub = np.where(hit, np.where(rng.random(sub.shape) < 0.5, lowc, _IUPAC[rng.integers(0, len(_IUPAC), sub.shape)]), sub)
        hb = rng.random(len(eh)) < 0.05
        pos = C + rng.integers(-20, 21, len(eh))
        sub[hb, rng.integers(0, 2, len(eh))[hb], pos[hb]] = rng.integers(0x80, 0x100, int(hb.sum()))
        mol[2 * eh[:, None] + np.arange(2)[None, :]] = sub
    hap_lo = np.repeat(C - pad, 2)
    hap_len = np.stack([ref_len, alt_len], axis=1).reshape(-1)
    return _pieces(mol, hap_lo, hap_lo + hap_len), hap_len, rd, L


def adversarial_batch(n_loci, reads, seed, families=ADV_FAMILIES, n_barcodes=500, chunk_loci=2048, pads=(20, 110)):
    """One batch, each locus of one of `families` (names of ADV_FAMILIES), chosen at random per locus; paddings drawn from `pads`
    (the default keeps every haplotype within 255 bases; above, the device scores the batch on round 3's path: band_refine_kernel)."""
    rng = np.random.default_rng(seed)
    fam_ids = np.array([ADV_FAMILIES.index(f) for f in families])
    loci = np.zeros(n_loci, LOCUS_DTYPE)
    recs = np.zeros(n_loci * reads, RECORD_DTYPE)
    hap_parts, read_parts = [], []
    hoff = roff = 0
    for c0 in range(0, n_loci, chunk_loci):
        nl = min(chunk_loci, n_loci - c0)
        hb, hl, rd, L = _adversarial_chunk(rng, fam_ids[rng.integers(0, len(fam_ids), nl)], reads, pads)
        lc = loci[c0:c0 + nl]
        lc["row"] = np.arange(c0, c0 + nl)
        lc["rec_begin"] = (c0 + np.arange(nl)) * reads
        lc["rec_count"] = reads
        off = hoff + np.cumsum(hl) - hl
        lc["ref_off"], lc["alt_off"] = off[0::2], off[1::2]
        lc["ref_len"], lc["alt_len"] = hl[0::2], hl[1::2]
        hoff += len(hb)
        hap_parts.append(hb)
        rc = recs[c0 * reads:(c0 + nl) * reads]
        rc["read_off"] = roff + np.cumsum(L) - L
        rc["read_len"] = L
        rc["cell_index"] = np.sort(rng.integers(0, n_barcodes, (nl, reads)), axis=1).reshape(-1)
        roff += len(rd)
        read_parts.append(rd)
    read_parts.append(np.zeros(16, np.uint8))                    # (a kernel may load a word past the last read)
    return PackedBatch(loci, recs, np.concatenate(hap_parts), np.concatenate(read_parts))


def adversarial_batches(n_loci=60, reads=32, seed=31337, families=ADV_FAMILIES, mixed=False, n_barcodes=500, pads=(20, 110)):
    """(label, batch, n_barcodes): one batch per family, or (mixed=True) one batch of all of them mixed."""
    if mixed:
        yield ("adversarial, %s mixed" % "/".join(families), adversarial_batch(n_loci, reads, seed, families, n_barcodes, pads=pads), n_barcodes)
        return
    for i, f in enumerate(families):
        yield ("adversarial, %s" % f, adversarial_batch(n_loci, reads, seed + i, (f,), n_barcodes, pads=pads), n_barcodes)
