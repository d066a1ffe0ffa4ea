"""Inputs for the tests of the SEGMENTED device-ingest plan (sparse loci): an authored two-contig genome, a BAM with reads all over
it and a VCF of a few loci far apart — in the manner of tests/test_host.py::test_index_guided_skipping_on_a_sparse_vcf, but on contigs
long enough that the stretches of two far loci (a locus' window to four 16 kb windows behind it) do not meet.

Everything is drawn from seeded generators, so the inflated stream (record bytes, BGZF block cuts, index) is the same wherever the
files are authored; only the compressed sizes depend on the zlib at hand."""
import os
import struct
import zlib

import numpy as np

# the developer library's knob: the "sparse" thresholds of vtxh_plan_ingest as if 64 MiB were 256 KiB (per locus: 4 KiB, merge
# distance: 16 KiB of inflated BAM)
SPARSE_KIB = "256"
CONTIGS = (("cA", 1_200_000), ("cB", 400_000))
# contig, 0-based position.  Two loci 200 bases apart; one that spliced reads reach from 30 kb away; one where no read lies (no read
# is authored within 20 kb of it); loci on both contigs
LOCI = (("cA", 50_000), ("cA", 300_000), ("cA", 300_200), ("cA", 640_000), ("cA", 900_000), ("cB", 100_000), ("cB", 330_000))
EMPTY = ("cA", 900_000)
N_BARCODES = 40


def author(tmp_path, block=4000, index="linear", seed=21, n_background=26000):
    """-> dict(vcf=, bam=, fasta=, cell_barcodes=) under tmp_path."""
    from oracle import bamwriter
    rng = np.random.default_rng(seed)
    d = str(tmp_path)
    genome = {}
    fa = os.path.join(d, "seg.fa")
    with open(fa, "wb") as fh, open(fa + ".fai", "w") as fai:
        off = 0
        for name, ln in CONTIGS:
            seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, ln)].tobytes()
            genome[name] = seq
            hdr = (">%s\n" % name).encode()
            fh.write(hdr)
            off += len(hdr)
            fai.write("%s\t%d\t%d\t60\t61\n" % (name, ln, off))
            body = b"".join(seq[i:i + 60] + b"\n" for i in range(0, ln, 60))
            fh.write(body)
            off += len(body)
    bcs = ["".join("ACGT"[c] for c in rng.integers(0, 4, 16)) + "-1" for _ in range(N_BARCODES)]
    bcp = os.path.join(d, "seg_bcs.tsv")
    open(bcp, "w").write("\n".join(bcs) + "\n")
    vcf = os.path.join(d, "seg.vcf")
    with open(vcf, "w") as fh:
        fh.write("##fileformat=VCFv4.2\n" + "".join("##contig=<ID=%s,length=%d>\n" % c for c in CONTIGS) +
                 "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for name, p in LOCI:
            ref = chr(genome[name][p])
            fh.write("%s\t%d\t.\t%s\t%s\t.\t.\t.\n" % (name, p + 1, ref, "ACGT"[("ACGT".index(ref) + 1) % 4]))
    tid_of = {name: t for t, (name, _) in enumerate(CONTIGS)}
    recs = []

    def tags(k):
        return [("CB", "Z", bcs[int(rng.integers(0, N_BARCODES))]), ("UB", "Z", "U%03d" % (k % 97))]
    total = sum(ln for _, ln in CONTIGS)
    for k in range(n_background):                                       # reads all over both contigs
        name, ln = CONTIGS[0] if int(rng.integers(0, total)) < CONTIGS[0][1] else CONTIGS[1]
        start = int(rng.integers(0, ln - 200))
        rl = int(rng.integers(60, 151))
        if name == EMPTY[0] and abs(start - EMPTY[1]) < 20_000:
            continue
        flag = 0 if k % 11 else (1024 if k % 22 else 256)                # some duplicates and secondary alignments
        recs.append((tid_of[name], start, bamwriter.record(tid_of[name], start, "r%05d" % k, genome[name][start:start + rl].decode(),
                                                           "%dM" % rl, flag=flag, mapq=int(rng.integers(0, 61)), tags=tags(k))))
    for name, p in LOCI:
        if (name, p) == EMPTY:
            continue
        seq = genome[name]
        for k in range(24):                                             # reads at the loci
            start = p - int(rng.integers(0, 100))
            recs.append((tid_of[name], start, bamwriter.record(tid_of[name], start, "l%s%d_%d" % (name, p, k), seq[start:start + 120].decode(),
                                                               "120M", mapq=60, tags=tags(k) if k % 7 else tags(k)[:1])))
        if p == 640_000:
            for k in range(3):                                          # spliced across 30 kb INTO the locus
                s0 = p - 30_050 - 7 * k
                sq = seq[s0:s0 + 40] + seq[p - 10:p + 70]
                recs.append((tid_of[name], s0, bamwriter.record(tid_of[name], s0, "sp%d" % k, sq.decode(), "40M%dN80M" % (p - 10 - (s0 + 40)),
                                                                mapq=60, tags=tags(k))))
    recs.sort(key=lambda t: (t[0], t[1]))
    bam = os.path.join(d, "seg_%d_%s.bam" % (block, index))
    bamwriter.write_bam(bam, list(CONTIGS), [r for _, _, r in recs], block=block, index=index)
    return dict(vcf=vcf, bam=bam, fasta=fa, cell_barcodes=bcp)


def bgzf_blocks(path):
    """Every BGZF block of the file: (payload offset, payload bytes, ISIZE)."""
    f = open(path, "rb").read()
    o, out = 0, []
    while o + 18 <= len(f):
        xlen = struct.unpack_from("<H", f, o + 10)[0]
        bsize = struct.unpack_from("<H", f, o + 16)[0] + 1
        out.append((o + 12 + xlen, bsize - 12 - xlen - 8, struct.unpack_from("<I", f, o + bsize - 4)[0]))
        o += bsize
    return f, out


def inflate(f, blocks):
    out = bytearray()
    for b in blocks:
        piece = zlib.decompress(f[int(b["coff"]):int(b["coff"]) + int(b["clen"])], -15)
        assert len(piece) == int(b["isize"])
        out += piece
    return bytes(out)
