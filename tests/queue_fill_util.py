"""Batches for tests/test_gpu_queue_fill.py: 2 loci x 16 reads each (32 tasks per locus: band_diag_kernel's blocks of three rows are on
by depth), built like those of tests/stress_batches.py (manual_batch).  The reads are the shapes at which the block arithmetic of the
queue fill can go wrong — a block of three rows ends at a row e = m - K (mod 3), the blocks alternate between the two lanes of a record
by e mod 6, and the rows live in 64-bit mask words:

  lengths     6, 7, 8, 9, 11 (m - K < 3: the first block starts below row 0), 63 - 66 and 127 - 130 (blocks straddle the mask words),
              150, 192 (three mask words full); 193, 250, 256 (four mask words).  m - K takes every residue mod 6.
  placement   0, 1, 2, 3, 5 and 49 bases of the read hanging over the haplotype's window, on the left and on the right (the rows without
              a main-diagonal k-mer: runs of blocks at one end)
  errors      none, or one substitution at read base 0, 1, 2, m - 3, m - 2 or m - 1 (the six rows around it, cut by the read's end)
"""
import numpy as np

from stress_batches import manual_batch

K = 6
LENS3 = (6, 7, 8, 9, 11, 63, 64, 65, 66, 127, 128, 129, 130, 150, 192)
LENS4 = (193, 250, 256)
CROSS = (9, 65, 129, 150, 250)          # lengths that get every placement x every error
HANG = (0, 1, 2, 3, 5, 49)
PAD = 120                                # haplotypes of 241 bases: two-byte match entries, twin lists
N_BARCODES = 30
ACGT = b"ACGT"


def read_specs():
    """(m, side, hang, sub): side 'L' / 'R', hang bases outside the window on that side, sub = read base to substitute or None."""
    assert sorted({(m - K) % 6 for m in LENS3}) == list(range(6))
    specs = []
    for m in LENS3 + LENS4:
        places = [("L", 0)] + [(s, h) for h in HANG[1:] for s in ("L", "R") if h < m]
        subs = [None, 0, 1, 2, m - 3, m - 2, m - 1]
        for pl in places:
            for sub in subs:
                if sub is not None and m not in CROSS and pl not in (("L", 0), ("L", 1), ("R", 1)):
                    continue
                specs.append((m, pl[0], pl[1], sub))
    return specs


def batches(seed=1506):
    """[(label, batch, n_barcodes)]: the specs in order, 32 to a batch (the last one filled up with the first specs again)."""
    rng = np.random.default_rng(seed)
    specs = read_specs()
    specs += specs[:(-len(specs)) % 32]
    out = []
    for b0 in range(0, len(specs), 32):
        haps, rds = [], []
        for l0 in range(b0, b0 + 32, 16):
            g = bytes(rng.choice(list(ACGT), 2 * PAD + 1 + 2 * 320).tolist())
            p = 320 + PAD
            ref = g[p - PAD:p + PAD + 1]
            alt = ref[:PAD] + bytes([ACGT[(ACGT.index(ref[PAD:PAD + 1]) + 1) % 4]]) + ref[PAD + 1:]
            haps.append((ref, alt))
            rl = []
            for i, (m, side, hang, sub) in enumerate(specs[l0:l0 + 16]):
                chrom = g[:p] + (alt[PAD:PAD + 1] if i & 1 else ref[PAD:PAD + 1]) + g[p + 1:]
                if hang == 0:
                    s = min(max(p - m // 2, p - PAD), p + PAD + 1 - m) if m <= 2 * PAD + 1 else p - PAD
                elif side == "L":
                    s = p - PAD - hang
                else:
                    s = p + PAD + 1 + hang - m
                rd = bytearray(chrom[s:s + m])
                assert len(rd) == m
                if sub is not None:
                    rd[sub] = ACGT[(ACGT.index(bytes(rd[sub:sub + 1])) + 1 + int(rng.integers(0, 3))) % 4]
                rl.append((i % N_BARCODES, 0, bytes(rd)))
            rds.append(rl)
        out.append(("reads %d - %d" % (b0, b0 + 31), manual_batch(haps, rds, N_BARCODES), N_BARCODES))
    return out
