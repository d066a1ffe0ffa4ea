"""Authored raw batches that make every rule of the raw-batch preparation (vartrix_amd/csrc/vtx_prep_core.h) DECIDE something, and the
ledger of what each must give.  A case names the rule it pins and the premise that makes it do so; tests/test_prep_core.py proves the
premises (pairs collide under the stated seed and not under the next, the wrap case wraps, a boundary case has its head where it
says) and runs the cases through the CPU harness, tests/test_gpu_prep_cases.py through vtx_submit_raw on the production library.

A record is R(barcode tag, UMI tag or None, what it must become): a cell index, NOT_BC (counted in num_not_cell_bc) or NON_UMI
(num_non_umi).  Tags are arbitrary bytes.  The tag arena is laid out so that equal tags are shared between records, a tag that occurs
inside the bytes already laid out overlaps them, and the last tag lies flush against the arena's end (nothing is appended behind it).
Every record has its own read (its read_off identifies it in the prepared batch); reads cover the SNV site of one haplotype pair as
REF, as ALT, or miss it, in turn, so that a read in the wrong cell or two molecules counted as one change the matrix.
"""
import random

import numpy as np

import prep_hash as ph
from vartrix_amd.abi import LOCUS_DTYPE, RAW_RECORD_DTYPE, TAG_MISSING, RawBatch

NOT_BC, NON_UMI = "not_cell_bc", "non_umi"
SEED0, SEED1 = ph.UMI_SEED0, ph.next_seed(ph.UMI_SEED0)
SHAPE_CAPS = (32, 64, 96, 128, 160, 192, 256, 512, 1024)      # kShapes of vtx_api.hip: rows per lane x lanes
BLOCK = 256


class R:
    def __init__(self, bc, umi, expect, read_len=32, **override):
        self.bc, self.umi, self.expect, self.read_len, self.override = bc, umi, expect, read_len, override


def _haplotypes(pad):
    rng = np.random.default_rng(20261021 + pad)
    flank = bytes(rng.choice(list(b"ACG"), 2 * pad).tolist())
    return flank[:pad] + b"T" + flank[pad:], flank[:pad] + b"A" + flank[pad:]


class Case:
    """One raw batch and its ledger entry.  loci: a list of record lists."""

    def __init__(self, name, group, rule, premise, barcodes, loci, use_umi=1, hash_rounds=1, pad=40, proofs=()):
        self.name, self.group, self.rule, self.premise = name, group, rule, premise
        self.barcodes, self.use_umi, self.hash_rounds, self.proofs = [bytes(b) for b in barcodes], use_umi, hash_rounds, list(proofs)
        self.specs = [r for recs in loci for r in recs]
        ref, alt = _haplotypes(pad)
        rng = random.Random(name)
        tags, reads, lo, rec = bytearray(), bytearray(), [], []

        def place(tag):
            at = bytes(tags).find(tag) if tag else len(tags)
            if at < 0:
                at = len(tags)
                tags.extend(tag)
            return at

        for li, recs in enumerate(loci):
            lo.append((li, len(rec), len(recs), 0, len(ref), len(ref), len(alt), 0))
            for r in recs:
                n, kind = r.read_len, len(rec) % 3
                if n <= 2 * pad and kind < 2:
                    bases = (ref, alt)[kind][pad - n // 2:pad - n // 2 + n]
                elif n <= pad:
                    bases = ref[:n]
                else:
                    bases = bytes(rng.choice(b"ACGT") for _ in range(n))
                row = {"read_off": len(reads), "read_len": n, "bc_off": place(r.bc), "bc_len": len(r.bc),
                       "umi_off": 0 if r.umi is None else place(r.umi), "umi_len": TAG_MISSING if r.umi is None else len(r.umi)}
                row.update(r.override)
                rec.append(tuple(row[k] for k in RAW_RECORD_DTYPE.names))
                reads += bases + b"A" * (n & 1)                     # every read starts at an even base (VTX_READS_NIBBLES)
        self.raw = RawBatch(np.array(lo, LOCUS_DTYPE).reshape(-1), np.array(rec, RAW_RECORD_DTYPE).reshape(-1),
                            np.frombuffer(ref + alt, np.uint8), np.frombuffer(bytes(reads), np.uint8), np.frombuffer(bytes(tags), np.uint8))
        self.not_cell_bc = sum(r.expect == NOT_BC for r in self.specs)
        self.non_umi = sum(r.expect == NON_UMI for r in self.specs)
        self.kept = len(self.specs) - self.not_cell_bc - self.non_umi

    @property
    def ledger(self):
        return {"rule": self.rule, "premise": self.premise, "num_not_cell_bc": self.not_cell_bc, "num_non_umi": self.non_umi,
                "kept": self.kept, "hash_rounds": self.hash_rounds}

    def expected_cells(self):
        """{read_off: cell} of the records that must be kept."""
        return {int(off): r.expect for off, r in zip(self.raw.records["read_off"], self.specs) if r.expect not in (NOT_BC, NON_UMI)}


CASES = []


def case(*a, **k):
    c = Case(*a, **k)
    assert c.name not in {x.name for x in CASES}, c.name
    CASES.append(c)
    return c


def _rand_bytes(seed, n):
    return random.Random(seed).randbytes(n)


U0, U1, U2 = b"UMI-AAAAAA", b"UMI-CCCCCC", b"\x00\xff\x80UMI"


# ================================================================ barcodes ================================================================
# a stem with NUL, bytes >= 0x80 and a repeated byte around the word edges; every listed barcode is a prefix of the longer ones
STEM = b"\x00ACG\xff\x80T\x00" + b"\x00GGA\xc3\xa9C\x7f" + b"TT\x00\x00\xfe-1\x01"
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 24)
assert len(STEM) == 24


def _flip(tag, i):
    return tag[:i] + bytes([tag[i] ^ 0x40]) + tag[i + 1:]


def _length_cases():
    bcs = [STEM[:n] for n in LENGTHS]
    recs = [R(b, U0, j) for j, b in enumerate(bcs)]
    for n in range(25):
        if n not in LENGTHS:                                       # a proper prefix of listed barcodes and a proper extension of others
            recs.append(R(STEM[:n], U0, NOT_BC))
    recs.append(R(STEM + b"\x00", U0, NOT_BC))
    recs.append(R(STEM[1:], U0, NOT_BC))
    for b in bcs:
        for i in (len(b) - 1, 7, 8):
            if 0 <= i < len(b):
                recs.append(R(_flip(b, i), U1, NOT_BC))
    recs += [R(b, U1, j) for j, b in enumerate(bcs)]               # the same tags again: shared bytes
    case("bc_lengths_and_neighbours", "barcode", "length compare + vtx_bytes_equal over every word of the tag",
         "listed: the prefixes of one 24-byte stem of 0, 1, 7, 8, 9, 15, 16, 17, 24 bytes; tags: every other prefix (a proper prefix of "
         "some listed barcodes, a proper extension of others), the stem plus one byte, and each listed barcode with its last byte, "
         "byte 7 or byte 8 changed", bcs, [recs[:20], recs[20:]])


_length_cases()

L16 = b"ACGTACGTACGTAC-1"
T16 = ph.collide_same_length(L16, b"TTTTGGGG")
case("bc_collision_same_length", "barcode", "vtx_bytes_equal decides when hash and length are equal",
     "the tag has the listed barcode's 64-bit hash (seed 0) and its length, other bytes in both words", [L16, b"GGGGACGTACGTAC-1"],
     [[R(L16, U0, 0), R(T16, U0, NOT_BC), R(T16, U1, NOT_BC), R(L16, U1, 0)]],
     proofs=[lambda env: env.collide(L16, T16, 0)])

L24 = b"ACGTACGTTTGACCAGTACGTA-1"
T24 = ph.collide_same_length(L24, b"\x00\x01\x02\x03\xfc\xfd\xfe\xff")
case("bc_collision_same_first_word", "barcode", "vtx_bytes_equal looks beyond the first word",
     "24 bytes: the tag has the listed barcode's hash, length and FIRST WORD; words two and three differ", [L24],
     [[R(T24, U0, NOT_BC), R(L24, U0, 0)]],
     proofs=[lambda env: env.collide(L24, T24, 0), lambda env: env.check(L24[:8] == T24[:8] and L24[8:16] != T24[8:16])])

L16B = ph.collide_same_length(L16, b"CCCCAAAA")
T16B = ph.collide_same_length(L16, b"\x80\x00\x00\x00\x00\x00\x00\x80")
case("bc_two_listed_collide", "barcode", "the probe walks on past an equal hash with other bytes",
     "barcodes 0 and 2 have one 64-bit hash, hence one home slot: the second sits behind the first; a third tag with that hash is not "
     "listed", [L16, b"GGGGACGTACGTAC-1", L16B],
     [[R(L16B, U0, 2), R(L16, U0, 0), R(T16B, U0, NOT_BC), R(L16B, U1, 2)], [R(T16B, U0, NOT_BC), R(L16B, U0, 2)]],
     proofs=[lambda env: env.collide(L16, L16B, 0), lambda env: env.collide(L16, T16B, 0), lambda env: env.check(T16B != L16B)])

S7, S5 = b"ACGTACG", b"TTG\x00A"
X8, Y8 = ph.collide_cross_length(S7), ph.collide_cross_length(S5)
case("bc_collision_cross_length", "barcode", "the length compare decides when the hashes are equal",
     "a 7-byte barcode and an 8-byte tag with one hash; an 8-byte barcode and a 5-byte tag with one hash", [S7, Y8],
     [[R(S7, U0, 0), R(X8, U0, NOT_BC), R(Y8, U0, 1), R(S5, U0, NOT_BC)]],
     proofs=[lambda env: env.collide(S7, X8, 0), lambda env: env.collide(S5, Y8, 0), lambda env: env.check(X8 == b"@CGTACG\x00")])

# the wrap: slots 14 and 15 of the 16 taken, then two more barcodes whose home is 15 and 14
_W = []
for _slot, _pre in ((14, b"w14a"), (15, b"w15a"), (15, b"w15b"), (14, b"w14b")):
    _W.append(ph.tag_with_home(_slot, 16, _pre, 12, _W))
W_MISS = ph.tag_with_home(15, 16, b"miss", 12, _W)
W_MISS14 = ph.tag_with_home(14, 16, b"m14-", 12, _W)
case("bc_probe_wraps", "barcode", "the probe goes from the table's last slot to slot 0",
     "16 slots; barcodes with home slots 14, 15, 15, 14 lie in slots 14, 15, 0, 1: barcode 2 is found behind the wrap, barcode 3 two "
     "slots behind it; unlisted tags with home 15 and 14 cross the wrap to the empty slot 2", _W,
     [[R(_W[2], U0, 2), R(_W[3], U0, 3), R(W_MISS, U0, NOT_BC), R(_W[0], U0, 0), R(_W[1], U0, 1), R(W_MISS14, U0, NOT_BC)]],
     proofs=[lambda env: env.check(env.slots(_W)[14:] == [1, 2] and env.slots(_W)[:3] == [3, 4, 0]),
             lambda env: env.check(ph.probe_path(env.slots(_W), _W, _W[2]) == ([15, 0], 2)),
             lambda env: env.check(ph.probe_path(env.slots(_W), _W, _W[3]) == ([14, 15, 0, 1], 3)),
             lambda env: env.check(ph.probe_path(env.slots(_W), _W, W_MISS) == ([15, 0, 1, 2], None)),
             lambda env: env.check(ph.probe_path(env.slots(_W), _W, W_MISS14) == ([14, 15, 0, 1, 2], None))])

DA, DB, DC = b"DUP-AAAA-1", b"DUP-BBBB-1", b"DUP-CCCC-1"
case("bc_duplicates_first_index", "barcode", "a repeated list entry keeps its first index", "list A B A C B: A is 0, B is 1, C is 3",
     [DA, DB, DA, DC, DB], [[R(DB, U0, 1), R(DA, U0, 0), R(DC, U0, 3), R(DA, U1, 0), R(DB, U1, 1), R(b"DUP-DDDD-1", U0, NOT_BC)]])

LIST9 = [b"BC%02d-\x00\xff-1" % j for j in range(9)]
for _n, _slots in ((0, 16), (1, 16), (8, 16), (9, 32)):
    _recs = [R(LIST9[j], U0, j if j < _n else NOT_BC) for j in (8, 0, 7, 1, 4)] + [R(b"", U0, NOT_BC), R(LIST9[0], None, NON_UMI if _n else NOT_BC)]
    case("bc_list_of_%d" % _n, "barcode", "table size: at least 16 slots, load <= 1/2",
         "%d barcodes: %d slots" % (_n, _slots), LIST9[:_n], [_recs[:3], _recs[3:]],
         proofs=[lambda env, n=_n, s=_slots: env.check(len(env.slots(LIST9[:n])) == s == ph.table_capacity(n))])

# ================================================================ order of the tests ================================================================
C = [b"CELL-%d-\x00\x80" % j for j in range(4)]
case("order_barcode_test_first", "order", "the barcode test comes first: a record counts once",
     "an unlisted barcode without UB is num_not_cell_bc, a listed one without UB num_non_umi", C,
     [[R(b"CELL-9-\x00\x80", None, NOT_BC), R(C[1], None, NON_UMI), R(C[1], U0, 1), R(b"CELL-9-\x00\x80", U0, NOT_BC), R(b"", None, NOT_BC)]])
case("order_no_umi_mode", "order", "without --umi the UB tag is not looked at",
     "use_umi = 0: a missing UB is kept; a umi_off far outside the arena is ignored", C,
     [[R(C[2], None, 2), R(C[0], U0, 0, umi_off=0xfffffff0, umi_len=64), R(C[0], U1, 0), R(b"nope", None, NOT_BC), R(C[3], U0, 3, umi_off=0xffffffff, umi_len=0xfffe)]],
     use_umi=0)

# ================================================================ UMIs ================================================================
case("umi_empty_vs_missing", "umi", "an empty UB is a UMI; a missing one is not", "length 0 present (twice: one molecule) and TAG_MISSING", C,
     [[R(C[0], b"", 0), R(C[0], None, NON_UMI), R(C[0], b"", 0), R(C[0], b"\x00", 0), R(C[1], None, NON_UMI)]])
case("umi_trailing_nul", "umi", "the length is part of a UMI", "A and A NUL in one cell: zero-extended words are equal, the lengths (and hashes) are not", C,
     [[R(C[0], b"A", 0), R(C[0], b"A\x00", 0), R(C[0], b"A", 0), R(C[0], b"A\x00\x00", 0), R(C[0], b"A\x00", 0)]])
for _n in (7, 8, 9, 16, 17):
    _u = _rand_bytes("umi%d" % _n, _n)
    _v = _u[:-1] + bytes([_u[-1] ^ 1])
    case("umi_last_byte_%d" % _n, "umi", "UMIs are compared to their last byte",
         "two UMIs of %d bytes that differ in the last byte only, alone in one cell (with every hash forced equal the byte compare is "
         "all that separates them: the CPU harness and the dev library run this case that way too)" % _n, C,
         [[R(C[1], _u, 1), R(C[1], _v, 1), R(C[1], _u, 1), R(C[1], _v, 1)]])
case("umi_same_bytes_other_group", "umi", "UMI groups live inside one (locus, cell)", "one UMI in two cells of a locus and in two loci", C,
     [[R(C[0], U0, 0), R(C[1], U0, 1), R(C[0], U0, 0)], [R(C[0], U0, 0), R(C[1], U0, 1)]])
case("umi_interleaved", "umi", "the UMI sort brings a molecule's reads together", "A B A B A in one cell", C,
     [[R(C[2], U0, 2), R(C[2], U1, 2), R(C[2], U0, 2), R(C[2], U1, 2), R(C[2], U0, 2)]])
UA = b"\x00MOLECULE-ONE\xff\x00\x80"
UB = ph.collide_same_length(UA, b"molecule", SEED0)
case("umi_collide_one_cell", "umi", "equal UMI hashes with other bytes raise the collision flag: the next seed is taken",
     "two 16-byte UMIs of one cell with one hash under the first seed and two under the second", C,
     [[R(C[0], UA, 0), R(C[0], UB, 0), R(C[0], UA, 0), R(C[1], UB, 1)]], hash_rounds=2,
     proofs=[lambda env: env.collide(UA, UB, SEED0), lambda env: env.check(env.hash(UA, SEED1) != env.hash(UB, SEED1))])
case("umi_collide_two_cells", "umi", "a collision across cells is none", "the same pair, one UMI per cell", C,
     [[R(C[0], UA, 0), R(C[1], UB, 1), R(C[0], UA, 0), R(C[1], UB, 1)], [R(C[0], UB, 0), R(C[1], UA, 1)]],
     proofs=[lambda env: env.collide(UA, UB, SEED0)])
UC = b"seven\x00\x80"
UD = ph.collide_cross_length(UC, SEED0)
case("umi_collide_cross_length", "umi", "the UMI head compares lengths before bytes",
     "a 7-byte and an 8-byte UMI of one cell with one hash under the first seed and two under the second", C,
     [[R(C[3], UC, 3), R(C[3], UD, 3), R(C[3], UD, 3), R(C[3], UC, 3)]], hash_rounds=2,
     proofs=[lambda env: env.collide(UC, UD, SEED0), lambda env: env.check(env.hash(UC, SEED1) != env.hash(UD, SEED1))])

# ================================================================ key widths ================================================================
WIDTH_BARCODES = (1, 2, 3, 4, 5, 8, 9)
WIDTH_LOCI = (1, 2, 3, 4, 5, 7, 8, 9)
for _nb in WIDTH_BARCODES:
    for _nl in WIDTH_LOCI:
        for _v in range(4):
            _bcs, _loci = LIST9[:_nb], []
            for _l in range(_nl):
                _recs = [R(_bcs[_l % _nb], U0, _l % _nb), R(_bcs[(_l + 1) % _nb], U1, (_l + 1) % _nb)]
                if _v & 2 and _l in (0, _nl // 2):
                    _recs.insert(1, R(b"unlisted", U0, NOT_BC))
                if _l == _nl - 1:
                    if _v & 2:
                        _recs.append(R(_bcs[0], None, NON_UMI))
                    if _v & 1:
                        _recs += [R(_bcs[-1], U0, _nb - 1), R(_bcs[-1], U2, _nb - 1)]
                    if _v & 2:
                        _recs += [R(LIST9[8] + b"x", U0, NOT_BC), R(_bcs[-1], None, NON_UMI)]
                    if _v & 1:
                        _recs.append(R(_bcs[-1], U0, _nb - 1))
                _loci.append(_recs)
            case("width_b%d_l%d_v%d" % (_nb, _nl, _v), "width", "cell_bits, end_bit and the dropped key",
                 "%d barcodes, %d loci: %s%s" % (_nb, _nl, "records of the last locus in the last cell; " if _v & 1 else "",
                                                 "dropped records in the first, a middle and the last locus" if _v & 2 else "no dropped record"),
                 _bcs, _loci)
for _where, _full in (("front", (3, 4)), ("middle", (0, 4)), ("end", (0, 1)), ("all_but_one", (2,))):
    _loci = []
    for _l in range(5):
        if _l in _full:
            _loci.append([R(C[3], U0, 3), R(C[0], U1, 0), R(b"?", U0, NOT_BC), R(C[3], U0, 3)])
        else:
            _loci.append([R(b"?", U0, NOT_BC), R(C[1], None, NON_UMI)] if _l & 1 else [])
    case("loci_empty_" + _where, "width", "locus ranges of loci without kept records",
         "5 loci, kept records in %s only: the others have no record or dropped records only" % (_full,), C, _loci)

# ================================================================ boundaries ================================================================
POOL = sorted((b"P%03d\x00\xffumi" % k for k in range(300)), key=lambda u: ph.hash_bytes(u, SEED0))    # ascending hash under the first seed


def _interleave(kept, seed):
    """kept records in a shuffled order with a dropped record behind every fourth: kept and raw indices differ"""
    rng = random.Random(seed)
    kept = list(kept)
    rng.shuffle(kept)
    out = []
    for k, r in enumerate(kept):
        out.append(r)
        if k % 4 == 3:
            out.append(R(b"not-a-cell", U0, NOT_BC) if k & 4 else R(C[k % 4], None, NON_UMI))
    return out


def _block(n, cells, n_umis, first_umi=0):
    return [R(C[cells[k % len(cells)]], POOL[first_umi + (k // len(cells)) % n_umis], cells[k % len(cells)]) for k in range(n)]


for _at in (256, 512):
    case("boundary_locus_at_%d" % _at, "boundary", "a locus run's first record reads its predecessor across a workgroup edge",
         "locus 0 has %d kept records: locus 1 begins at kept record %d" % (_at, _at), C,
         [_interleave(_block(_at, (0, 1, 2), 40), _at), _interleave(_block(6, (0, 2), 2), 1)],
         proofs=[lambda env, at=_at: env.check(list(env.prepared("boundary_locus_at_%d" % at)[1]) == [0, at])])
    case("boundary_cell_at_%d" % _at, "boundary", "a cell group's head reads its predecessor across a workgroup edge",
         "cell 0 has %d kept records in locus 0: cell 2 begins at kept record %d with the UMI cell 0 ends with" % (_at, _at), C,
         [_interleave(_block(_at, (0,), 1) + _block(3, (2,), 1), _at + 1), [R(C[1], U0, 1)]],
         proofs=[lambda env, at=_at: env.check([int(x) for x in env.prepared("boundary_cell_at_%d" % at)[0]["cell_index"][at - 1:at + 2]] == [0, 2, 2])])
    case("boundary_umi_at_%d" % _at, "boundary", "a UMI head reads its predecessor across a workgroup edge",
         "one cell: the %d UMIs with the smallest hashes under the first seed, two reads each, then the next UMI with three reads, "
         "which begins at kept record %d" % (_at // 2, _at), C,
         [_interleave(_block(_at, (1,), _at // 2)[:_at // 2] * 2 + _block(3, (1,), 1, _at // 2), _at + 2)],
         proofs=[lambda env, at=_at: env.check((lambda u: u[at - 2] == u[at - 1] != u[at] == u[at + 1] == u[at + 2] and len(set(u)) == at // 2 + 1)(
             [int(x) for x in env.prepared("boundary_umi_at_%d" % at)[0]["umi_id"]]))])
for _n in (255, 256, 257, 511, 512, 513):
    case("n_kept_%d" % _n, "boundary", "the last workgroup's size, groups that span a workgroup edge",
         "%d kept records in 3 loci, 4 cells, 5 UMIs per cell, dropped records interleaved" % _n, C,
         [_interleave([R(C[(k * 7) % 4], POOL[(k * 13) % 5], (k * 7) % 4) for k in range(_l * _n // 3, (_l + 1) * _n // 3)], _n + _l) for _l in range(3)])
case("group_spans_256", "boundary", "record 256 is a head only if its key differs from record 255's",
     "300 kept reads of ONE molecule: the only head is record 0, the locus has one range", C, [_interleave(_block(300, (2,), 1), 300)])
case("shape_caps", "boundary", "every kernel shape's cap and one above, in one batch",
     "reads of 32, 64, 96, 128, 160, 192, 256, 512, 1024 bases and one more each (1025: the slow list)", C,
     [[R(C[k % 4], POOL[k % 3], k % 4, read_len=n) for k, n in enumerate(x for cap in SHAPE_CAPS for x in (cap, cap + 1))]], pad=600)

LEDGER = {c.name: c.ledger for c in CASES}
BY_NAME = {c.name: c for c in CASES}
# the cases that are also run with every UMI hash forced equal in the first round (harness: weak_rounds = 1; dev library:
# VTX_PREP_WEAK_ROUNDS=1): the byte compare alone separates the molecules, and two rounds are needed
WEAK_ROUND_CASES = tuple("umi_last_byte_%d" % n for n in (7, 8, 9, 16, 17)) + ("umi_trailing_nul", "umi_interleaved")


# ---- forged tables: the probe over arrays whose HASHES are set by hand, so that the length compare meets what no real list gives it ----
def forged_probe_cases():
    """[(name, entries [(bytes, forged hash or None)], tag, want index or None)]: entry j lies in the slot its (forged) hash says,
    and the entries' bytes lie one behind the other."""
    tag = b"ACGTACGTAC-1"
    h = ph.hash_bytes(tag)
    return [
        ("forged_prefix", [(tag[:-1], h), (b"1\x00", None)], tag, None),       # a listed proper prefix with the tag's hash; the byte behind it is the tag's last
        ("forged_prefix_then_tag", [(tag[:-1], h), (tag, None)], tag, 1),
        ("forged_extension", [(tag + b"-", h)], tag, None),
        ("forged_extension_then_tag", [(tag + b"-", h), (tag, None)], tag, 1),
        ("forged_empty", [(b"", h), (tag, None)], tag, 1),
        ("forged_same_length_other_bytes", [(tag[:-1] + b"2", h), (tag, None)], tag, 1),
    ]
