"""An independent model of how one BAM record is read — CIGAR, end position, aux block, bases — for tests/test_scan_core.py,
tests/test_bam_grammar.py and tests/test_gpu_bam_grammar.py.

The repository holds the parsing rules in several near-identical C copies (vartrix_amd/csrc/vtx_scan_core.h, host/vtx_host.cpp,
oracle/vtx_oracle.c) plus oracle/refpipe.py; they share one structure — a two-phase walk with running positions — so agreement
among them proves little.  This file is written differently on purpose:

  * a CIGAR is first turned into a table of op rows with prefix sums; a probe is answered by looking for the first row that decides
    it (no running state);
  * for CIGARs that are valid under the SAM spec the answer is also derived from a coverage set, and the two must agree;
  * irregular CIGARs have a hand-written table (IRREGULAR), each row naming the match arm of rust-htslib 0.36
    CigarStringView::read_pos (as called at src/main.rs:796: include_softclips = false, include_dels = true) that decides it;
  * the aux block is tokenised as a whole before any tag is looked up;
  * bases come from a literal 16-entry table.
"""
import itertools
import struct

OPS = "MIDNSHP=X"
REF_OPS = frozenset("MDN=X")          # consume reference (SAM spec 1.4.6)
QUERY_OPS = frozenset("MIS=X")        # consume query
COVER_OPS = frozenset("M=XD")         # a probe under one of these is Some (include_dels = true)

SOME, NONE, ERR = 1, 0, -1

NT16 = ("=", "A", "C", "M", "G", "R", "S", "V", "T", "W", "Y", "H", "K", "D", "B", "N")    # SAM spec 4.2.3, code 0 .. 15


def parse(text):
    """"5H3S10M" -> [("H", 5), ("S", 3), ("M", 10)]"""
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append((ch, int(num)))
            num = ""
    assert not num
    return out


def encode(cigar):
    """BAM's uint32 per op: len << 4 | code"""
    return [(n << 4) | OPS.index(op) for op, n in cigar]


def text(cigar):
    return "".join("%d%s" % (n, op) for op, n in cigar) or "*"


def is_valid(cigar):
    """SAM spec 1.4.6: H only outermost, S only next to H or at the ends; plus the crate's own demand: no D / N before the first
    query-consuming op.  (A CIGAR with no query-consuming op at all is not valid here.)"""
    ops = [op for op, _ in cigar]
    core = ops[:]
    if core and core[0] == "H":          # "H can only be present as the first and/or last operation": one at each end
        core.pop(0)
    if core and core[-1] == "H":
        core.pop()
    if "H" in core:
        return False
    inner = core[:]
    while inner and inner[0] == "S":
        inner.pop(0)
    while inner and inner[-1] == "S":
        inner.pop()
    if "S" in inner:
        return False
    first_q = next((i for i, op in enumerate(ops) if op in QUERY_OPS), None)
    if first_q is None:
        return False
    return not any(op in "DN" for op in ops[:first_q])


def covered(cigar, pos):
    """The reference positions under M, =, X or D, as a list of half-open ranges (a set would not hold a 2^28 op)."""
    out, at = [], pos
    for op, n in cigar:
        if op in COVER_OPS and n:
            out.append((at, at + n))
        if op in REF_OPS:
            at += n
    return out


def in_ranges(ranges, p):
    return any(a <= p < b for a, b in ranges)


def endpos(cigar, pos, flag=0):
    """htslib bam_endpos: pos + max(1, positions under M D N = X); pos + 1 for an unmapped record (flag 0x4) whatever its CIGAR."""
    if flag & 0x4:
        return pos + 1
    return pos + max(1, sum(n for op, n in cigar if op in REF_OPS))


def read_pos(cigar, pos, ref_pos):
    """-> (SOME, query position) | (NONE, None) | (ERR, None): what read_pos(ref_pos, false, true) answers.

    Rows, not a walk.  The head of the CIGAR is its leading run of H / P.  The head decides when (a) it holds an H that is neither
    first nor last: Err; (b) it is the whole CIGAR: None; (c) the op behind it is D or N: Err.  Otherwise every op from there on
    gets its reference start and query start as prefix sums; the rows whose reference start is <= ref_pos are "in reach" (the
    start never decreases, so they are a prefix), and the first row in reach that is decisive decides: M = X D holding ref_pos ->
    Some; H -> Err unless it is the CIGAR's last op, then None.  No decisive row in reach: None."""
    n = len(cigar)
    head = len(list(itertools.takewhile(lambda t: t[0] in "HP", cigar)))
    if any(cigar[i][0] == "H" and 0 < i < n - 1 for i in range(head)):
        return ERR, None
    if head == n:
        return NONE, None
    if cigar[head][0] in "DN":
        return ERR, None
    body = cigar[head:]
    r_start = [pos + s for s in itertools.accumulate([0] + [l if op in REF_OPS else 0 for op, l in body])][:-1]
    q_start = list(itertools.accumulate([0] + [l if op in QUERY_OPS else 0 for op, l in body]))[:-1]
    for k, (op, l) in enumerate(body):
        if r_start[k] > ref_pos:
            break
        if op in COVER_OPS and r_start[k] <= ref_pos < r_start[k] + l:
            return SOME, q_start[k] + (ref_pos - r_start[k] if op != "D" else 0)
        if op == "H":
            return (ERR, None) if head + k < n - 1 else (NONE, None)
    return NONE, None


def read_pos_valid(cigar, pos, ref_pos):
    """The same answer for a VALID CIGAR, from the coverage set alone: Some exactly on covered positions, never Err."""
    assert is_valid(cigar)
    return SOME if in_ranges(covered(cigar, pos), ref_pos) else NONE


def useful(cigar, pos, start, end):
    """useful_alignment (src/main.rs:790-806): probes start..=end in order; the first answer that is not None decides (Some: useful;
    Err: the read is dropped, :799-802)."""
    for p in range(start, end + 1):
        r = read_pos(cigar, pos, p)[0]
        if r != NONE:
            return r == SOME
    return False


def useful_valid(cigar, pos, start, end):
    """For a valid CIGAR: [start, end] (inclusive) meets the coverage set."""
    assert is_valid(cigar)
    return any(a <= end and b > start for a, b in covered(cigar, pos))


def phases(cigar, pos, ref_pos):
    """Which ops the model's two stages look at for this probe: (ops of the head that are inspected, ops of the body in reach up to
    the deciding one).  For the coverage conditions of the enumeration."""
    n = len(cigar)
    head = len(list(itertools.takewhile(lambda t: t[0] in "HP", cigar)))
    seen_head = []
    for i in range(min(head + 1, n)):
        seen_head.append(cigar[i][0])
        if cigar[i][0] == "H" and 0 < i < n - 1:
            return seen_head, []
    if head == n or cigar[head][0] in "DN":
        return seen_head, []
    at, seen_body = pos, []
    for k in range(head, n):
        op, l = cigar[k]
        if at > ref_pos:
            break
        seen_body.append(op)
        if (op in COVER_OPS and at <= ref_pos < at + l) or op == "H":
            break
        if op in REF_OPS:
            at += l
    return seen_head, seen_body


# Irregular CIGARs: (text, pos, {probe: expected}, the rust-htslib read_pos arm that decides).  Written by hand from the match arms;
# "first loop" is the search for the first op that refers to query position 0, "walk" the `while rpos <= ref_pos && j < len` loop.
IRREGULAR = [
    # first loop, arm `Cigar::Del(_) => Err(.. "'deletion' (D) found before any operation describing read sequence")`
    ("2D5M", 100, {98: ERR, 100: ERR, 103: ERR, 110: ERR}, "first loop: Del -> Err, whatever the probe"),
    # first loop, arm `Cigar::RefSkip(_) => Err(.. "'reference skip' (N) found before any operation describing read sequence")`
    ("2N5M", 100, {99: ERR, 100: ERR, 104: ERR}, "first loop: RefSkip -> Err"),
    # walk, arm `Cigar::HardClip(_) if j < self.len() - 1 => Err(.. "'hard clip' (H) found in between operations")`: rpos after 5M is
    # 105, so probes >= 105 reach the H; probes inside the 5M return Some before it
    ("5M2H5M", 100, {99: NONE, 100: SOME, 104: SOME, 105: ERR, 107: ERR, 200: ERR}, "walk: HardClip in the middle, reached -> Err"),
    # the same H is NOT reached when `rpos > ref_pos` ends the loop first: 5M3D2H5M, probe 104 is Some in the M, 106 Some in the D;
    # and in 1I5M2H3M a probe before pos never enters the loop
    ("5M3D2H5M", 100, {104: SOME, 106: SOME, 107: SOME, 108: ERR, 99: NONE}, "walk: loop condition rpos <= ref_pos comes before the H"),
    ("1I5M2H3M", 100, {99: NONE, 98: NONE, 102: SOME, 105: ERR}, "walk: a probe below pos never enters the loop, the H is not seen"),
    # first loop, arm `Cigar::Pad(_) | Cigar::HardClip(_) if i == self.len() - 1 => Ok(None)`
    ("3H", 100, {99: NONE, 100: NONE, 101: NONE}, "first loop: only hard clips -> Ok(None)"),
    ("2P", 100, {100: NONE, 101: NONE}, "first loop: only pads -> Ok(None)"),
    ("3H2P", 100, {100: NONE}, "first loop: H then P last -> Ok(None)"),
    ("2P3H", 100, {100: NONE}, "first loop: P then H last (i == len - 1, not 'in between') -> Ok(None)"),
    # first loop, arm `Cigar::HardClip(_) if i > 0 && i < self.len() - 1 => Err(..)`: the middle H of three
    ("1H1H1H", 100, {99: ERR, 100: ERR}, "first loop: H with i > 0 && i < len - 1 -> Err"),
    ("2P3H5M", 100, {100: ERR, 102: ERR}, "first loop: H behind a leading pad is 'in between' -> Err"),
    # walk, arm `Cigar::HardClip(_) => Ok(None)` (the last op)
    ("5M3H", 100, {100: SOME, 104: SOME, 105: NONE, 106: NONE, 1000: NONE}, "walk: HardClip last -> Ok(None)"),
    ("5M2S3H", 100, {104: SOME, 105: NONE, 107: NONE}, "walk: SoftClip (no softclips included) then HardClip last -> Ok(None)"),
    # first loop: leading H is skipped (`Pad | HardClip => ()`), SoftClip sets j; walk: SoftClip arm advances j only
    ("5H3S10M", 100, {97: NONE, 99: NONE, 100: SOME, 109: SOME, 110: NONE}, "first loop: H skipped, S breaks; S consumes no reference"),
    # no ops: neither loop runs
    ("", 100, {99: NONE, 100: NONE, 101: NONE}, "empty CIGAR: Ok(None) at the function's end"),
    # walk, arm `Match(l) if contains_ref_pos(rpos, l)`: l = 0 holds nothing, the plain Match arm moves on (rpos += 0, j += 1)
    ("0M5M", 100, {100: SOME, 104: SOME, 105: NONE}, "walk: zero-length M contains nothing, next op decides"),
    ("0M", 100, {100: NONE}, "walk: zero-length M alone -> Ok(None)"),
    ("3M0D3M", 100, {103: SOME, 105: SOME, 106: NONE}, "walk: zero-length D contains nothing"),
    # first loop, arm `Match | Diff | Equal | Ins => { j = i; break }`; walk, arm `Ins(l) => { qpos += l; j += 1 }`
    ("3I5M", 100, {99: NONE, 100: SOME, 104: SOME, 105: NONE}, "first loop: Ins breaks; it consumes no reference"),
    ("3I", 100, {100: NONE}, "walk: Ins alone -> Ok(None)"),
    # first loop: a leading P is skipped; the D behind it is still 'before any operation describing read sequence'
    ("2P5M", 100, {100: SOME, 104: SOME, 105: NONE}, "first loop: leading Pad skipped"),
    ("2P3D5M", 100, {100: ERR, 104: ERR}, "first loop: Pad skipped, then Del -> Err"),
    # walk: Pad in the middle, RefSkip, Equal and Diff
    ("3=2P2X4N3M", 100, {102: SOME, 103: SOME, 104: SOME, 105: NONE, 108: NONE, 109: SOME, 111: SOME, 112: NONE}, "walk: = and X like M, P skipped, N never Some"),
    # trailing S then H
    ("4M2S1H", 100, {103: SOME, 104: NONE}, "walk: S then the last H -> Ok(None)"),
]

# the query positions for the rows above where the answer is Some and the arithmetic is worth pinning: qpos counts M = X I S
IRREGULAR_QPOS = [
    ("5H3S10M", 100, 100, 3), ("5H3S10M", 100, 109, 12), ("3I5M", 100, 100, 3), ("5M3D2H5M", 100, 106, 5), ("3=2P2X4N3M", 100, 109, 5),
    ("0M5M", 100, 104, 4), ("2P5M", 100, 102, 2),
]


# ---------------------------------------------------------------------------------------------------------------------------
# aux
# ---------------------------------------------------------------------------------------------------------------------------
_FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}
_B_ELEM = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def tokenise(aux):
    """The whole aux block -> ([(tag, type, value bytes)], well_formed).  SAM spec 4.2.4.  Tokens in front of a malformed spot are
    kept; nothing behind it is looked at.  Malformed: an unknown type, a value that runs past the block, a Z / H without its NUL,
    fewer than three bytes left over."""
    toks, o, n = [], 0, len(aux)
    while o < n:
        if o + 3 > n:
            return toks, False
        tag, ty = bytes(aux[o:o + 2]), chr(aux[o + 2])
        o += 3
        if ty in _FIXED:
            e = o + _FIXED[ty]
        elif ty in "ZH":
            z = aux.find(b"\x00", o)
            if z < 0:
                return toks, False
            toks.append((tag, ty, bytes(aux[o:z])))
            o = z + 1
            continue
        elif ty == "B":
            if o + 5 > n or chr(aux[o]) not in _B_ELEM:
                return toks, False
            e = o + 5 + struct.unpack_from("<I", aux, o + 1)[0] * _B_ELEM[chr(aux[o])]
        else:
            return toks, False
        if e > n:
            return toks, False
        toks.append((tag, ty, bytes(aux[o:e])))
        o = e
    return toks, True


def aux_lookup(aux, tag):
    """rec.aux(tag) matched against Aux::String (src/main.rs:742-748, :753-755): the tag's FIRST occurrence decides, and only a Z
    value is a string.  None: missing.  A malformed block answers for the tokens in front of the malformed spot only (htslib's
    bam_aux_get gives NULL on corrupt aux data: missing)."""
    toks, _ = tokenise(aux)
    for t, ty, val in toks:
        if t == tag:
            return val if ty == "Z" else None
    return None


def decode_bases(packed, l_seq):
    return "".join(NT16[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))


# ---------------------------------------------------------------------------------------------------------------------------
# one record's fate at one locus: the filters of evaluate_alns in their order (src/main.rs:831-895)
# ---------------------------------------------------------------------------------------------------------------------------
def pair_outcome(case, start, end, barcodes, mapq=0, primary_only=False, no_duplicates=False, use_umi=False, bam_tag=b"CB"):
    """case: dict(pos, cigar (parsed), flag, mapq, aux bytes).  -> None when bam.fetch does not return the record for [start, end),
    else "kept" or the Metrics counter the pair lands in."""
    e = endpos(case["cigar"], case["pos"], case["flag"])
    if not (case["pos"] < end and e > start):
        return None
    if case["mapq"] < mapq:
        return "num_low_mapq"
    if primary_only and case["flag"] & 0x900:
        return "num_non_primary"
    if no_duplicates and case["flag"] & 0x400:
        return "num_duplicates"
    if not useful(case["cigar"], case["pos"], start, end):
        return "num_not_useful"
    cb = aux_lookup(case["aux"], bam_tag)
    if cb is None or cb not in barcodes:
        return "num_not_cell_bc"
    if use_umi and aux_lookup(case["aux"], b"UB") is None:
        return "num_non_umi"
    return "kept"


# ---------------------------------------------------------------------------------------------------------------------------
# grammar BAMs: every record is one case, over tests/golden/test_dna.fa / test_dna.vcf
# ---------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("ops", "endpos", "aux", "bases", "layout")

_OPS_CASES = ["60M", "60=", "25=3X32=", "10H50M", "50M10H", "5H3S50M", "3I50M", "50M3I", "2D50M", "2N50M", "25M2H25M", "25M3D2H25M", "3H", "2P",
              "3H2P", "2P3H", "1H1H1H", "*", "0M50M", "25M0D25M", "0M", "2P50M", "2P3D50M", "20=2P5X40N20M", "50M2S1H", "30M300N30M", "3S50M4S",
              "1I25M2H3M", "25M6D25M", "25M0I25M", "0H50M0H", "50M0P", "2P3H5M", "5M3H", "0S0M50M", "30X", "20M5P20M", "0D50M", "0N50M", "4H"]
_ENDPOS_CASES = ["60M", "5I", "10S", "*", "3H", "2P", "50N", "5S5I", "0M", "3I4S", "40M20N", "0M0D0N"]
_IUPAC = "=ACMGRSVTWYHKDBN"


def _flags_for(i):
    return (0x400 if i % 7 == 3 else 0) | (0x100 if i % 7 == 5 else 0) | (0x800 if i % 11 == 6 else 0), (20 if i % 5 == 0 else 60)


def family_cases(family, fasta, vcf, barcodes):
    """(A UB value of 65 535 bytes or more is not among the cases: tag lengths travel as 16 bits with 0xffff for "missing", so the
    packer and the device count such a read as one without a UMI where the reference would keep it.  That limit has its own test,
    tests/test_bam_grammar.py::test_umi_of_65535_bytes_is_beyond_the_tag_length_format.)

    -> list of dict(name, tid, pos, cigar (parsed), flag, mapq, seq, qname, aux): one BAM record each, every one with its own
    l_seq (a differing raw record names its case by read_len).  fasta: the contig's bytes (upper case); vcf: refpipe.read_vcf's
    records; barcodes: the listed barcodes (bytes)."""
    from oracle import bamwriter
    loci = [v.pos for v in vcf]
    cases = []

    def add(name, pos, cigar, flag=0, mapq=60, seq=None, qname=None, aux=None, tid=0, l_seq=None):
        k = len(cases)
        n = 20 + k if l_seq is None else l_seq
        if seq is None:
            seq = fasta[max(pos, 0):max(pos, 0) + n].decode()
        if aux is None:
            aux = bamwriter.aux_bytes([("CB", "Z", barcodes[k % 40]), ("UB", "Z", "UMI%02d" % (k % 9)), ("NM", "i", 0)])
        cases.append(dict(name="%s/%s" % (family, name), tid=tid, pos=pos, cigar=parse("" if cigar == "*" else cigar), flag=flag, mapq=mapq,
                          seq=seq, qname=("c%03d" % k) if qname is None else qname, aux=aux))

    if family == "ops":
        for i, cg in enumerate(_OPS_CASES):
            at = loci[(3 * i) % len(loci)]
            for d in (0, 27, 70):                      # starts at the locus, straddles it, lies in front of it (or reaches it through an N)
                flag, mapq = _flags_for(len(cases))
                add("%s@-%d" % (cg, d), at - d, cg, flag, mapq)
        add("61987 and 61989 both", 61960, "60M")       # several loci under one read
        add("49514 and 49515 through a deletion", 49500, "14M3D40M")
        add("66487 and 66521 through =/X", 66470, "30=2X40=")
    elif family == "endpos":
        for i, cg in enumerate(_ENDPOS_CASES):
            at = loci[(5 * i + 1) % len(loci)]
            for d in (0, 1, 10):
                for unmapped in (0, 4):
                    flag, mapq = _flags_for(len(cases))
                    add("%s@-%d flag %#x" % (cg, d, unmapped), at - d, cg, flag | unmapped, mapq)
    elif family == "aux":
        ab = bamwriter.aux_bytes
        fill = [("XA", "A", "q"), ("Xc", "c", -5), ("XC", "C", 200), ("Xs", "s", -300), ("XS", "S", 60000), ("Xi", "i", -70000), ("XI", "I", 4000000000),
                ("Xf", "f", 1.5), ("Xd", "d", 0.25), ("XZ", "Z", "CBZfake"), ("XH", "H", "1AE301"), ("Ba", "B", ("c", [-1, 2])), ("Bb", "B", ("C", [1, 2, 3])),
                ("Bc", "B", ("s", [-1])), ("Bd", "B", ("S", [1, 65535])), ("Be", "B", ("i", [-1, 7])), ("Bf", "B", ("I", [1])), ("Bg", "B", ("f", [0.5, 2.0])),
                ("B0", "B", ("i", [])), ("Bz", "B", ("C", []))]
        blocks = []
        for k in range(len(fill) + 1):
            blocks.append(("CB behind %d fields" % k, lambda cb, k=k: ab(fill[:k] + [("CB", "Z", cb), ("UB", "Z", "UMIx")] + fill[k:])))
        blocks += [("no aux", lambda cb: b""), ("CB alone, ends at the record's end", lambda cb: ab([("CB", "Z", cb)])),
                   ("absent", lambda cb: ab(fill)), ("twice", lambda cb: ab([("CB", "Z", cb), ("Xi", "i", 1), ("CB", "Z", "SECOND")])),
                   ("twice, the listed one second", lambda cb: ab([("CB", "Z", "FIRST"), ("CB", "Z", cb)])),
                   ("i then Z", lambda cb: ab([("CB", "i", 3), ("CB", "Z", cb), ("UB", "Z", "U")])),
                   ("Z then i", lambda cb: ab([("CB", "Z", cb), ("CB", "i", 3)])),
                   ("empty Z", lambda cb: ab([("CB", "Z", ""), ("UB", "Z", "U")])), ("empty UB", lambda cb: ab([("CB", "Z", cb), ("UB", "Z", "")])),
                   ("UB before CB", lambda cb: ab([("UB", "Z", "UMIy"), ("Xi", "i", 1), ("CB", "Z", cb)])),
                   ("UB twice", lambda cb: ab([("UB", "Z", "UMI1"), ("CB", "Z", cb), ("UB", "Z", "UMI2")])),
                   ("UB as i", lambda cb: ab([("CB", "Z", cb), ("UB", "i", 5)])),
                   ("CB of 65534 bytes", lambda cb: ab([("CB", "Z", b"A" * 65534), ("UB", "Z", "U")])),
                   ("CB of 65535 bytes", lambda cb: ab([("CB", "Z", b"C" * 65535), ("UB", "Z", "U")])),
                   ("UB of 65534 bytes", lambda cb: ab([("CB", "Z", cb), ("UB", "Z", b"G" * 65534)])),
                   ("not listed", lambda cb: ab([("CB", "Z", "NOTLISTED-1"), ("UB", "Z", "U")]))]
        for ty, val in (("A", "Q"), ("c", 7), ("C", 7), ("s", 7), ("S", 7), ("i", 7), ("I", 7), ("f", 7.0), ("d", 7.0), ("B", ("C", [65, 67, 71, 84])), ("B", ("f", []))):
            blocks.append(("CB as %s" % ty, lambda cb, ty=ty, val=val: ab([("Xi", "i", 1), ("CB", ty, val), ("UB", "Z", "U")])))
        for i, (name, make) in enumerate(blocks):
            flag, mapq = _flags_for(i)
            at = loci[(7 * i + 2) % len(loci)]
            add(name, at - 20 - i % 13, "60M", flag, mapq, aux=make(barcodes[i % 40]))
    elif family == "bases":
        for i in range(16):                              # each code on its own, then all of them, at both nibble positions
            at = loci[(2 * i + 3) % len(loci)]
            n = 100 + len(cases)                       # long enough to score above the reference's MIN_SCORE with the code as a mismatch
            body = fasta[at - 40:at - 40 + n].decode()
            add("code %d every 23rd base" % i, at - 40, "%dM" % n, seq="".join(_IUPAC[i] if j % 23 == 11 else ch for j, ch in enumerate(body)))
        for i, l_seq in enumerate((0, 1, 2, 3, 16, 17, 33)):
            at = loci[(4 * i) % len(loci)]
            add("l_seq %d" % l_seq, at, "40M", l_seq=l_seq, seq=(_IUPAC * 3)[i:i + l_seq])
        at = loci[9]
        add("all sixteen twice", at - 5, "32M", seq=_IUPAC + _IUPAC[::-1], l_seq=32)
        add("all N", at - 6, "41M", seq="N" * 41, l_seq=41)
        add("all =", at - 7, "43M", seq="=" * 43, l_seq=43)
    elif family == "layout":
        for i, qlen in enumerate((0, 1, 2, 3, 4, 5, 6, 7, 8, 100, 253, 254)):      # l_read_name 1 .. 255: every alignment of the later fields
            at = loci[(3 * i + 1) % len(loci)]
            for cg in ("60M", "*", "5H3S50M2S"):
                flag, mapq = _flags_for(len(cases))
                add("l_read_name %d, %s" % (qlen + 1, cg), at - 9, cg, flag, mapq, qname="q" * qlen)
        add("H in the CB value's place", loci[4] - 3, "60M", aux=bamwriter.aux_bytes([("CB", "B", ("c", [])), ("UB", "Z", "U")]))
        for k in range(5):                               # unplaced reads at the file's end
            add("tid -1 #%d" % k, -1, "*", flag=4, tid=-1)
            add("tid -1 with a position #%d" % k, loci[k], "60M", flag=4, tid=-1)
    else:
        raise ValueError(family)
    assert len({len(c["seq"]) for c in cases}) == len(cases), "every case its own l_seq"
    return cases


def write_family(path, cases, ref_len, block=700, index="linear"):
    """The cases as a coordinate-sorted BAM (tid -1 last) with BGZF blocks of `block` bytes: records straddle them."""
    from oracle import bamwriter
    order = sorted(range(len(cases)), key=lambda i: (cases[i]["tid"] < 0, cases[i]["tid"], cases[i]["pos"], i))
    recs = [bamwriter.record(c["tid"], c["pos"], c["qname"], c["seq"], encode(c["cigar"]), flag=c["flag"], mapq=c["mapq"], tags=[(None, "raw", c["aux"])])
            for c in (cases[i] for i in order)]
    bamwriter.write_bam(path, [("1", ref_len)], recs, block=block, index=index)
    return path


def predict(cases, vcf, barcodes, valid_chars=b"ATGCatgc", **opts):
    """What the model says becomes of every (case, locus) pair: -> (metrics of the seven read-level counters, {vcf row: sorted
    read_len of the kept reads})."""
    listed = set(barcodes)
    metrics = dict.fromkeys(("num_reads", "num_low_mapq", "num_non_primary", "num_duplicates", "num_not_cell_bc", "num_not_useful", "num_non_umi"), 0)
    kept = {}
    for row, v in enumerate(vcf):
        if len(v.alleles) > 2:
            continue
        start, end = v.pos, v.pos + len(v.alleles[0])
        kept[row] = []
        for c in cases:
            if c["tid"] != 0:
                continue
            o = pair_outcome(c, start, end, listed, **opts)
            if o is None:
                continue
            metrics["num_reads"] += 1
            if o == "kept":
                kept[row].append(len(c["seq"]))
            else:
                metrics[o] += 1
        kept[row].sort()
    return metrics, kept
