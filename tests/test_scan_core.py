"""CPU unit tests of vartrix_amd/csrc/vtx_scan_core.h — the record logic bam_scan_kernel is compiled from (view_record with htslib's
bam_endpos rule, the CIGAR walk behind useful_alignment, the aux lookup, the overlap-and-filter loop, the base codes) — built for
the host by tests/scancore/Makefile, against the independently written model in tests/bam_grammar_util.py.  The oracle's
vtxo_cigar_read_pos / vtxo_useful_alignment, oracle/refpipe.py's aux_string and the host packer's own copies (test hooks of
libvtxhost_dev.so) are compared with the same model on the same cases.  The device runs the same grammar through the kernel in
tests/test_gpu_bam_grammar.py.  What the record logic and the record-chain step TOUCH is checked by a stand-alone program
(tests/scancore/main.cpp) in allocations of exactly the device's sizes, plain and under AddressSanitizer and UBSan; nothing sanitized
is loaded into Python."""
import bisect
import ctypes as C
import itertools
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bam_grammar_util as M  # noqa: E402
from oracle import bamwriter, oracle, refpipe  # noqa: E402

SOME, NONE, ERR = M.SOME, M.NONE, M.ERR
NAMES = {SOME: "Some", NONE: "None", ERR: "Err"}
VTX_TAG_MISSING = 0xFFFF


@pytest.fixture(scope="module")
def core():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "scancore"), "-s"])
    L = C.CDLL(os.path.join(HERE, "scancore", "libscan_host.so"))
    L.vtxs_t_read_pos.argtypes = [C.c_void_p, C.c_uint32, C.c_int64, C.c_int64]
    L.vtxs_t_useful.argtypes = [C.c_void_p, C.c_uint32, C.c_int64, C.c_int64, C.c_int64]
    L.vtxs_t_read_pos_table.argtypes = L.vtxs_t_useful_table.argtypes = [C.c_void_p] * 2 + [C.c_uint64] + [C.c_void_p] * 4
    L.vtxs_t_read_pos_table.restype = L.vtxs_t_useful_table.restype = None
    L.vtxs_t_view.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p]
    L.vtxs_t_view_table.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.vtxs_t_view.restype = L.vtxs_t_view_table.restype = None
    L.vtxs_t_aux_string.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.POINTER(C.c_uint32)]
    L.vtxs_t_aux_string.restype = C.c_uint32
    L.vtxs_t_first_not_below.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int64]
    L.vtxs_t_first_not_below.restype = C.c_uint32
    L.vtxs_t_nt16.argtypes = [C.c_uint32]
    L.vtxs_t_nt16.restype = C.c_uint32
    L.vtxs_t_scan.argtypes = [C.c_char_p, C.c_uint64] + [C.c_void_p] * 7 + [C.c_uint32, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def hostdev():
    """The developer build of the host packer: vtxh_test_aux_string / vtxh_test_cigar_read_pos exist there only."""
    path = os.path.join(os.path.dirname(HERE), "vartrix_amd", "libvtxhost_dev.so")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    L = C.CDLL(path)
    L.vtxh_test_aux_string.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.vtxh_test_cigar_read_pos.argtypes = [C.c_void_p, C.c_uint32, C.c_int64, C.c_int64]
    return L


def ops_array(cigar):
    return np.array(M.encode(cigar), dtype=np.uint32)


def oracle_read_pos(a, pos, p):
    q = C.c_int64(-1)
    r = oracle.lib().vtxo_cigar_read_pos(a.ctypes.data, len(a), pos, p, 0, 1, C.byref(q))
    return r, (q.value if r == SOME else None)


def test_irregular_cigar_table(core, hostdev):
    """Every row of the hand-written table, in the model, the device header, the oracle and the host packer."""
    for txt, pos, probes, arm in M.IRREGULAR:
        cig = M.parse(txt)
        a = ops_array(cig)
        for p, want in probes.items():
            where = "%s at %d, probe %d (%s): want %s" % (txt or "*", pos, p, arm, NAMES[want])
            assert M.read_pos(cig, pos, p)[0] == want, "model, " + where
            assert core.vtxs_t_read_pos(a.ctypes.data, len(a), pos, p) == want, "vtx_scan_core.h, " + where
            assert oracle_read_pos(a, pos, p)[0] == want, "vtxo_cigar_read_pos, " + where
            assert hostdev.vtxh_test_cigar_read_pos(a.ctypes.data, len(a), pos, p) == want, "vtx_host.cpp, " + where
    for txt, pos, p, q in M.IRREGULAR_QPOS:
        cig = M.parse(txt)
        assert M.read_pos(cig, pos, p) == (SOME, q), (txt, p)
        assert oracle_read_pos(ops_array(cig), pos, p) == (SOME, q), (txt, p)


def enumerated_cigars():
    """Every CIGAR of 0 to 3 ops over the nine op codes with lengths in {0, 1, 3}: 1 + 27 + 27^2 + 27^3 = 20 440."""
    atoms = [(op, n) for op in M.OPS for n in (0, 1, 3)]
    for k in range(4):
        for c in itertools.product(atoms, repeat=k):
            yield list(c)


BIG = (1 << 28) - 1


def random_cigars(seed=20260, count=400):
    """4 to 8 ops, lengths that leave 16 bits (and one op at the format's limit, 2^28 - 1, in every eighth CIGAR)."""
    rng = random.Random(seed)
    out = []
    for t in range(count):
        k = rng.randint(4, 8)
        # mostly plausible shapes (clips outside, M-like ops inside) so that the walk gets far; some fully random
        if t % 4 == 3:
            ops = [rng.choice(M.OPS) for _ in range(k)]
        else:
            inner = [rng.choice("MMM=XIDNPS" if i else "MI=XSP") for i in range(k - 2)]
            ops = [rng.choice("HSM")] + inner + [rng.choice("HSM=")]
        cig = [(op, rng.choice([0, 1, 2, 3, 7, 150, 65535, 65536, 65537, 100000, 1 << 20])) for op in ops]
        if t % 8 == 0:
            i = rng.randrange(k)
            cig[i] = (cig[i][0] if t % 16 else "M", BIG)
        out.append(cig)
    return out


def boundary_probes(cig, pos, flag=0):
    """pos - 2 .. endpos + 2 when that is short, else two positions either side of every op's reference start and of the end."""
    end = M.endpos(cig, pos, flag)
    if end - pos <= 40:
        return list(range(pos - 2, end + 3))
    marks, at = {pos, end}, pos
    for op, n in cig:
        if op in M.REF_OPS:
            at += n
        marks.add(at)
    return sorted({m + d for m in marks for d in (-2, -1, 0, 1, 2)})


def run_tables(core, cigars, poss, probe_lists, window_lists):
    """One call per table into the device header -> (verdict per probe, useful per window), flat."""
    flat = np.array([c for cig in cigars for c in M.encode(cig)] or [0], dtype=np.uint32)
    cig_off = np.cumsum([0] + [len(c) for c in cigars]).astype(np.uint64)
    pos = np.array(poss, dtype=np.int64)
    probes = np.array([p for pl in probe_lists for p in pl], dtype=np.int64)
    probe_off = np.cumsum([0] + [len(pl) for pl in probe_lists]).astype(np.uint64)
    out = np.full(len(probes), 99, dtype=np.int8)
    core.vtxs_t_read_pos_table(flat.ctypes.data, cig_off.ctypes.data, len(cigars), pos.ctypes.data, probes.ctypes.data, probe_off.ctypes.data, out.ctypes.data)
    win = np.array([x for wl in window_lists for w in wl for x in w] or [0], dtype=np.int64)
    win_off = np.cumsum([0] + [len(wl) for wl in window_lists]).astype(np.uint64)
    uout = np.full(int(win_off[-1]), 99, dtype=np.int8)
    core.vtxs_t_useful_table(flat.ctypes.data, cig_off.ctypes.data, len(cigars), pos.ctypes.data, win.ctypes.data, win_off.ctypes.data, uout.ctypes.data)
    return out, uout


def check_cigar_space(core, cigars, poss):
    """Model vs device header vs oracle on every probe (verdict and, for the oracle, the query position), on windows of 1, 2 and 4
    positions, and on the end position with and without flag 0x4.  Returns the model's verdicts and phase coverage."""
    O = oracle.lib()
    probe_lists = [boundary_probes(c, p) for c, p in zip(cigars, poss)]
    window_lists = []
    for pl in probe_lists:
        have = set(pl)
        window_lists.append([(s, s + w) for s in pl[:-1] for w in (0, 1, 3) if all(p in have for p in range(s, s + w + 1))])
    dev, dev_useful = run_tables(core, cigars, poss, probe_lists, window_lists)
    counts = {SOME: 0, NONE: 0, ERR: 0}
    head_ops, body_ops = set(), set()
    q, wq = 0, 0
    qv = C.c_int64()
    for cig, pos, pl, wl in zip(cigars, poss, probe_lists, window_lists):
        a = ops_array(cig)
        ap, an = a.ctypes.data, len(a)
        valid = M.is_valid(cig)
        verdict = {}
        for p in pl:
            want, wq_pos = M.read_pos(cig, pos, p)
            verdict[p] = want
            counts[want] += 1
            if valid:
                assert M.read_pos_valid(cig, pos, p) == want, "the model's two derivations differ: %s at %d, probe %d" % (M.text(cig), pos, p)
            assert dev[q] == want, "vtx_scan_core.h: %s at %d, probe %d: %s, model %s" % (M.text(cig), pos, p, NAMES.get(int(dev[q])), NAMES[want])
            r = O.vtxo_cigar_read_pos(ap, an, pos, p, 0, 1, C.byref(qv))
            assert r == want and (want != SOME or qv.value == wq_pos), "vtxo_cigar_read_pos: %s at %d, probe %d: %s q %d, model %s q %s" % (
                M.text(cig), pos, p, NAMES.get(r), qv.value, NAMES[want], wq_pos)
            q += 1
        if len(cig) <= 3:
            for p in pl:
                h, b = M.phases(cig, pos, p)
                head_ops.update(h)
                body_ops.update(b)
        for s, e in wl:
            want = next((verdict[p] == SOME for p in range(s, e + 1) if verdict[p] != NONE), False)       # the first answer that is not None
            if valid:
                assert M.useful_valid(cig, pos, s, e) == want, (M.text(cig), pos, s, e)
            assert bool(dev_useful[wq]) == want, "vtx_scan_core.h useful_alignment: %s at %d, window [%d, %d]: %d, model %s" % (M.text(cig), pos, s, e, dev_useful[wq], want)
            assert bool(O.vtxo_useful_alignment(ap, an, pos, s, e)) == want, "vtxo_useful_alignment: %s at %d, window [%d, %d]" % (M.text(cig), pos, s, e)
            wq += 1
    assert q == len(dev) and wq == len(dev_useful)          # no case skipped
    # end position: the record as bytes through view_record, flag 0 and flag 0x4
    for flag in (0, 4, 0x14):
        recs = [bamwriter.record(0, p, "q", "", M.encode(c), flag=flag) for c, p in zip(cigars, poss)]
        off = np.cumsum([0] + [len(r) for r in recs]).astype(np.uint64)
        out = np.zeros(12 * len(recs), dtype=np.int64)
        core.vtxs_t_view_table(b"".join(recs), off.ctypes.data, len(recs), out.ctypes.data)
        out = out.reshape(-1, 12)
        for i, (c, p) in enumerate(zip(cigars, poss)):
            want = M.endpos(c, p, flag)
            assert out[i, 3] == want and out[i, 11] == 0, "vtx_scan_core.h view_record: end of %s at %d with flag %#x: %d, model %d" % (M.text(c), p, flag, out[i, 3], want)
            assert bamwriter._ref_span(recs[i])[2] == want, "bamwriter._ref_span: %s flag %#x" % (M.text(c), flag)
    return counts, head_ops, body_ops, q


def test_exhaustive_cigar_space(core):
    """All 20 440 CIGARs of up to three ops, every probe from pos - 2 to endpos + 2."""
    cigars = list(enumerated_cigars())
    assert len(cigars) == 1 + 27 + 27 ** 2 + 27 ** 3
    counts, head_ops, body_ops, n = check_cigar_space(core, cigars, [1000] * len(cigars))
    share = {NAMES[k]: v / n for k, v in counts.items()}
    print("enumerated (CIGAR, probe) pairs: %d, shares %s" % (n, share))
    assert min(share.values()) >= 0.05, share                # each outcome is at least 5 % of the pairs
    assert head_ops == set(M.OPS) and body_ops == set(M.OPS), (head_ops, body_ops)      # every op code in each phase of the walk


def test_refpipe_end_position_on_the_enumeration(tmp_path):
    """oracle/refpipe.py read_bam's `end` (what its fetch tests overlap with) on a sample of the enumeration, flags 0 and 0x4:
    htslib's bam_endpos, i.e. pos + 1 for an unmapped record whatever its CIGAR."""
    cigars = list(enumerated_cigars())[::7]
    for flag in (0, 4):
        recs = [bamwriter.record(0, 1000, "q", "", M.encode(c), flag=flag) for c in cigars]
        path = str(tmp_path / ("e%d.bam" % flag))
        bamwriter.write_bam(path, [("1", 100000)], recs)
        got = refpipe.read_bam(path).recs
        assert len(got) == len(cigars)
        for c, r in zip(cigars, got):
            assert r.end == M.endpos(c, 1000, flag), "refpipe.read_bam: end of %s with flag %#x: %d, model %d" % (M.text(c), flag, r.end, M.endpos(c, 1000, flag))


def test_long_cigars_with_large_lengths(core):
    """A seeded sample of 4 to 8 ops with lengths above 2^16 and ops at 2^28 - 1, probed around every op boundary."""
    cigars = random_cigars()
    assert any(n == BIG for c in cigars for _, n in c) and any(n > 1 << 16 for c in cigars for _, n in c)
    rng = random.Random(5)
    poss = [rng.choice([0, 1, 5000, 1 << 20]) for _ in cigars]
    counts, _, _, n = check_cigar_space(core, cigars, poss)
    assert all(v > 0 for v in counts.values()), counts


# ---------------------------------------------------------------------------------------------------------------------------
# aux
# ---------------------------------------------------------------------------------------------------------------------------
FILLERS = [("XA", "A", "q"), ("Xc", "c", -5), ("XC", "C", 200), ("Xs", "s", -300), ("XS", "S", 60000), ("Xi", "i", -70000), ("XI", "I", 4000000000),
           ("Xf", "f", 1.5), ("Xd", "d", 0.25), ("XZ", "Z", "text"), ("XH", "H", "1AE301"), ("Ba", "B", ("c", [-1, 2])), ("Bb", "B", ("C", [1, 2, 3])),
           ("Bc", "B", ("s", [-1])), ("Bd", "B", ("S", [1, 65535])), ("Be", "B", ("i", [-1, 7])), ("Bf", "B", ("I", [1])), ("Bg", "B", ("f", [0.5, 2.0])),
           ("B0", "B", ("i", [])), ("Bz", "B", ("C", []))]
NON_Z = [("A", "Q"), ("c", 7), ("C", 7), ("s", 7), ("S", 7), ("i", 7), ("I", 7), ("f", 7.0), ("d", 7.0), ("B", ("C", [65, 67, 71, 84])), ("B", ("i", []))]


def aux_corpus():
    """(name, aux bytes, well formed).  The wanted tag is CB (and UB)."""
    ab = bamwriter.aux_bytes
    cb = ("CB", "Z", "ACGT-1")
    out = [("no aux bytes at all", b"", True), ("CB alone", ab([cb]), True), ("absent", ab(FILLERS), True),
           ("first", ab([cb] + FILLERS), True), ("last: the value ends at the record's end", ab(FILLERS + [cb]), True)]
    for k in range(1, len(FILLERS)):
        out.append(("in the middle, behind %s" % FILLERS[k - 1][1], ab(FILLERS[:k] + [cb] + FILLERS[k:]), True))
    out += [("twice: the first wins", ab([("CB", "Z", "FIRST")] + FILLERS[:3] + [("CB", "Z", "SECOND")]), True),
            ("Z then i", ab([("CB", "Z", "FIRST"), ("CB", "i", 3)]), True),
            ("i then Z: the first occurrence is no string", ab([("CB", "i", 3), ("CB", "Z", "SECOND")]), True),
            ("empty Z", ab([("XZ", "Z", ""), ("CB", "Z", ""), ("UB", "Z", "U")]), True),
            ("empty Z last", ab([("UB", "Z", "U"), ("CB", "Z", "")]), True),
            ("UB before CB", ab([("UB", "Z", "UMI"), ("Xi", "i", 1), cb]), True),
            ("65534 bytes", ab([("Xi", "i", 1), ("CB", "Z", b"A" * 65534), ("UB", "Z", "U")]), True),
            ("65535 bytes", ab([("CB", "Z", b"C" * 65535), ("UB", "Z", "U")]), True),
            ("70000 bytes", ab([("UB", "Z", b"G" * 70000), ("CB", "Z", b"T" * 70000)]), True),
            ("lower-case look-alike", ab([("cb", "Z", "no"), ("Cb", "Z", "no"), ("BC", "Z", "no")]), True),
            ("tag bytes inside a value", ab([("XZ", "Z", "CBZfake"), ("Bb", "B", ("C", list(b"CBZfake\x00"))), cb]), True)]
    for ty, val in NON_Z:
        out.append(("CB as %s%s" % (ty, ":" + val[0] + str(len(val[1])) if ty == "B" else ""), ab(FILLERS[:2] + [("CB", ty, val), ("UB", "Z", "U")]), True))
    # malformed blocks
    out += [("ends right after a Z header", ab(FILLERS[:4]) + b"CBZ", False), ("ends right after an i header", ab(FILLERS[:4]) + b"CBi", False),
            ("ends right after a B header", ab(FILLERS[:4]) + b"CBB", False), ("ends inside a B header", ab([cb]) + b"XBBi\x01\x00", False),
            ("Z without its NUL", b"CBZACGT", False), ("Z without its NUL behind CB", ab([cb]) + b"XZZabc", False),
            ("unknown type in front of CB", b"XQ?\x00" + ab([cb]), False), ("unknown type behind CB", ab([cb]) + b"XQ?\x00", False),
            ("unknown B subtype in front of CB", b"XBBx\x01\x00\x00\x00abcd" + ab([cb]), False),
            ("B count beyond the block in front of CB", b"XBBi\xff\xff\xff\x7f" + ab([cb]), False),
            ("B count 0xffffffff", b"XBBC\xff\xff\xff\xff" + ab([cb]), False),
            ("i cut short", ab([("UB", "Z", "U")]) + b"CBi\x01\x02", False), ("one stray byte", ab([cb]) + b"X", False),
            ("two stray bytes", ab([("UB", "Z", "U")]) + b"CB", False)]
    return out


def refpipe_lookup(aux, tag):
    """refpipe.aux_string; "raises" where malformed bytes make it raise."""
    try:
        return refpipe.aux_string(aux, tag)
    except (ValueError, KeyError, struct.error, IndexError):
        return "raises"


def c_lookups(core, hostdev, aux, tag):
    ln = C.c_uint32(0)
    o = core.vtxs_t_aux_string(aux, len(aux), tag, C.byref(ln))
    dev = None if o == 0xFFFFFFFF else bytes(aux[o:o + ln.value])
    ho, hl = C.c_uint64(0), C.c_uint64(0)
    host = bytes(aux[ho.value:ho.value + hl.value]) if hostdev.vtxh_test_aux_string(aux, len(aux), tag, C.byref(ho), C.byref(hl)) else None
    return dev, host


def test_aux_corpus(core, hostdev):
    """Every type and B subtype, the wanted tag first / in the middle / last / absent / twice / of another type, the empty Z, values
    at the 16-bit edge, blocks that stop early.  Device header == host packer == model everywhere; refpipe == model on well-formed
    blocks.  On a malformed block refpipe may raise where the C copies answer for what lies in front of the malformed spot
    ("missing" when the tag is not there): that is asserted as it is — refpipe either raises or agrees, and it must raise or say
    None whenever the model says missing."""
    seen_raise = 0
    for name, aux, well in aux_corpus():
        assert M.tokenise(aux)[1] == well, name
        for tag in (b"CB", b"UB", b"XZ", b"Bg", b"ZZ"):
            want = M.aux_lookup(aux, tag)
            dev, host = c_lookups(core, hostdev, aux, tag)
            assert dev == want, "vtx_scan_core.h aux_string, case %r, tag %s: %r, model %r" % (name, tag.decode(), dev and dev[:20], want and want[:20])
            assert host == want, "vtx_host.cpp aux_string, case %r, tag %s: %r, model %r" % (name, tag.decode(), host and host[:20], want and want[:20])
            ref = refpipe_lookup(aux, tag)
            if well:
                assert ref == want, "refpipe.aux_string, case %r, tag %s" % (name, tag.decode())
            else:
                seen_raise += ref == "raises"
                assert ref == "raises" or ref == want, "refpipe.aux_string, malformed case %r, tag %s: %r, model %r" % (name, tag.decode(), ref, want)
    assert seen_raise >= 8
    # exactly what happens on the blocks that stop early
    ab = bamwriter.aux_bytes
    for aux in (ab(FILLERS[:4]) + b"CBZ", b"CBZACGT", b"XQ?\x00" + ab([("CB", "Z", "ACGT-1")])):
        assert c_lookups(core, hostdev, aux, b"CB") == (None, None) and M.aux_lookup(aux, b"CB") is None
        assert refpipe_lookup(aux, b"CB") == "raises"
    # a wanted tag IN FRONT of the malformed spot is still answered (the lookup stops at the tag)
    aux = ab([("CB", "Z", "ACGT-1")]) + b"XQ?\x00"
    assert c_lookups(core, hostdev, aux, b"CB") == (b"ACGT-1", b"ACGT-1") and refpipe_lookup(aux, b"CB") == b"ACGT-1"


def test_hex_tag_is_not_a_string(core, hostdev):
    """ASSUMPTION, not derivable on this machine (the crate's source is not here; labelled like the recollected details of
    tests/golden/band_kat.json): rust-htslib 0.36's Record::aux returns Aux::HexByteArray for a type-H field, not Aux::String, so
    `CB:H:...` is no barcode for get_cell_barcode (src/main.rs:742-748) and the pair lands in num_not_cell_bc.  Every copy in the
    repository reads it that way.  A failure here means one copy changed its reading; if the crate turns out to return
    Aux::String for H, ALL copies and bam_grammar_util.aux_lookup change together — nothing else in the suite depends on this."""
    aux = bamwriter.aux_bytes([("Xi", "i", 1), ("CB", "H", "1AE301"), ("UB", "Z", "U")])
    assert M.aux_lookup(aux, b"CB") is None
    assert c_lookups(core, hostdev, aux, b"CB") == (None, None)
    assert refpipe.aux_string(aux, b"CB") is None
    assert M.aux_lookup(aux, b"UB") == b"U" and c_lookups(core, hostdev, aux, b"UB") == (b"U", b"U")      # H is stepped over like Z


# ---------------------------------------------------------------------------------------------------------------------------
# record layout, bases, the overlap-and-filter loop
# ---------------------------------------------------------------------------------------------------------------------------
def view(core, blob, p=0):
    out = np.zeros(12, dtype=np.int64)
    core.vtxs_t_view(blob, p, out.ctypes.data)
    return dict(zip(("bs", "tid", "pos", "endpos", "mapq", "flag", "n_cig", "l_seq", "cig", "sq", "aux", "malformed"), (int(x) for x in out)))


@pytest.mark.parametrize("shift", [0, 1, 2, 3, 5])
def test_record_layout_extremes(core, shift):
    """l_read_name 1 and 255 and everything between that moves the later fields' alignment; l_seq 0, 1, odd, even; 0 and many
    CIGAR ops; the record at every byte alignment inside the buffer (`shift`); tid -1."""
    for qlen, l_seq, cigar, tid, flag, mapq in itertools.product((0, 1, 2, 3, 17, 254), (0, 1, 2, 7, 150), ("*", "3S", "2H3M1D2=1X4N1I2P3S"), (0, 3, -1), (0, 0x4, 0x904), (0, 255)):
        seq = "".join(M.NT16[(i * 7 + qlen) % 16] for i in range(l_seq))
        tags = [("CB", "Z", "AC-1")] if l_seq % 2 else []
        rec = bamwriter.record(tid, 123456, "n" * qlen, seq, cigar, flag=flag, mapq=mapq, tags=tags)
        blob = b"\xa5" * shift + rec + b"\xa5" * 8
        v = view(core, blob, shift)
        cig = M.parse("" if cigar == "*" else cigar)
        want = dict(bs=len(rec) - 4, tid=tid, pos=123456, endpos=M.endpos(cig, 123456, flag), mapq=mapq, flag=flag, n_cig=len(cig), l_seq=l_seq,
                    cig=32 + qlen + 1, sq=32 + qlen + 1 + 4 * len(cig), aux=32 + qlen + 1 + 4 * len(cig) + (l_seq + 1) // 2 + l_seq, malformed=0)
        assert v == want, (qlen, l_seq, cigar, tid, flag, mapq)
        assert M.decode_bases(rec[4 + v["sq"]:], l_seq) == seq
        assert len(rec) - 4 - v["aux"] == len(bamwriter.aux_bytes(tags))
    # fields that run past block_size: declined, and the aux block is empty rather than somewhere outside the record
    rec = bytearray(bamwriter.record(0, 10, "name", "ACGT", "4M"))
    struct.pack_into("<i", rec, 20, 4000)                # l_seq
    v = view(core, bytes(rec))
    assert v["malformed"] == 1 and v["aux"] == v["bs"] and v["endpos"] == 11
    rec = bytearray(bamwriter.record(0, 10, "name", "ACGT", "4M"))
    struct.pack_into("<H", rec, 16, 60000)               # n_cigar_op
    assert view(core, bytes(rec))["malformed"] == 1


def test_base_codes(core):
    """The 16 nibble codes: the header's table (unpack_nibbles_kernel decodes with it), refpipe's, the packer-side helpers'."""
    from vartrix_amd import abi
    for code in range(16):
        assert chr(core.vtxs_t_nt16(code)) == M.NT16[code], "vtx_scan_core.h nt16_char: code %d -> %r, SAM spec %r" % (code, chr(core.vtxs_t_nt16(code)), M.NT16[code])
        assert chr(refpipe.SEQ_NT16[code]) == M.NT16[code]
        assert bamwriter._NT16[M.NT16[code]] == code
    allb = "".join(M.NT16).encode()
    assert bytes(abi.pack_nibbles(np.frombuffer(allb, np.uint8))) == bytes((2 * i << 4) | (2 * i + 1) for i in range(8))


def test_first_not_below(core):
    rng = random.Random(3)
    for _ in range(300):
        n = rng.randint(0, 40)
        starts = sorted(rng.randint(-5, 60) for _ in range(n))
        a = np.array(starts + [0], dtype=np.int32)
        lo = rng.randint(0, n)
        for e in range(-7, 63):
            assert core.vtxs_t_first_not_below(a.ctypes.data, lo, n, e) == max(lo, bisect.bisect_left(starts, e))


def scan(core, rec, flt, iv, n_ref=2, tid_of_iv=0):
    """The counting pass on one record.  iv: sorted (start, end) of contig `tid_of_iv`."""
    st = np.array([s for s, _ in iv] + [0], dtype=np.int32)
    en = np.array([e for _, e in iv] + [0], dtype=np.int32)
    tb = np.array([0 if t <= tid_of_iv else len(iv) for t in range(n_ref + 1)], dtype=np.uint32)
    span = np.array([max([e - s for s, e in iv], default=0) if t == tid_of_iv else 0 for t in range(n_ref)], dtype=np.int32)
    f = np.array([n_ref, flt.get("mapq", 0), int(flt.get("primary_only", False)), int(flt.get("no_duplicates", False)),
                  struct.unpack("<H", flt.get("bam_tag", b"CB"))[0]], dtype=np.uint32)
    pk, po, vd = np.zeros(64, np.uint32), np.zeros(64, np.uint32), np.zeros(11, np.uint32)
    n = core.vtxs_t_scan(rec, 0, f.ctypes.data, st.ctypes.data, en.ctypes.data, tb.ctypes.data, span.ctypes.data, pk.ctypes.data, po.ctypes.data, 64, vd.ctypes.data)
    names = ("hits", "reads", "low_mapq", "non_primary", "duplicate", "not_useful", "no_barcode", "bc_rel", "umi_rel", "bc_len", "umi_len")
    return n, [(int(k), int(o)) for k, o in zip(pk[:max(n, 0)], po[:max(n, 0)])], dict(zip(names, (int(x) for x in vd)))


OUTCOME = {None: None, "kept": 0, "num_low_mapq": 1, "num_non_primary": 2, "num_duplicates": 3, "num_not_useful": 4, "num_not_cell_bc": 5}


def test_overlap_and_filter_loop(core):
    """scan_pairs on single records against the model: which intervals are visited (htslib's overlap of [pos, endpos) with
    [start, end), highest interval first), what becomes of each pair, the counters, where the tag bytes lie."""
    rng = random.Random(11)
    iv = sorted({(s, s + w) for s in range(90, 140, 3) for w in (1, 2, 9)})
    aux_choices = [[("CB", "Z", "ACGT-1"), ("UB", "Z", "UMI1")], [("UB", "Z", "UMI1"), ("Xi", "i", 3), ("CB", "Z", "ACGT-1")], [("CB", "Z", "ACGT-1")],
                   [("UB", "Z", "UMI1")], [], [("CB", "i", 5), ("CB", "Z", "ACGT-1")], [("CB", "Z", b"A" * 65534), ("UB", "Z", b"U" * 65535)],
                   [("CB", "Z", b"A" * 65535), ("UB", "Z", "U")], [("CB", "Z", ""), ("UB", "Z", "")]]
    cig_choices = ["10M", "*", "3S4M2D4M", "2D5M", "5M2H5M", "4M6N4M", "3H", "5H3S10M", "1I", "3M0D3M", "2=2X", "6M3S2H"]
    n_cases = 0
    for cigar, tags, flag, mapq, flt in itertools.product(cig_choices, aux_choices, (0, 0x4, 0x100, 0x400, 0x800), (0, 40),
                                                          (dict(), dict(mapq=30), dict(primary_only=True, no_duplicates=True))):
        if rng.random() < 0.6:
            continue
        pos = rng.choice([80, 95, 100, 118, 139, 150])
        seq = "ACGTN"[:rng.randint(0, 5)]
        rec = bamwriter.record(0, pos, "r", seq, cigar, flag=flag, mapq=mapq, tags=tags)
        aux = bamwriter.aux_bytes(tags)
        cig = M.parse("" if cigar == "*" else cigar)
        case = dict(pos=pos, cigar=cig, flag=flag, mapq=mapq, aux=aux)
        cb = M.aux_lookup(aux, b"CB")
        listed = {cb} if cb is not None and len(cb) < VTX_TAG_MISSING else set()        # (a value of 65 535 bytes or more cannot travel: missing)
        want = [(k, OUTCOME[M.pair_outcome(case, s, e, listed, **flt)]) for k, (s, e) in enumerate(iv)]
        want = [(k, o) for k, o in reversed(want) if o is not None]
        n, pairs, V = scan(core, rec, flt, iv)
        label = "%s pos %d flag %#x mapq %d tags %s filter %s" % (cigar, pos, flag, mapq, [t[:2] for t in tags], flt)
        assert n == len(want) and pairs == want, label + ": pairs %s, model %s" % (pairs[:6], want[:6])
        for name, code in (("low_mapq", 1), ("non_primary", 2), ("duplicate", 3), ("not_useful", 4), ("no_barcode", 5), ("hits", 0)):
            assert V[name] == sum(o == code for _, o in want), (label, name)
        assert V["reads"] == len(want)
        if any(o in (0, 5) for _, o in want):          # the tags were looked up
            body = rec[4:]
            got_cb = body[V["bc_rel"]:V["bc_rel"] + V["bc_len"]] if V["bc_len"] != VTX_TAG_MISSING else None
            assert got_cb == (cb if listed else None), label
            if got_cb is not None:
                ub = M.aux_lookup(aux, b"UB")
                ub = ub if ub is not None and len(ub) < VTX_TAG_MISSING else None
                got_ub = body[V["umi_rel"]:V["umi_rel"] + V["umi_len"]] if V["umi_len"] != VTX_TAG_MISSING else None
                assert got_ub == ub, label
        n_cases += 1
    assert n_cases > 800
    # other contigs and tid -1 (the unplaced reads at a file's end): no pair
    for tid in (1, 2, 7, -1):
        rec = bamwriter.record(tid, 100, "r", "ACGT", "10M", tags=[("CB", "Z", "ACGT-1")])
        assert scan(core, rec, {}, iv)[:2] == (0, [])


# ---------------------------------------------------------------------------------------------------------------------------
# what the record logic touches: the stand-alone program, plain and sanitized
# ---------------------------------------------------------------------------------------------------------------------------
def run_program(cases, tmp, san):
    """cases: [(kind, payload)] through tests/scancore/main.cpp in ONE process -> [bytes]."""
    name = "scan_host_san" if san else "scan_host"
    subprocess.check_call(["make", "-C", os.path.join(HERE, "scancore"), "-s", name])
    src, dst = os.path.join(tmp, name + ".in"), os.path.join(tmp, name + ".out")
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for kind, payload in cases:
            f.write(struct.pack("<II", kind, len(payload)) + payload)
    r = subprocess.run([os.path.join(HERE, "scancore", name), src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, "exit %d\n%s" % (r.returncode, r.stderr[-4000:])
    blob, q, out = open(dst, "rb").read(), 0, []
    for _ in cases:
        m, = struct.unpack_from("<I", blob, q)
        out.append(blob[q + 4:q + 4 + m])
        q += 4 + m
    assert q == len(blob)
    return out


def with_raw_aux(rec, aux):
    """A record of bamwriter's with `aux` as its aux block, whatever the bytes are."""
    return struct.pack("<I", len(rec) - 4 + len(aux)) + rec[4:] + aux


def chain_model(data, p, stop):
    """The walk of bam_chain_kernel / bam_chain_seg_kernel as they were written before the step moved into vtx_scan_core.h:
    (records, bad, p at the end, highest byte offset read + 1)."""
    limit, k, bad, read_to = len(data), 0, False, 0
    while p < stop:
        if p + 36 > limit:
            bad = True
            break
        bs, = struct.unpack_from("<I", data, p)
        read_to = max(read_to, p + 4)
        if bs < 32 or p + 4 + bs > limit:
            bad = True
            break
        k += 1
        p += 4 + bs
    return k, int(bad or p != stop), p, read_to


def chain_corpus():
    """[(name, data, p, stop)]: block_size 0, 31, 32 and 0xFFFFFFFF in the first, a middle and the last record; the last record
    ending exactly at the limit, one byte past it, and with fewer than 36 bytes left in front of the limit."""
    def rec(bs, body=None):
        return struct.pack("<I", bs) + b"\x5a" * (bs if body is None else body)
    good = [rec(32), rec(40), rec(33), rec(100)]
    out = []
    whole = b"".join(good)
    out.append(("four records, the last ends exactly at the limit", whole, 0, len(whole)))
    out.append(("the last record ends one byte past the limit", whole[:-1], 0, len(whole)))
    out.append(("the last record ends one byte past the limit, stop at the limit", whole[:-1], 0, len(whole) - 1))
    out.append(("a record of 36 bytes is all there is", rec(32), 0, 36))
    out.append(("35 bytes left in front of the limit", whole + rec(32)[:35], 0, len(whole) + 36))
    out.append(("4 bytes left in front of the limit", whole + rec(32)[:4], 0, len(whole) + 36))
    out.append(("nothing left in front of the limit, stop behind it", whole, 0, len(whole) + 36))
    out.append(("the chain steps over the stop", whole, 0, len(whole) - 50))
    out.append(("starts at the stop", whole, 36, 36))
    out.append(("starts behind the limit", whole, len(whole) + 8, len(whole) + 80))
    for bs in (0, 31, 32, 0xFFFFFFFF, 0x7FFFFFFF, 0xFFFFFFFC):
        for where in range(4):
            recs = list(good)
            recs[where] = rec(bs, body=bs if bs <= 32 else 32)
            data = b"".join(recs)
            out.append(("block_size %#x in record %d" % (bs, where), data, 0, len(data)))
    return out


def test_the_record_logic_reads_nothing_outside_the_inflated_buffer(core, tmp_path):
    """view_record, aux_string and scan_pairs on the record-layout extremes, the malformed records and the aux corpus (each aux
    block also as the aux block of a record that gets as far as the tag lookup), every record or block the LAST thing of a buffer
    of exactly its size + 64; the chain walk over buffers of exactly `limit` bytes.  The stand-alone program answers what the
    shared object answers in the tests above (and, for aux blocks and chains, what the models say), and its build under
    AddressSanitizer and UBSan exits 0 without a report and answers the same."""
    cases, want = [], []
    fills = (0x00, 0xFF, 0xA5)
    # view_record
    recs = []
    for qlen, l_seq, cigar, flag in itertools.product((0, 1, 3, 254), (0, 1, 7, 150), ("*", "3S", "2H3M1D2=1X4N1I2P3S"), (0, 0x4)):
        seq = "".join(M.NT16[(i * 7 + qlen) % 16] for i in range(l_seq))
        recs.append(bamwriter.record(3, 123456, "n" * qlen, seq, cigar, flag=flag, tags=[("CB", "Z", "AC-1")] if l_seq % 2 else []))
    malformed = []
    for off, fmt, val in ((20, "<i", 4000), (16, "<H", 60000), (20, "<i", 0x7FFFFFFF), (12, "<B", 255)):
        r = bytearray(bamwriter.record(0, 10, "name", "ACGT", "4M"))
        struct.pack_into(fmt, r, off, val)                   # l_seq, n_cigar_op, l_seq, l_read_name beyond block_size
        malformed.append(bytes(r))
    for i, r in enumerate(recs + malformed):
        pre = (0, 1, 2, 3, 5)[i % 5]
        cases.append((0, struct.pack("<II", pre, fills[i % 3]) + r))
        v = view(core, b"\xa5" * pre + r + b"\xa5" * 8, pre)
        want.append(struct.pack("<12q", *v.values()))
    for r in malformed:
        v = view(core, r + b"\xa5" * 8)
        assert v["malformed"] == 1 and v["aux"] == v["bs"] and v["endpos"] == 11
    # aux_string
    for i, (name, aux, _) in enumerate(aux_corpus()):
        for tag in (b"CB", b"UB", b"XZ", b"Bg", b"ZZ"):
            cases.append((1, struct.pack("<III", i % 7, fills[i % 3], struct.unpack("<H", tag)[0]) + aux))
            got = M.aux_lookup(aux, tag)
            # (the offset of the value: behind the first occurrence of tag + 'Z' that the model's tokens name)
            want.append(("aux", aux, got))
    # scan_pairs: the aux corpus as the aux block of a record that overlaps loci, and the filters
    iv = sorted({(s, s + w) for s in range(90, 140, 3) for w in (1, 2, 9)})
    st = np.array([s for s, _ in iv], dtype=np.int32)
    en = np.array([e for _, e in iv], dtype=np.int32)
    tables = st.tobytes() + en.tobytes() + struct.pack("<3I", 0, len(iv), len(iv)) + struct.pack("<2i", 9, 0)
    scans = [(with_raw_aux(bamwriter.record(0, 100, "r", "ACGTN", "10M"), aux), {}) for _, aux, _ in aux_corpus()]
    for cigar, flag, flt in itertools.product(("10M", "*", "3S4M2D4M", "5M2H5M", "3H", "6M3S2H"), (0, 0x4, 0x100, 0x400), (dict(), dict(mapq=30), dict(primary_only=True, no_duplicates=True))):
        scans.append((bamwriter.record(0, 118, "r", "ACG", cigar, flag=flag, mapq=40, tags=[("UB", "Z", "UMI1"), ("Xi", "i", 3), ("CB", "Z", "ACGT-1")]), flt))
    scans.append((bamwriter.record(-1, 100, "r", "ACGT", "10M", tags=[("CB", "Z", "ACGT-1")]), {}))
    scans.append((malformed[0], {}))
    for i, (r, flt) in enumerate(scans):
        f = struct.pack("<5I", 2, flt.get("mapq", 0), int(flt.get("primary_only", False)), int(flt.get("no_duplicates", False)), struct.unpack("<H", b"CB")[0])
        cases.append((2, struct.pack("<II", i % 5, fills[i % 3]) + f + struct.pack("<II", 2, len(iv)) + tables + r))
        n, pairs, V = scan(core, r, flt, iv)
        assert n >= -1
        want.append(struct.pack("<i11I", n, *V.values()) + b"".join(struct.pack("<II", k, o) for k, o in pairs))
    assert sum(w[:4] != b"\0\0\0\0" and w[:4] != b"\xff\xff\xff\xff" for w in want[-len(scans):]) > 100      # most records meet loci
    # the record-chain walk
    chains = chain_corpus()
    verdicts = set()
    for name, data, p, stop in chains:
        cases.append((3, struct.pack("<QQ", p, stop) + data))
        k, bad, end, read_to = chain_model(data, p, stop)
        assert read_to <= len(data), name                   # the kernels as they were read nothing at or beyond the limit
        verdicts.add((bad, k > 0))
        want.append(struct.pack("<IIQ", k, bad, end))
    assert verdicts == {(0, True), (0, False), (1, True), (1, False)}
    assert chain_model(chains[0][1], 0, len(chains[0][1]))[:2] == (4, 0) and chain_model(chains[1][1], 0, len(chains[1][1]) + 1)[:2] == (3, 1)

    for san in (False, True):
        got = run_program(cases, str(tmp_path), san)
        for (kind, _), g, w in zip(cases, got, want):
            if kind == 1:
                _, aux, val = w
                o, ln = struct.unpack("<II", g)
                assert (None if o == 0xFFFFFFFF else aux[o:o + ln]) == val, (san, aux[:40], val)
            elif kind == 2 and w[:4] == b"\xff\xff\xff\xff":
                assert g[:4] == w[:4], san                   # a malformed record is not scanned: there is no verdict to compare
            else:
                assert g == w, (san, kind)
