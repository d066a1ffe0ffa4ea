"""CPU unit tests of vartrix_amd/csrc/vtx_prep_core.h — the rules prep_resolve_kernel, prep_finalize_kernel, prep_check_kernel and
vtx_set_barcodes are compiled from (barcode lookup, UB test, UMI grouping, sort keys: reference src/main.rs:697-718, :737-750,
:867-888, :932, :1047-1057) — built for the host by tests/prepcore/Makefile.  The harness runs the WHOLE preparation from those
functions; it must equal oracle/prep.py on the authored cases of tests/prep_cases.py (whose premises are proved here first: the
colliding pairs collide, the wrap case wraps, the boundary cases have their heads where they say) and on 2 000 random tiny batches.
What the functions TOUCH is checked by a stand-alone program (tests/prepcore/main.cpp) in allocations of exactly the arrays' sizes,
plain and under AddressSanitizer and UBSan; nothing sanitized is loaded into Python.  Ten mutants of the header (VTXR_MUTANT), each
with one rule wrong, are each killed by the cases named in KILLERS.  The device runs the same cases in tests/test_gpu_prep_cases.py."""
import random

import numpy as np
import pytest

import prep_cases as PC
import prep_hash as ph
import prep_util as PU
from oracle import prep
from vartrix_amd.abi import LOCUS_DTYPE, RAW_RECORD_DTYPE, TAG_MISSING, RawBatch


@pytest.fixture(scope="module")
def core():
    return PU.load()


def oracle_of(raw, barcodes, use_umi):
    want, st = prep.prep_raw(raw, barcodes, bool(use_umi))
    return want, st, prep.canonical_records(want.records, want.loci["rec_begin"], want.loci["rec_count"])


def agrees(got, raw, barcodes, use_umi, rounds=None):
    """Is (status, stats, records, begin, count) what oracle/prep.py gives?  -> None, or what differs"""
    rc, st, recs, begin, count = got
    want, wst, wcanon = oracle_of(raw, barcodes, use_umi)
    if rc != 0:
        return "status %d" % rc
    if (st["num_not_cell_bc"], st["num_non_umi"], st["kept"]) != (wst["num_not_cell_bc"], wst["num_non_umi"], want.n_records):
        return "counters %r" % (st,)
    if rounds is not None and st["hash_rounds"] != rounds:
        return "hash_rounds %d, not %d" % (st["hash_rounds"], rounds)
    if not (np.array_equal(begin, want.loci["rec_begin"]) and np.array_equal(count, want.loci["rec_count"])):
        return "locus ranges %r %r" % (list(begin), list(count))
    if prep.canonical_records(recs, begin, count) != wcanon:
        return "records"
    for b0, c in zip(begin, count):          # the order vtx_submit demands: (cell, UMI group) non-decreasing inside a locus
        r = recs[int(b0):int(b0) + int(c)]
        if np.any(np.diff(r["cell_index"].astype(np.int64) << 32 | r["umi_id"].astype(np.int64)) < 0):
            return "order"
    return None


def case_verdict(L, c, weak_rounds=0):
    got = PU.prepare(L, c.raw, c.barcodes, c.use_umi, weak_rounds)
    bad = agrees(got, c.raw, c.barcodes, c.use_umi, rounds=2 if weak_rounds == 1 else c.hash_rounds)
    if bad is None:
        st = got[1]
        if (st["num_not_cell_bc"], st["num_non_umi"], st["kept"]) != (c.not_cell_bc, c.non_umi, c.kept):
            return "ledger counters %r" % (st,)
        cells = {int(r["read_off"]): int(r["cell_index"]) for r in got[2]}
        if cells != c.expected_cells():
            return "cells"
    return bad


# ---------------------------------------------------------------- hash, compare, seeds, widths, table ----------------------------------------------------------------
SEEDS = (0, PC.SEED0, PC.SEED1, 1, (1 << 64) - 1, 0x0123456789abcdef)


def test_mirror_equals_the_core_hash(core):
    rng = random.Random(1)
    for n in range(41):
        for data in (rng.randbytes(n), b"\x00" * n, b"\xff" * n, bytes(rng.choice(b"ACGT") for _ in range(n))):
            for seed in SEEDS:
                assert core.vtxt_hash_bytes(data, n, seed) == ph.hash_bytes(data, seed), (n, seed)
    s = 0
    for k in range(8):                       # the seed sequence of raw_prepare's rounds
        s = core.vtxt_next_seed(s)
        assert s == (PC.SEED0 if k == 0 else ph.next_seed(prev))
        prev = s


def bytes_equal_agrees(L):
    rng = random.Random(2)
    for n in range(41):
        a = rng.randbytes(n)
        if not L.vtxt_bytes_equal(a, bytes(a), n):
            return False
        for i in sorted({0, 6, 7, 8, 9, 15, 16, 17, n - 1} | set(range(n))):
            if 0 <= i < n:
                b = a[:i] + bytes([a[i] ^ (1 << rng.randrange(8))]) + a[i + 1:]
                if L.vtxt_bytes_equal(a, b, n):
                    return False
    return True


def test_bytes_equal_is_python_equality_over_all_length_pairs(core):
    """The compare as its callers use it — lengths first, then vtx_bytes_equal over that length — against ==, for every pair of
    lengths 0..40 of strings that share their common prefix, and for every single-byte difference (first, word edges, last)."""
    assert bytes_equal_agrees(core)
    rng = random.Random(3)
    stem = rng.randbytes(40)
    for la in range(41):
        for lb in range(41):
            a, b = stem[:la], stem[:lb]
            assert (la == lb and bool(core.vtxt_bytes_equal(a, b, la))) == (a == b)
            if la == lb and la:
                for i in (0, la - 1, min(7, la - 1), min(8, la - 1)):
                    b2 = b[:i] + bytes([b[i] ^ 0x80]) + b[i + 1:]
                    assert not core.vtxt_bytes_equal(a, b2, la)


def test_the_printable_constructor(core):
    """What the end-to-end BAM of tests/test_gpu_prep_cases.py is built from: 16 printable bytes with the hash of 16 others."""
    rng = random.Random(7)
    env = Env(core)
    for a, seed in ((b"ACGTACGTACGTAC-1", 0), (b"AACCGGTTAC-umi01", PC.SEED0)):
        b = ph.collide_printable(a, rng, seed)
        env.collide(a, b, seed)
        assert len(b) == 16 and all(0x21 <= x <= 0x7e for x in b) and env.hash(a, ph.next_seed(seed)) != env.hash(b, ph.next_seed(seed))


def bits(v):
    return max(1, int(v).bit_length())


def test_key_widths(core):
    out = np.zeros(4, np.uint64)
    for nb in list(range(0, 20)) + [255, 256, 257, 65535, 65536, 65537, 2 ** 32 - 1]:
        for nl in list(range(0, 20)) + [255, 256, 257, 2 ** 31, 2 ** 32 - 1]:
            core.vtxt_key_widths(nb, nl, out.ctypes.data)
            cb, eb, dropped, last = (int(x) for x in out)
            assert cb == bits(max(nb, 1) - 1) and eb == cb + bits(nl)
            assert dropped == nl << cb and dropped < 1 << eb            # the sort sees all of the dropped key
            if nl and nb:
                assert last == ((nl - 1) << cb | (nb - 1)) < dropped


def test_table_equals_the_mirror(core):
    rng = random.Random(4)
    lists = [c.barcodes for c in PC.CASES if c.group in ("barcode", "order")]
    for n in (0, 1, 2, 7, 8, 9, 15, 16, 17, 100, 1000):
        bcs = [rng.randbytes(rng.choice((0, 1, 7, 8, 9, 16, 18))) for _ in range(n)]
        lists.append(bcs + bcs[:n // 3])                                # with repeated entries
    for bcs in lists:
        slots = PU.table_slots(core, bcs)
        assert slots == ph.table_build(bcs)
        assert len(slots) == ph.table_capacity(len(bcs)) >= max(16, 2 * len(bcs)) and len(slots) < max(17, 4 * len(bcs))


def forged(L, entries, tag):
    """table_probe over a table whose hashes are set by hand: entry j lies in the slot its (forged) hash says"""
    bcs = [e[0] for e in entries]
    hashes = np.array([ph.hash_bytes(b) if h is None else h for b, h in entries], np.uint64)
    slots = np.zeros(16, np.uint32)
    for j, h in enumerate(hashes):
        s = int(h) & 15
        while slots[s]:
            s = (s + 1) & 15
        slots[s] = j + 1
    off, data = PU.barcode_arrays(bcs)
    got = L.vtxt_table_probe(slots.ctypes.data, 15, hashes.ctypes.data, off.ctypes.data, data.ctypes.data, len(bcs), tag, len(tag))
    return None if got == PU.NO_CELL else got


def test_the_length_compare_decides_in_forged_tables(core):
    for name, entries, tag, want in PC.forged_probe_cases():
        assert forged(core, entries, tag) == want, name


# ---------------------------------------------------------------- the ledger ----------------------------------------------------------------
class Env:
    """what a premise may ask: the hash (mirror and core must agree), the table, a case as the harness prepares it"""

    def __init__(self, L):
        self.L, self._prepared = L, {}

    def hash(self, p, seed):
        h = ph.hash_bytes(p, seed)
        assert self.L.vtxt_hash_bytes(p, len(p), seed) == h
        return h

    def collide(self, a, b, seed):
        assert a != b and self.hash(a, seed) == self.hash(b, seed), (a, b, seed)

    def check(self, ok):
        assert ok

    def slots(self, barcodes):
        slots = PU.table_slots(self.L, barcodes)
        assert slots == ph.table_build(barcodes)
        return slots

    def prepared(self, name):
        if name not in self._prepared:
            c = PC.BY_NAME[name]
            rc, st, recs, begin, count = PU.prepare(self.L, c.raw, c.barcodes, c.use_umi)
            assert rc == 0
            self._prepared[name] = (recs, begin, count)
        return self._prepared[name]


def test_the_ledger_names_what_the_issue_lists():
    names = set(PC.LEDGER)
    assert len(names) == len(PC.CASES)
    assert {"width_b%d_l%d_v%d" % (b, l, v) for b in (1, 2, 3, 4, 5, 8, 9) for l in (1, 2, 3, 4, 5, 7, 8, 9) for v in range(4)} <= names
    assert {"n_kept_%d" % n for n in (255, 256, 257, 511, 512, 513)} <= names
    assert {"boundary_%s_at_%d" % (k, a) for k in ("locus", "cell", "umi") for a in (256, 512)} <= names
    assert {"bc_list_of_%d" % n for n in (0, 1, 8, 9)} <= names and {"umi_last_byte_%d" % n for n in (7, 8, 9, 16, 17)} <= names
    assert PC.LEDGER["umi_collide_one_cell"]["hash_rounds"] == 2 and PC.LEDGER["umi_collide_two_cells"]["hash_rounds"] == 1
    assert all(e["rule"] and e["premise"] for e in PC.LEDGER.values())
    for c in PC.CASES:
        assert c.kept + c.not_cell_bc + c.non_umi == c.raw.n_records
    # tags: arbitrary bytes, shared, overlapping, flush against the arena's end
    c = PC.BY_NAME["bc_lengths_and_neighbours"]
    r, n = c.raw.records, c.raw.tag_arena.size
    assert 0 in c.raw.tag_arena and c.raw.tag_arena.max() >= 0x80
    assert (r["bc_off"].astype(np.int64) + r["bc_len"]).max() == n or (r["umi_off"].astype(np.int64) + r["umi_len"])[r["umi_len"] != TAG_MISSING].max() == n
    spans = sorted({(int(o), int(o) + int(ln)) for o, ln in zip(r["bc_off"], r["bc_len"]) if ln})
    assert len(spans) < len(r) and any(a[0] < b[0] < a[1] or (a[0] == b[0] and a[1] != b[1]) for a, b in zip(spans, spans[1:]))


def test_every_premise_of_the_ledger(core):
    env = Env(core)
    proved = 0
    for c in PC.CASES:
        for proof in c.proofs:
            proof(env)
            proved += 1
    assert proved == sum(len(c.proofs) for c in PC.CASES)
    for c in PC.CASES:                       # a constructed premise has its proof
        if c.name.startswith(("bc_collision", "bc_two_listed", "bc_probe_wraps", "bc_list_of", "umi_collide", "boundary_")):
            assert c.proofs, c.name
    # the cases of 256 and 512 kept records and the spanning group really have a record 256 whose predecessor decides
    recs, begin, count = env.prepared("group_spans_256")
    assert len(recs) == 300 and len(set(recs["umi_id"].tolist())) == 1 and list(count) == [300]
    for c in PC.CASES:                       # kept and raw indices differ wherever the boundary cases say so
        if c.group == "boundary" and c.name != "shape_caps":
            assert c.not_cell_bc and c.non_umi and c.kept >= 255


@pytest.mark.parametrize("group", ["barcode", "order", "umi", "width", "boundary"])
def test_harness_equals_the_oracle_on_every_case(core, group):
    cases = [c for c in PC.CASES if c.group == group]
    assert cases
    for c in cases:
        assert case_verdict(core, c) is None, c.name


def test_forced_equal_hashes_leave_the_byte_compare_alone(core):
    """weak_rounds = 1: every UMI hashes to 0 in the first round, so the byte (and length) compare is all that separates two molecules;
    the second round has the real hash.  Eight such rounds are the state error."""
    for name in PC.WEAK_ROUND_CASES:
        assert case_verdict(core, PC.BY_NAME[name], weak_rounds=1) is None, name
    c = PC.BY_NAME["umi_last_byte_9"]
    assert PU.prepare(core, c.raw, c.barcodes, 1, weak_rounds=8)[0] == -6
    assert PU.prepare(core, c.raw, c.barcodes, 1, weak_rounds=7)[1]["hash_rounds"] == 8


def test_a_bad_raw_record_is_turned_away(core):
    c = PC.BY_NAME["umi_interleaved"]
    n_tag, n_read = int(c.raw.tag_arena.size), int(c.raw.read_arena.size)
    for field, value, use_umi, bad in (("bc_off", n_tag - 10, 1, False), ("bc_off", n_tag - 9, 1, True), ("umi_off", n_tag - 10, 1, False),
                                       ("umi_off", n_tag - 9, 1, True), ("umi_off", n_tag - 9, 0, False), ("read_off", n_read - 32, 1, False),
                                       ("read_off", n_read - 31, 1, True)):
        recs = c.raw.records.copy()
        recs["bc_len"][2], recs["umi_len"][2] = 10, 10
        recs[field][2] = value
        raw = RawBatch(c.raw.loci, recs, c.raw.hap_arena, c.raw.read_arena, c.raw.tag_arena)
        assert (PU.prepare(core, raw, c.barcodes, use_umi)[0] == -1) == bad, (field, value)


def random_batch(rng):
    """A tiny batch over a tiny alphabet: variable-length tags that repeat, overlap and share bytes; lists with repeats and the empty string."""
    def tag():
        return bytes(rng.choice(b"A\x00\xff") for _ in range(rng.choice((0, 1, 1, 2, 2, 3, 8, 9, 16, 17))))
    barcodes = [tag() for _ in range(rng.randrange(0, 7))]
    pool = barcodes + [tag() for _ in range(4)]
    umis = [tag() for _ in range(rng.randrange(1, 5))]
    arena = bytearray(b"".join(pool + umis))
    nl = rng.randrange(0, 5)
    loci, recs = np.zeros(nl, LOCUS_DTYPE), []
    for l in range(nl):
        cnt = rng.randrange(0, 7)
        loci[l] = (l, len(recs), cnt, 0, 4, 4, 4, 0)
        for _ in range(cnt):
            if rng.random() < 0.8 and pool:
                t = rng.choice(pool)
                bo, bl = bytes(arena).find(t), len(t)
            else:                                                      # any span of the arena, its last bytes included
                bl = min(rng.randrange(0, 4), len(arena))
                bo = rng.randrange(0, len(arena) - bl + 1)
            if rng.random() < 0.15:
                uo, ul = 0, TAG_MISSING
            else:
                t = rng.choice(umis)
                uo, ul = bytes(arena).find(t), len(t)
            recs.append((2 * len(recs), 2, bo, uo, bl, ul))
    raw = RawBatch(loci, np.array(recs, RAW_RECORD_DTYPE).reshape(-1), np.frombuffer(b"ACGTACGT", np.uint8),
                   np.zeros(2 * len(recs) + 2, np.uint8), np.frombuffer(bytes(arena), np.uint8))
    return raw, barcodes, rng.randrange(2)


@pytest.fixture(scope="module")
def random_batches():
    rng = random.Random(20261021)
    return [random_batch(rng) for _ in range(2000)]


def test_harness_equals_the_oracle_on_2000_random_tiny_batches(core, random_batches):
    kept = dropped = 0
    for k, (raw, barcodes, use_umi) in enumerate(random_batches):
        got = PU.prepare(core, raw, barcodes, use_umi, weak_rounds=k % 3 == 0)
        assert agrees(got, raw, barcodes, use_umi) is None, k
        kept += got[1]["kept"]
        dropped += got[1]["num_not_cell_bc"] + got[1]["num_non_umi"]
    assert kept > 2000 and dropped > 2000


def test_the_stand_alone_program_runs_the_cases_clean_under_sanitizers(core, random_batches, tmp_path):
    """Every case and the first 300 random batches through tests/prepcore/main.cpp, each array in an allocation of exactly its size:
    the plain program and its AddressSanitizer + UBSan build exit 0 without a report and give what the harness gives."""
    items = [(c.raw, c.barcodes, c.use_umi, 0) for c in PC.CASES] + [(PC.BY_NAME[n].raw, PC.BY_NAME[n].barcodes, 1, 1) for n in PC.WEAK_ROUND_CASES]
    items += [(raw, barcodes, use_umi, 0) for raw, barcodes, use_umi in random_batches[:300]]
    want = [PU.prepare(core, raw, barcodes, use_umi, weak) for raw, barcodes, use_umi, weak in items]
    for san in (False, True):
        got = PU.run_program(items, str(tmp_path), san)
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g[0] == w[0] == 0 and all(g[1][key] == w[1][key] for key in g[1]), (san, k)
            assert np.array_equal(g[2], w[2]) and np.array_equal(g[3], w[3]) and np.array_equal(g[4], w[4]), (san, k)


# ---------------------------------------------------------------- mutants ----------------------------------------------------------------
# what kills each mutant: a ledger case, a ledger case with forced equal hashes ("@weak"), a forged table, or the compare's own test
KILLERS = {
    1: ("bc_collision_same_first_word", "bytes_equal"),                               # vtx_bytes_equal compares the first word only
    2: ("umi_last_byte_7@weak", "umi_last_byte_9@weak", "umi_last_byte_17@weak", "bytes_equal"),   # ... ignores the partial last word
    3: ("forged_prefix", "forged_extension"),                                         # the probe skips the length compare
    4: ("bc_two_listed_collide", "forged_prefix_then_tag", "forged_same_length_other_bytes"),      # ... stops at the first equal hash
    5: ("bc_probe_wraps",),                                                           # ... wraps to slot 1
    6: ("width_b1_l1_v3", "width_b3_l3_v3", "width_b4_l4_v3", "width_b9_l9_v3", "loci_empty_front", "n_kept_256"),   # dropped key = last locus
    7: ("width_b1_l1_v2", "width_b2_l2_v3", "width_b4_l4_v2", "width_b8_l8_v3", "width_b5_l3_v0", "loci_empty_end"),  # end_bit one short
    8: ("umi_collide_one_cell", "umi_collide_cross_length", "umi_last_byte_8@weak", "umi_trailing_nul@weak"),        # hashes only, no flag
    9: ("order_barcode_test_first", "bc_list_of_0"),                               # the UB test first
    10: ("group_spans_256", "boundary_locus_at_512", "n_kept_513"),                   # no predecessor at 256 k
}


def passes(L, name):
    if name == "bytes_equal":
        return bytes_equal_agrees(L)
    if name.startswith("forged_"):
        entries, tag, want = next(x[1:] for x in PC.forged_probe_cases() if x[0] == name)
        return forged(L, entries, tag) == want
    base, _, weak = name.partition("@")
    return case_verdict(L, PC.BY_NAME[base], weak_rounds=1 if weak else 0) is None


def test_the_real_header_passes_every_killer(core):
    for names in KILLERS.values():
        for name in names:
            assert passes(core, name), name


@pytest.mark.parametrize("mutant", PU.MUTANTS)
def test_every_mutant_is_killed_by_its_cases(mutant):
    L = PU.load(mutant)
    assert set(KILLERS) == set(PU.MUTANTS)
    for name in KILLERS[mutant]:
        assert not passes(L, name), "mutant %d survives %s" % (mutant, name)
