"""CPU side of the table checks: the checker of tests/tables_model.py is tied to the header, the corpus of tests/tables_cases.py holds what
it claims, the host mirror's tables (tests/fastcore/fastcore_host.cpp: build_table, exported as vtxt_build_tables) pass the checker, and
the checker rejects every single corruption under the name of the property it breaks.  The device's tables meet the same checker and
the mirror's bytes in tests/test_gpu_tables_model.py."""
import ctypes as C

import numpy as np
import pytest

import tables_cases as TC
import tables_model as TM
from tables_model import P1, P2, P3, P5, P6, P7, P8, P9

HEADS = (256, 512, 1024)


@pytest.fixture(scope="module")
def mirror():
    return TM.load_mirror()


# ---- a. the restatements against the header ----------------------------------------------------------------------------------------------
def _header_kw(L, lo, hi, n_heads):
    out = np.zeros((len(lo), 10), np.uint32)
    lo32, hi32 = np.ascontiguousarray(lo, np.uint32), np.ascontiguousarray(hi, np.uint32)
    L.vtxt_kw_many(lo32.ctypes.data, hi32.ctypes.data, len(lo32), n_heads, out.ctypes.data)
    return out


@pytest.mark.parametrize("n_heads", HEADS)
def test_hash_and_codes_equal_the_headers(mirror, n_heads):
    rng = np.random.default_rng(n_heads)
    kmers = np.concatenate([TM._acgt_kmers(), rng.integers(0, 256, (100000, 6), dtype=np.uint8)])
    lo, hi = TM._lo_hi_rows(kmers)
    want = _header_kw(mirror, lo, hi, n_heads)
    h = TM.kw_mix(lo, hi)
    code = TM.kw_code(lo, hi)
    assert np.array_equal(h, want[:, 0]) and np.array_equal(TM.kw_bucket(h, np.uint64(n_heads - 1)), want[:, 1])
    assert np.array_equal(TM.kw_tag(h), want[:, 2]) and np.array_equal(code, want[:, 3])
    assert want[:, 2].max() == 14 and (want[:, 0] >> 28).max() == 15
    (wa, ba), (wb, bb), (wc, bc) = TM.t3_places(code)
    assert np.array_equal(np.stack([wa, ba, wb, bb, wc, bc], axis=1), want[:, 4:10])
    # the scalar path check_table walks with, and vtxt_kw itself
    one = np.zeros(4, np.uint32)
    for i in list(range(0, 4096, 97)) + list(range(4096, 4096 + 300)):
        k = kmers[i].tobytes()
        l, hh = TM.lo_hi(k)
        mirror.vtxt_kw(l, hh, n_heads, one.ctypes.data)
        m = TM.kw_mix(l, hh)
        assert [m, TM.kw_bucket(m, n_heads - 1), TM.kw_tag(m), TM.kw_code(l, hh)] == one.tolist() == want[i, :4].tolist()
        assert [x for p in TM.t3_places(int(one[3])) for x in p] == want[i, 4:10].tolist()


def test_layout_equals_the_headers(mirror):
    out = np.zeros(14, np.uint32)
    for n_heads in HEADS:
        for max_hap in list(range(1, 70)) + [127, 128, 129, 180, 200, 201, 255, 256, 257, 1542, 2399, 2400]:
            mirror.vtxt_tab_layout(max_hap, n_heads, out.ctypes.data)
            assert TM.Layout(max_hap, n_heads).as_header_list() == out.tolist(), (max_hap, n_heads)


# ---- b. the corpus holds what it claims ----------------------------------------------------------------------------------------------------
def _buckets(hap, n_heads=1024):
    b = {}
    for y in range(max(len(hap) - 5, 0)):
        lo, hi = TM.lo_hi(hap[y:y + 6])
        b.setdefault(TM.kw_bucket(TM.kw_mix(lo, hi), n_heads - 1), []).append(y)
    return b


def _haps(batch):
    arena = batch.hap_arena.tobytes()
    return [arena[int(L[o]):int(L[o]) + int(L[n])] for L in batch.loci for o, n in (("ref_off", "ref_len"), ("alt_off", "alt_len"))]


def test_every_family_at_both_depths_in_one_pass():
    for fam in TC.FAMILIES:
        got = TC.cases(fam)
        assert {TC.uses_t3(b) for _, b, _ in got} == {False, True}, fam
        for label, b, _ in got:
            assert TC.one_pass(b) and 0 < b.n_loci <= 300, label
            assert (b.records["read_len"] >= 16).all() and (b.loci["rec_count"] > 0).all(), label


def test_premises_lengths_and_long_batch():
    _, b, _ = TC.lengths(TC.SHALLOW)
    lens = set(b.loci["ref_len"].tolist()) | set(b.loci["alt_len"].tolist())
    assert lens == set(TC.LENGTHS) and (b.loci["ref_len"] != b.loci["alt_len"]).all()
    assert set(TC.LENGTHS) >= {0, 1, 5, 6, 7, 63 + 5, 64 + 5, 65 + 5, 128 + 5, 129 + 5, 255, 256, 257}
    _, b, _ = TC.long_batch(TC.DEEP)
    assert (np.maximum(b.loci["ref_len"], b.loci["alt_len"]) > 255).all()
    ref, alt = _haps(b)[-2:]
    assert len(ref) == len(alt) == TM.FAST_HAP_LEN == 2400 and alt == b"A" * 2400 and TM.n_ordered_pairs(ref) < 2400
    assert max(len(v) for v in _buckets(alt).values()) == 2395


def test_premises_one_bucket_many_entries():
    seen = set()
    for unit, c, hap in TC.repeat_haps():
        pos = TM.positions_of(hap)
        assert len(pos) == len(unit) and sorted(len(p) for p in pos.values()) == [c - 1] * (len(unit) - 1) + [c], (unit, c)
        pops = sorted(len(v) for v in _buckets(hap).values())
        assert pops == [c - 1] * (len(unit) - 1) + [c], (unit, c, pops)          # (no two k-mers of a unit share a bucket: a bucket = a k-mer)
        seen.add((len(unit), c))
    assert seen == {(u, c) for u in (1, 2, 3, 4, 6, 12) for c in (63, 64, 65, 128, 129)}
    assert set(_haps(TC.one_bucket(TC.SHALLOW)[1])) >= {h for _, _, h in TC.repeat_haps()}


def test_premises_twin_list_edges():
    haps = set(_haps(TC.twin_edges(TC.SHALLOW)[1]))
    for hap, n_pairs, tw0 in TC.TWIN_PREMISES:
        assert hap in haps and TM.n_ordered_pairs(hap) == n_pairs
        none = len(hap) > 256 or max(hap) >= 0x80 or n_pairs > TM.TW_MAX
        assert (tw0 is None) == none and (none or tw0 == n_pairs)
    assert sorted((len(h), n) for h, n, _ in TC.TWIN_PREMISES) == [(200, 2), (200, 2), (200, 60), (200, 60), (200, 62), (256, 60), (257, 2)]
    assert max(len(p) for p in TM.positions_of(TC.TWINS_60_TRIPLE).values()) == 3 and max(len(p) for p in TM.positions_of(TC.TWINS_60).values()) == 2
    assert TC.TWINS_2_7F.count(b"\x7f") == 1 and max(TC.TWINS_2_7F) == 0x7f
    assert [i for i in range(200) if TC.TWINS_2_7F[i] != TC.TWINS_2_80[i]] == [60] and TC.TWINS_2_80[60] == 0x80


def test_premises_tags_and_buckets():
    haps = set(_haps(TC.tags_and_buckets(TC.DEEP)[1]))
    assert {TC.SHARED_TAG, TC.SHARED_BUCKET, TC.SLOT_CROWD} <= haps
    # two distinct k-mers in one bucket
    assert any(len({TC.SHARED_BUCKET[y:y + 6] for y in ys}) > 1 for ys in _buckets(TC.SHARED_BUCKET).values())
    # ... that also share h >> 28
    k1, k2 = TC.SHARED_TAG_KMERS
    h1, h2 = (TM.kw_mix(*TM.lo_hi(k)) for k in (k1, k2))
    assert k1 != k2 and k1 in TC.SHARED_TAG and k2 in TC.SHARED_TAG
    assert TM.kw_bucket(h1, 1023) == TM.kw_bucket(h2, 1023) and h1 >> 28 == h2 >> 28
    # a k-mer whose top nibble is 15, alone in its bucket: the clamp of kw_tag decides its head word
    clamp = [ys for ys in _buckets(TC.SHARED_TAG).values() if len(ys) == 1 and TM.kw_mix(*TM.lo_hi(TC.SHARED_TAG[ys[0]:ys[0] + 6])) >> 28 == 15]
    assert clamp and TM.kw_tag(0xf0000000) == 14
    # every position of a round of 64 on ONE link slot, over three buckets
    b = _buckets(TC.SLOT_CROWD)
    nk = len(TC.SLOT_CROWD) - 5
    assert nk > 64 and len(b) == 3 and len({k & 127 for k in b}) == 1
    assert sorted(y for ys in b.values() for y in ys if y < 64) == list(range(64))


def test_premises_alphabet():
    haps = set(_haps(TC.alphabet(TC.SHALLOW)[1]))
    A = TC.ALPHABET
    assert set(A.values()) <= haps
    assert b"NNN" in A["N runs"] and b"N" * 14 in A["N runs"] and max(A["N runs"]) < 0x80
    assert any(c in b"acgt" for c in A["lower case"]) and all(c in A["IUPAC"] for c in b"RYKMSWBDHVN")
    for name, where in (("a byte >= 0x80 first", 0), ("a byte >= 0x80 in the middle", 90), ("a byte >= 0x80 last", 179)):
        assert [i for i, c in enumerate(A[name]) if c >= 0x80] == [where] and len(A[name]) == 180
    assert b"NNNNNNGGGGGG" in A["NNNNNN next to GGGGGG"]
    assert TM.kw_code(*TM.lo_hi(b"NNNNNN")) == TM.kw_code(*TM.lo_hi(b"GGGGGG")) == 4095


# ---- c. the mirror's tables pass the checker -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(TC.FAMILIES))
def test_mirror_tables_pass(mirror, family):
    """(The mirror builds no t3[] and its tables do not depend on the depth: one depth.)"""
    for label, batch, _ in TC.cases(family, depths=(TC.SHALLOW,)):
        for n_heads in HEADS:
            tables = TM.mirror_tables(mirror, batch, n_heads)
            n, _ = TM.check_tables(tables, batch, n_heads, False, "%s, mirror, %d heads" % (label, n_heads))
            assert n == 2 * batch.n_loci


def test_mirror_decides_the_corpus_like_the_oracle(mirror):
    """The corpus through the per-task logic on the mirror's tables (what band_diag_kernel runs on the device's): every score it decides is
    the oracle's.  Haplotypes of 0 - 7 bases, bytes >= 0x80 and 2 400-base chains included."""
    import os
    from oracle import oracle
    from vartrix_amd.abi import VtxBatch, default_config
    mirror.vtxt_fastcore_batch.argtypes = [C.POINTER(VtxBatch), C.c_uint32, C.c_void_p, C.c_void_p]
    mirror.vtxt_fastcore_batch.restype = C.c_int
    decided = 0
    for family in TC.FAMILIES:
        for label, batch, nb in TC.cases(family, depths=(TC.SHALLOW,)):
            st = batch.as_struct()
            sc, why = np.zeros(2 * batch.n_records, np.int32), np.zeros(2 * batch.n_records, np.uint32)
            assert mirror.vtxt_fastcore_batch(C.byref(st), 1024, sc.ctypes.data, why.ctypes.data) == 0
            r, a = oracle.batch_scores(batch, default_config(aligner="banded", n_barcodes=nb), threads=min(os.cpu_count() or 8, 16))
            want = np.empty(2 * batch.n_records, np.int32)
            want[0::2], want[1::2] = r, a
            bad = np.nonzero((sc >= 0) & (sc != want))[0]
            assert bad.size == 0, "%s: task %d decided at %d, oracle %d" % (label, bad[0], sc[bad[0]], want[bad[0]])
            decided += int((sc >= 0).sum())
    assert decided > 500


# ---- d. the checker can fail --------------------------------------------------------------------------------------------------------------------
ORDINARY = TC.rnd(4300, 230)
REPEAT = b"ACG" * 40 + TC.rnd(4301, 40)          # 120 bases of a unit of three, then unique sequence: repeated and unique k-mers, > 60 pairs
FEW_TWINS = TC.TWINS_60                           # for the twin-list corruptions: a table that has a list


def _table(mirror, hap, n_heads=256, t3=True):
    """A mirror-built table of one haplotype (256 buckets: an ordinary haplotype then has chains of several entries), with a model-built
    t3[] put in; (table, layout)."""
    from vartrix_amd.abi import PackedBatch
    import stress_batches as SB
    batch = SB.manual_batch([(hap, b"")], [[(0, 0, hap[:50])]], 4)
    tb = TM.mirror_tables(mirror, batch, n_heads)[:TM.Layout(len(hap), n_heads).stride].copy()
    lay = TM.Layout(len(hap), n_heads)
    if t3:
        codes = [TM.kw_code(*TM.lo_hi(hap[y:y + 6])) for y in range(len(hap) - 5)]
        tb[lay.t3:lay.t3 + TM.T3_BYTES] = TM.t3_model(codes).view(np.uint8)
    return tb, lay


def _check(tb, hap, lay):
    return TM.check_table(tb, hap, lay.max_hap, lay.n_heads, True)


def _chain_of(v, nk, min_len, hap=None, distinct=False):
    """The entries of a chain of at least min_len entries (distinct: holding two different k-mers)."""
    for raw in v.head.tolist():
        if raw == TM.HEAD_END:
            continue
        ys, y = [], raw & 0xfff
        while y != TM.HEAD_END:
            ys.append(y)
            y = int(v.ent[y] >> np.uint64(48))
        if len(ys) >= min_len and (not distinct or len({hap[y:y + 6] for y in ys}) > 1):
            return ys
    raise AssertionError("no such chain")


def _set_next(v, y, nxt):
    v.ent[y] = (v.ent[y] & np.uint64(0x0000ffffffffffff)) | (np.uint64(nxt) << np.uint64(48))


@pytest.mark.parametrize("which", ["ordinary", "repeat"])
def test_checker_rejects_single_corruptions(mirror, which):
    hap = ORDINARY if which == "ordinary" else REPEAT
    clean, lay = _table(mirror, hap)
    assert _check(clean, hap, lay) == []
    nk = len(hap) - 5
    pos = TM.positions_of(hap)
    found = {}

    def corrupt(name, want, edit):
        tb = clean.copy()
        edit(TM.View(tb, lay), tb)
        assert not np.array_equal(tb, clean), name
        found[name] = TM.check_table(tb, hap, lay.max_hap, lay.n_heads, True)
        assert found[name] == [want], (which, name, found[name])

    cv = TM.View(clean, lay)
    # chains: a link skipped (an entry's k-mer is then missed: in the repeat a chain of ONE k-mer, so nothing else can notice)
    chain = _chain_of(cv, nk, 3)
    corrupt("link skipped", P1, lambda v, tb: _set_next(v, chain[0], int(v.ent[chain[1]] >> np.uint64(48))))
    corrupt("link pointing back", P2, lambda v, tb: _set_next(v, chain[2], chain[0]))
    corrupt("next beyond nk", P2, lambda v, tb: _set_next(v, chain[-1], nk))
    # heads
    heads = cv.head.tolist()
    single = next(b for b, raw in enumerate(heads) if raw != TM.HEAD_END and raw >> 12 != TM.HEAD_MULTI)
    multi = next(b for b, raw in enumerate(heads) if raw != TM.HEAD_END and raw >> 12 == TM.HEAD_MULTI)
    empty = heads.index(TM.HEAD_END)
    mpos = heads[multi] & 0xfff
    mtag = TM.kw_tag(TM.kw_mix(*TM.lo_hi(hap[mpos:mpos + 6])))

    def to_multi(v, tb):
        v.head[single] = (heads[single] & 0xfff) | (TM.HEAD_MULTI << 12)

    def to_tag(v, tb):
        v.head[multi] = mpos | (mtag << 12)

    def zero_head(v, tb):
        v.head[empty] = 0

    corrupt("tag -> MULTI", P3, to_multi)
    corrupt("MULTI -> tag", P3, to_tag)
    corrupt("empty head 0x0000", P3, zero_head)
    # uniqueness
    rep_y = next(p[0] for p in pos.values() if len(p) > 1) if which == "repeat" else None
    uni_y = next(p[0] for p in pos.values() if len(p) == 1)

    def flip_uq(y):
        def f(v, tb):
            v.uq[TM.UQ_PAD_WORDS + (y >> 5)] ^= np.uint32(1 << (y & 31))
        return f

    def pad_bit(v, tb):
        v.uq[TM.UQ_PAD_WORDS - 1] |= np.uint32(1 << 31)

    def behind_nk(v, tb):
        v.uq[TM.UQ_PAD_WORDS + (nk >> 5)] |= np.uint32(1 << (nk & 31))

    def fb_flag(v, tb):
        v.fb[uni_y + 5] &= 0x7f

    if which == "repeat":
        corrupt("uq set on a repeated k-mer", P6, flip_uq(rep_y))
    corrupt("uq cleared on a unique k-mer", P6, flip_uq(uni_y))
    corrupt("a pad bit", P6, pad_bit)
    corrupt("a uq bit behind nk", P6, behind_nk)
    corrupt("fb flag cleared", P6, fb_flag)
    # pb
    code = TM.kw_code(*TM.lo_hi(hap[:6]))
    free = next(c for c in range(4096) if not (int(cv.pb[c >> 5]) >> (c & 31)) & 1)

    def pb_clear(v, tb):
        v.pb[code >> 5] &= np.uint32(~(1 << (code & 31)) & 0xffffffff)

    def pb_set(v, tb):
        v.pb[free >> 5] |= np.uint32(1 << (free & 31))

    corrupt("pb bit cleared", P7, pb_clear)
    corrupt("pb bit set", P7, pb_set)
    # t3: one bit of each set
    (wa, ba), (wb, bb), (wc, bc) = TM.t3_places(code)
    for name, w, b in (("t3 set 0", wa, ba), ("t3 set 1", wb, bb), ("t3 set 2", wc, bc)):
        def t3_clear(v, tb, w=w, b=b):
            assert (int(v.t3[w]) >> b) & 1
            v.t3[w] &= np.uint32(~(1 << b) & 0xffffffff)
        corrupt(name + " bit cleared", P9, t3_clear)
    # bytes

    def byte(v, tb):
        v.bytes[17] ^= 0x04

    corrupt("a haplotype byte", P5, byte)
    assert len(found) == (17 if which == "repeat" else 16)


def test_checker_rejects_twin_list_corruptions(mirror):
    hap = FEW_TWINS
    clean, lay = _table(mirror, hap)
    assert _check(clean, hap, lay) == [] and clean[lay.tw] == 60

    def corrupt(name, edit):
        tb = clean.copy()
        edit(tb[lay.tw:lay.tw + TM.TW_BYTES])
        assert _check(tb, hap, lay) == [P8], name

    def swap(tw):
        tw[8:10], tw[10:12] = tw[10:12].copy(), tw[8:10].copy()

    def drop(tw):
        tw[8 + 2 * 20:8 + 2 * 59] = tw[8 + 2 * 21:8 + 2 * 60].copy()
        tw[0] = 59

    def none(tw):
        tw[0] = TM.TW_NONE

    corrupt("two pairs swapped", swap)
    corrupt("a pair dropped, the count lowered", drop)
    corrupt("60 -> TW_NONE", none)
    # TW_NONE -> 60: a haplotype that must have no list (62 pairs) claiming one
    hap2 = TC.TWINS_62
    tb, lay2 = _table(mirror, hap2)
    assert _check(tb, hap2, lay2) == [] and tb[lay2.tw] == TM.TW_NONE
    tb[lay2.tw] = 60
    assert _check(tb, hap2, lay2) == [P8]
    # ... and the repeat of the other test, whose list a byte >= 0x80 takes away
    hap3 = TC.TWINS_2_80
    tb, lay3 = _table(mirror, hap3)
    assert _check(tb, hap3, lay3) == [] and tb[lay3.tw] == TM.TW_NONE
    tb[lay3.tw] = 2
    assert _check(tb, hap3, lay3) == [P8]
