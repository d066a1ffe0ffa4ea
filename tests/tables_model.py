"""An independent checker of the per-haplotype k-mer tables (vartrix_amd/csrc/vtx_fast_core.h: Tab; built on the device by
band_tables_kernel and round 3's band_tables_v1_kernel, on the host by build_table of tests/fastcore/fastcore_host.cpp).

Every certificate stage of the banded flavour decides scores on the premise that a table tells the truth about its haplotype.
check_table() takes ONE table as bytes and the haplotype's bytes and tests that premise property by property.  The expected
side of every property comes from the haplotype alone, by brute force: a dict from each 6-byte string to the sorted list of its
positions.  No builder's output is ever the expectation.  To find a bucket the checker needs the hash: kw_mix, kw_bucket, kw_tag,
kw_code and the t3 maps are restated here from the header's comments, and tests/test_tables_model.py ties them to the header's own
functions (vtxt_kw, vtxt_kw_many, vtxt_tab_layout of the host build).

Properties (nk = max(hn - 5, 0), the number of k-mers):
  P1 walk-complete   walk_bucket (this module's restatement of the header's: head word, tag test, ent[] compare, next) yields for every
                     k-mer of the haplotype exactly its positions, ASCENDING.  The order is part of the contract: the header's twin
                     list is "in (y, y') order" (vtx_fast_core.h, tab_tw_off's comment) and both device builders write a position's
                     twins in chain order ("the chains ascend": vtx_band.hip, build_twins_wave and band_tables_kernel; build_tables
                     inserts "descending y => ascending chains"); front_rest / probe_rows append a row's matches in walk order.
  P2 walk-sound      every chain is acyclic, every next is < nk or HEAD_END, the chains hold nk entries in all, and the walk of a k-mer
                     that is NOT in the haplotype yields nothing: all absent 6-mers over ACGT (up to 4 096) and 256 random byte strings.
  P3 heads           empty bucket: 0xffff; one entry: its kw_tag (never 15) and its position; two or more ENTRIES (one k-mer twice counts):
                     HEAD_MULTI and the smallest position.
  P4 entries         ent[y], y < nk: bytes 0-3 and 4-5 of the k-mer at y.
  P5 bytes           bytes[0:hn] is the haplotype, fb[y] & 0x7f == hap[y] & 0x7f.
  P6 uniqueness      uq bit y <=> the k-mer at y occurs once; fb[y] & 0x80 <=> y >= 5 and the k-mer at y - 5 occurs once; a haplotype with
                     a byte >= 0x80 has neither; the UQ_PAD_WORDS words in front and every bit from nk on are zero.
  P7 pb              the 4 096 bits are exactly {kw_code(k)} (bytes outside ACGT alias: that is part of the definition).
  P8 twins           tw[0] == TW_NONE <=> hn > 256, a byte >= 0x80, or more than TW_MAX ordered pairs; else the count, and from byte 8 all
                     pairs (y, y'), y != y', of equal k-mers in lexicographic order.
  P9 t3              (with_t3 only) all 512 words equal the three-set model.

What is reported.  check_table returns the names of the violated properties.  The chain properties lean on each other: a chain with a
cycle cannot be walked, and a walk from a wrong head word says nothing about the links.  So they are looked at in the order P2
(structure: next in range, acyclic) -> P3 -> P1 -> P2 (the count of entries and the absent k-mers), and a later one is looked at only
when the earlier ones hold.  The set of tables that pass is the same as with every property looked at on its own; only the NAME a
broken table is reported under is the first in that order.  P4 - P9 are always looked at.

Bytes the layout leaves undefined, which no property reads: the gaps between the arrays (behind head[], bytes[hn:] and fb[hn:] up to
their max_hap + 8, the alignment in front of uq[] and behind t3[]), ent[y] for y >= nk, tw[1:8], the pairs behind tw[8 + 2 * count]
(all of them when tw[0] == TW_NONE), and t3[] of a table built without it.  The consumers, as read for this module: diag_mask and
verify_diag load 8-byte words that reach up to 7 bytes past bytes[hn - 1] and mask them with the row range; walk_bucket and the
chain walks never index ent[] at or above nk unless a next or a head says so (P2, P3); twin_matches reads whole 8-byte groups of tw[]
and drops the pairs at or above the count; t3[] is read only by a kernel launched with the same per-batch switch that built it.
"""
import ctypes as C
import os
import subprocess

import numpy as np

K = 6
HEAD_END, HEAD_MULTI = 0xffff, 15
UQ_PAD_WORDS = 8
TW_MAX, TW_BYTES, TW_NONE = 60, 128, 0xff
T3_BYTES = 2048
FAST_HAP_LEN = 2400           # a locus with a longer haplotype is on the slow list: its two tables are those of empty haplotypes
HERE = os.path.dirname(os.path.abspath(__file__))

PROPS = ("P1 walk-complete", "P2 walk-sound", "P3 heads", "P4 entries", "P5 bytes", "P6 uniqueness", "P7 pb", "P8 twins", "P9 t3")
P1, P2, P3, P4, P5, P6, P7, P8, P9 = PROPS


# ---- the layout (vtx_fast_core.h: tab_bytes_off .. tab_stride) --------------------------------------------------------------------
def _table_layout(max_hap, n_heads):
    """vtx_fast_core.h: tab_bytes_off .. tab_stride."""
    bytes_off = max_hap * 8 + n_heads * 2
    fb_off = bytes_off + max_hap + 8
    uq_off = (fb_off + max_hap + 8 + 3) & ~3
    pb_off = uq_off + 4 * (8 + (max_hap + 31) // 32 + 8)
    return bytes_off, fb_off, uq_off, pb_off, (pb_off + 512 + 128 + 2048 + 15) & ~15        # (round 6: tw[128], the twin list, and t3[2048], the three-row sets, behind pb[])


def _uses_t3(batch):
    """vtx_band.hip, band_use_t3: t3[] is built for batches of at least 16 tasks (8 reads) per locus on average."""
    return (2 * batch.n_records) // max(batch.n_loci, 1) >= 16


def _defined_bytes(tables, batch, n_heads=1024):
    """The bytes of the tables that MEAN something (entries of existing k-mers, head words, haplotype and flag bytes, the two
    bitmaps), table by table; the gaps between them are whatever the LDS held."""
    nl = batch.n_loci
    stride = len(tables) // (2 * nl)
    longest = int(max(batch.loci["ref_len"].max(), batch.loci["alt_len"].max()))
    max_hap = next(m for m in range(longest, longest + 64) if _table_layout(m, n_heads)[4] == stride)
    bytes_off, fb_off, uq_off, pb_off, _ = _table_layout(max_hap, n_heads)
    out = []
    for t in range(2 * nl):
        tb = tables[t * stride:(t + 1) * stride]
        hn = int(batch.loci["alt_len" if t & 1 else "ref_len"][t >> 1])
        nk = max(hn - 5, 0)
        out += [tb[:8 * nk], tb[max_hap * 8:bytes_off], tb[bytes_off:bytes_off + hn], tb[fb_off:fb_off + hn], tb[uq_off:pb_off + 512]]
        tw = tb[pb_off + 512:pb_off + 640]
        out += [tw[:1], tw[8:8 + 2 * (0 if tw[0] == 0xff else int(tw[0]))]]          # the twin list: its length, its pairs
        if _uses_t3(batch):
            out += [tb[pb_off + 640:pb_off + 640 + 2048]]                             # the three-row sets
    return np.concatenate(out)


class Layout:
    """Byte offsets of one table's arrays."""

    def __init__(self, max_hap, n_heads):
        self.max_hap, self.n_heads = max_hap, n_heads
        self.ent = 0
        self.head = max_hap * 8
        self.bytes, self.fb, self.uq, self.pb, self.stride = _table_layout(max_hap, n_heads)
        self.uq_words = UQ_PAD_WORDS + (max_hap + 31) // 32 + 8
        self.tw = self.pb + 512
        self.t3 = self.tw + TW_BYTES

    def as_header_list(self):
        """In the order of vtxt_tab_layout (tests/fastcore/fastcore_host.cpp)."""
        return [self.bytes, self.fb, self.uq, self.pb, self.tw, self.t3, self.stride,
                UQ_PAD_WORDS, HEAD_END, HEAD_MULTI, TW_MAX, TW_BYTES, TW_NONE, T3_BYTES]


# ---- the hash and the codes, restated from the header's comments (ints or numpy uint64 arrays alike) -------------------------------
def kw_mix(lo, hi):
    """hash of a k-mer (bytes 0-3 in lo, bytes 4-5 in hi): one 32-bit multiply of lo ^ hi << 11 ^ hi >> 3."""
    return (((lo ^ (hi << 11) ^ (hi >> 3)) & 0xffffffff) * 0x9E3779B1) & 0xffffffff


def kw_bucket(h, head_mask):
    """bucket = bits 18.. of the product."""
    return (h >> 18) & head_mask


def kw_tag(h):
    """tag = the product's top 4 bits; 15 is HEAD_MULTI's, a k-mer that would carry it carries 14."""
    t = h >> 28
    return t - (t == HEAD_MULTI)


def kw_code(lo, hi):
    """12-bit code, two bits per byte ((b >> 1) & 3: A 0, C 1, T 2, G 3), byte i at bits 2 i."""
    c = 0
    for i in range(4):
        c = c | ((((lo >> (8 * i)) >> 1) & 3) << (2 * i))
    for i in range(2):
        c = c | ((((hi >> (8 * i)) >> 1) & 3) << (8 + 2 * i))
    return c


def t3_places(c):
    """(word, bit) of k-mer code c in t3[] for its three roles.  Eight read bases b0 .. b7 hold the k-mers of rows r, r + 1, r + 2,
    which share b2 .. b5; entry S = the 8-bit code of those four bases, two words: word 2 S bits 0-15 the (b0, b1) in front of S,
    bits 16-31 the (b1, b6) around it, word 2 S + 1 bits 0-15 the (b6, b7) behind it."""
    a = (2 * (c >> 4), c & 15)                                           # the k-mer is b0 .. b5: S = its bases 2-5, (b0, b1) = bases 0-1
    b = (2 * ((c >> 2) & 0xff), 16 + ((c & 3) | ((c >> 10) << 2)))       # b1 .. b6: S = bases 1-4, (b1, b6) = bases 0 and 5
    cc = (2 * (c & 0xff) + 1, c >> 8)                                    # b2 .. b7: S = bases 0-3, (b6, b7) = bases 4-5
    return a, b, cc


def lo_hi(kmer):
    return int.from_bytes(kmer[:4], "little"), int.from_bytes(kmer[4:6], "little")


def positions_of(hap):
    """The brute-force index every expectation comes from: 6-byte string -> ascending positions."""
    pos = {}
    for y in range(max(len(hap) - K + 1, 0)):
        pos.setdefault(hap[y:y + K], []).append(y)
    return pos


def ordered_pairs(pos, limit=None):
    """All (y, y'), y != y', of equal k-mers, lexicographic; None when there are more than `limit`."""
    total = sum(len(p) * (len(p) - 1) for p in pos.values())
    if limit is not None and total > limit:
        return None
    out = [(y, z) for p in pos.values() if len(p) > 1 for y in p for z in p if z != y]
    out.sort()
    return out


def n_ordered_pairs(hap):
    return sum(len(p) * (len(p) - 1) for p in positions_of(hap).values())


# ---- a table's arrays ------------------------------------------------------------------------------------------------------------
class View:
    def __init__(self, tb, lay):
        tb = np.ascontiguousarray(tb, np.uint8)
        assert len(tb) >= lay.stride, (len(tb), lay.stride)
        self.lay = lay
        self.ent = tb[:8 * lay.max_hap].view("<u8")
        self.head = tb[lay.head:lay.head + 2 * lay.n_heads].view("<u2")
        self.bytes = tb[lay.bytes:lay.bytes + lay.max_hap + 8]
        self.fb = tb[lay.fb:lay.fb + lay.max_hap + 8]
        self.uq = tb[lay.uq:lay.uq + 4 * lay.uq_words].view("<u4")
        self.pb = tb[lay.pb:lay.pb + 512].view("<u4")
        self.tw = tb[lay.tw:lay.tw + TW_BYTES]
        self.t3 = tb[lay.t3:lay.t3 + T3_BYTES].view("<u4")


def walk_bucket(ent, head, n_heads, kmer, limit):
    """vtx_fast_core.h, walk_bucket, on a table's own words (ent, head: lists of ints): the positions it yields for the 6 bytes `kmer`,
    in the order it yields them.  limit: entries a table may hold — a walk that takes more steps, or leaves the table, returns None."""
    lo, hi = lo_hi(kmer)
    h = kw_mix(lo, hi)
    raw = head[kw_bucket(h, n_heads - 1)]
    if raw == HEAD_END:
        return []
    tag = raw >> 12
    if tag != HEAD_MULTI and tag != kw_tag(h):
        return []
    out, yc, steps = [], raw & 0xfff, 0
    while yc != HEAD_END:
        if yc >= limit or steps >= limit:
            return None
        e = ent[yc]
        if (e & 0xffffffff) == lo and ((e >> 32) & 0xffff) == hi:
            out.append(yc)
        yc = e >> 48
        steps += 1
    return out


_ACGT_KMERS = None


def _acgt_kmers():
    """All 4 096 6-mers over ACGT: bytes (4096, 6), lo, hi."""
    global _ACGT_KMERS
    if _ACGT_KMERS is None:
        idx = np.arange(4096)
        b = np.frombuffer(b"ACGT", np.uint8)[(idx[:, None] >> (2 * np.arange(6)[None, :])) & 3]
        _ACGT_KMERS = b
    return _ACGT_KMERS


def _lo_hi_rows(b):
    b = b.astype(np.uint64)
    lo = b[:, 0] | (b[:, 1] << np.uint64(8)) | (b[:, 2] << np.uint64(16)) | (b[:, 3] << np.uint64(24))
    hi = b[:, 4] | (b[:, 5] << np.uint64(8))
    return lo, hi


def _absent_walks(v, ent, head, pos, nk, seed):
    """P2's absent part: True when the walk of every absent ACGT 6-mer and of 256 random absent byte strings yields nothing.  The head
    word and tag tests of walk_bucket for all of them at once; the few that pass them are walked one by one."""
    rng = np.random.default_rng(seed)
    cand = np.concatenate([_acgt_kmers(), rng.integers(0, 256, (256, 6), dtype=np.uint8)])
    lo, hi = _lo_hi_rows(cand)
    h = kw_mix(lo, hi)
    raw = v.head[kw_bucket(h, np.uint64(v.lay.n_heads - 1)).astype(np.int64)].astype(np.uint64)
    tag = raw >> np.uint64(12)
    go = (raw != HEAD_END) & ((tag == HEAD_MULTI) | (tag == kw_tag(h)))
    for i in np.nonzero(go)[0]:
        kmer = cand[i].tobytes()
        if kmer in pos:
            continue
        if walk_bucket(ent, head, v.lay.n_heads, kmer, nk) != []:
            return False
    return True


def t3_model(codes):
    """The three sets of every entry from the haplotype's k-mer codes."""
    t3 = np.zeros(512, np.uint32)
    for c in sorted(set(int(c) for c in codes)):
        for w, b in t3_places(c):
            t3[w] |= np.uint32(1 << b)
    return t3


def check_table(tb, hap, max_hap, n_heads, with_t3, absent=True, seed=0, detail=None):
    """The violated properties of one table (names of PROPS; [] = the table tells the truth about `hap`).  absent=False leaves P2's walks
    of absent k-mers out (the callers' sample of the long tables).  detail: a list that receives one line per finding, the ones
    the order of the chain properties keeps out of the result included."""
    hap = bytes(hap)
    hn = len(hap)
    nk = max(hn - K + 1, 0)
    lay = Layout(max_hap, n_heads)
    v = View(tb, lay)
    bad = []

    def fail(prop, msg, report=True):
        if report and prop not in bad:
            bad.append(prop)
        if detail is not None:
            detail.append("%s: %s" % (prop, msg))

    pos = positions_of(hap)
    hb = np.frombuffer(hap, np.uint8)
    hib = bool((hb >= 0x80).any())
    ent, head = v.ent.tolist(), v.head.tolist()
    ky = [hap[y:y + K] for y in range(nk)]
    lohi = [lo_hi(k) for k in ky]
    hashes = [kw_mix(lo, hi) for lo, hi in lohi]

    # P4
    for y in range(nk):
        if (ent[y] & 0xffffffff) != lohi[y][0] or ((ent[y] >> 32) & 0xffff) != lohi[y][1]:
            fail(P4, "ent[%d] does not hold the k-mer at %d" % (y, y))
            break
    # P5
    if not np.array_equal(v.bytes[:hn], hb):
        fail(P5, "bytes[] differs from the haplotype at %d" % int(np.nonzero(v.bytes[:hn] != hb)[0][0]))
    if not np.array_equal(v.fb[:hn] & 0x7f, hb & 0x7f):
        fail(P5, "fb[] & 0x7f differs from the haplotype at %d" % int(np.nonzero((v.fb[:hn] & 0x7f) != (hb & 0x7f))[0][0]))
    # P6
    once = np.array([len(pos[k]) == 1 for k in ky], bool) & (not hib)
    bits = np.unpackbits(v.uq.view(np.uint8), bitorder="little")
    if bits[:32 * UQ_PAD_WORDS].any():
        fail(P6, "a bit in the pad words in front of uq[]")
    ub = bits[32 * UQ_PAD_WORDS:]
    if not np.array_equal(ub[:nk].astype(bool), once):
        y = int(np.nonzero(ub[:nk].astype(bool) != once)[0][0])
        fail(P6, "uq bit %d is %d, the k-mer occurs %d times%s" % (y, ub[y], len(pos[ky[y]]), " (a byte >= 0x80: no flags)" if hib else ""))
    if ub[nk:].any():
        fail(P6, "uq bit %d set, at or behind nk = %d" % (nk + int(np.nonzero(ub[nk:])[0][0]), nk))
    want_fb = np.zeros(hn, bool)
    want_fb[K - 1:K - 1 + nk] = once
    if not np.array_equal((v.fb[:hn] & 0x80) != 0, want_fb):
        y = int(np.nonzero(((v.fb[:hn] & 0x80) != 0) != want_fb)[0][0])
        fail(P6, "fb[%d] & 0x80 is %d" % (y, int(v.fb[y]) >> 7))
    # P7
    codes = [kw_code(lo, hi) for lo, hi in lohi]
    want_pb = np.zeros(4096, np.uint8)
    want_pb[codes] = 1
    got_pb = np.unpackbits(v.pb.view(np.uint8), bitorder="little")
    if not np.array_equal(got_pb, want_pb):
        c = int(np.nonzero(got_pb != want_pb)[0][0])
        fail(P7, "pb bit %d is %d" % (c, got_pb[c]))
    # P8
    pairs = None if (hn > 256 or hib) else ordered_pairs(pos, TW_MAX)
    tw = v.tw
    if pairs is None:
        if tw[0] != TW_NONE:
            fail(P8, "tw[0] = %d, expected TW_NONE" % tw[0])
    elif tw[0] != len(pairs):
        fail(P8, "tw[0] = %d, the haplotype has %d ordered pairs" % (tw[0], len(pairs)))
    else:
        got = [(int(tw[8 + 2 * i]), int(tw[9 + 2 * i])) for i in range(len(pairs))]
        if got != pairs:
            fail(P8, "pairs %s, expected %s" % (got, pairs))
    # P9
    if with_t3:
        want_t3 = t3_model(codes)
        if not np.array_equal(v.t3, want_t3):
            w = int(np.nonzero(v.t3 != want_t3)[0][0])
            fail(P9, "t3 word %d is %#x, expected %#x" % (w, int(v.t3[w]), int(want_t3[w])))

    # ---- the chains: P2 (structure) -> P3 -> P1 -> P2 (count, absent k-mers) ----
    nxt = np.array([e >> 48 for e in ent[:nk]], np.int64)
    ok = True
    if ((nxt >= nk) & (nxt != HEAD_END)).any():
        y = int(np.nonzero((nxt >= nk) & (nxt != HEAD_END))[0][0])
        fail(P2, "next of entry %d is %d: neither below nk = %d nor HEAD_END" % (y, nxt[y], nk))
        ok = False
    else:
        # acyclic: with HEAD_END as a sink every entry must reach it; pointer doubling
        jump = np.append(np.where(nxt == HEAD_END, nk, nxt), nk)
        for _ in range(max(nk, 1).bit_length() + 1):
            jump = jump[jump]
        if (jump != nk).any():
            fail(P2, "a chain with a cycle through entry %d" % int(np.nonzero(jump != nk)[0][0]))
            ok = False
    # P3
    buckets = {}
    for y in range(nk):
        buckets.setdefault(kw_bucket(hashes[y], n_heads - 1), []).append(y)
    heads_ok = True
    for b in range(n_heads):
        raw, ys = head[b], buckets.get(b)
        if ys is None:
            want = HEAD_END
        elif len(ys) == 1:
            want = ys[0] | (kw_tag(hashes[ys[0]]) << 12)
            assert kw_tag(hashes[ys[0]]) != HEAD_MULTI
        else:
            want = ys[0] | (HEAD_MULTI << 12)
        if raw != want:
            fail(P3, "head[%d] = %#06x, expected %#06x (%d entries)" % (b, raw, want, len(ys or [])), report=ok)
            heads_ok = False
            break
    # P1
    walks_ok = True
    if ok:
        for kmer, want in pos.items():
            got = walk_bucket(ent, head, n_heads, kmer, nk)
            if got != want:
                fail(P1, "the walk of the k-mer at %d yields %s, it sits at %s" % (want[0], got if got is None or len(got) < 12 else got[:12] + ["..."],
                                                                                  want if len(want) < 12 else want[:12] + ["..."]), report=heads_ok)
                walks_ok = False
                break
    # P2: the count, the absent k-mers
    if ok:
        total = 0
        for b in range(n_heads):
            if head[b] == HEAD_END:
                continue
            yc = head[b] & 0xfff
            while yc != HEAD_END and yc < nk and total <= 2 * nk + n_heads:
                total += 1
                yc = ent[yc] >> 48
        if total != nk:
            fail(P2, "the chains hold %d entries, the haplotype has %d k-mers" % (total, nk), report=heads_ok and walks_ok)
        if absent and not _absent_walks(v, ent, head, pos, nk, seed):
            fail(P2, "the walk of a k-mer that is not in the haplotype yields a position", report=heads_ok and walks_ok)
    return bad


# ---- batches ----------------------------------------------------------------------------------------------------------------------
def batch_max_hap(batch):
    """The table size of a batch's one banded pass: its longest haplotype within the fast kernels' limit (vtx_api.hip: max_hap_len)."""
    hl = np.maximum(batch.loci["ref_len"], batch.loci["alt_len"]).astype(np.int64)
    hl = hl[hl <= FAST_HAP_LEN]
    return int(hl.max()) if len(hl) else 0


def batch_haps(batch):
    """The haplotype of every table, 2 * locus + hap; a locus of the slow list has two empty ones."""
    arena = batch.hap_arena.tobytes()
    out = []
    for L in batch.loci:
        slow = max(int(L["ref_len"]), int(L["alt_len"])) > FAST_HAP_LEN
        for off, ln in ((int(L["ref_off"]), int(L["ref_len"])), (int(L["alt_off"]), int(L["alt_len"]))):
            out.append(b"" if slow else arena[off:off + ln])
    return out


def split(tables, batch, n_heads, with_t3):
    """[(table bytes, haplotype bytes)] of a dump of every table of the batch (vtx_debug_tables after a one-pass run, or
    mirror_tables); the stride must be the header's for the batch's longest haplotype."""
    lay = Layout(batch_max_hap(batch), n_heads)
    haps = batch_haps(batch)
    assert len(tables) == len(haps) * lay.stride, "%d bytes for %d tables of stride %d (t3 %s)" % (len(tables), len(haps), lay.stride, with_t3)
    return [(tables[t * lay.stride:(t + 1) * lay.stride], haps[t]) for t in range(len(haps))]


def defined_without_t3(tb, hn, lay):
    """One table's defined bytes but t3[]: what a device table and the mirror's must share byte for byte."""
    nk = max(hn - K + 1, 0)
    tw = tb[lay.tw:lay.tw + TW_BYTES]
    n_pairs = 0 if tw[0] == TW_NONE else int(tw[0])
    return np.concatenate([tb[:8 * nk], tb[lay.head:lay.bytes], tb[lay.bytes:lay.bytes + hn], tb[lay.fb:lay.fb + hn], tb[lay.uq:lay.pb + 512],
                           tw[:1], tw[8:8 + 2 * min(n_pairs, TW_MAX)]])


def check_tables(tables, batch, n_heads, with_t3, label, long_sample=16, mirror=None):
    """Every table of a dump through check_table (the absent-k-mer walks on every table of at most 400 bases and on `long_sample` of
    the longer ones) and, with `mirror` (mirror_tables of the same batch), against the mirror's defined bytes.  Returns (tables
    checked, tables compared with the mirror); raises on the first table that fails."""
    parts = split(tables, batch, n_heads, with_t3)
    lay = Layout(batch_max_hap(batch), n_heads)
    long_ones = [t for t, (_, hap) in enumerate(parts) if len(hap) > 400]
    step = max(1, len(long_ones) // long_sample)
    sampled = set(long_ones[::step][:long_sample])
    mparts = split(mirror, batch, n_heads, False) if mirror is not None else None
    compared = 0
    for t, (tb, hap) in enumerate(parts):
        detail = []
        bad = check_table(tb, hap, lay.max_hap, n_heads, with_t3, absent=len(hap) <= 400 or t in sampled, seed=t, detail=detail)
        assert not bad, "%s: table %d (%d bases): %s\n%s" % (label, t, len(hap), bad, "\n".join(detail))
        if mparts is not None:
            a, b = defined_without_t3(tb, len(hap), lay), defined_without_t3(mparts[t][0], len(hap), lay)
            assert len(a) == len(b) and np.array_equal(a, b), "%s: table %d (%d bases) differs from the mirror's in %d defined bytes" % (
                label, t, len(hap), int((a != b).sum()) if len(a) == len(b) else -1)
            compared += 1
    return len(parts), compared


# ---- the mirror (tests/fastcore/fastcore_host.cpp) ----------------------------------------------------------------------------------
def load_mirror():
    from vartrix_amd.abi import VtxBatch
    subprocess.check_call(["make", "-C", os.path.join(HERE, "fastcore"), "-s"])
    L = C.CDLL(os.path.join(HERE, "fastcore", "libfastcore_host.so"))
    L.vtxt_build_tables.argtypes = [C.POINTER(VtxBatch), C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64]
    L.vtxt_build_tables.restype = C.c_int
    L.vtxt_kw.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.vtxt_kw.restype = None
    L.vtxt_kw_many.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.vtxt_kw_many.restype = None
    L.vtxt_tab_layout.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
    L.vtxt_tab_layout.restype = None
    return L


def mirror_tables(L, batch, n_heads):
    """build_table's tables of every locus of the batch, laid out like a device dump (no t3[]).  A locus of the slow list gets empty
    haplotypes, as on the device."""
    from vartrix_amd.abi import PackedBatch
    lay = Layout(batch_max_hap(batch), n_heads)
    loci = batch.loci.copy()
    slow = np.maximum(loci["ref_len"], loci["alt_len"]) > FAST_HAP_LEN
    loci["ref_len"][slow] = 0
    loci["alt_len"][slow] = 0
    b = PackedBatch(loci, batch.records, batch.hap_arena, batch.read_arena)
    st = b.as_struct()
    out = np.zeros(2 * b.n_loci * lay.stride + 64, np.uint8)
    rc = L.vtxt_build_tables(C.byref(st), n_heads, lay.max_hap, out.ctypes.data, lay.stride)
    assert rc == 0, rc
    return out[:2 * b.n_loci * lay.stride]
