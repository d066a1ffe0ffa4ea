"""CPU unit tests of vartrix_amd/csrc/vtx_ingest_plan_core.h — the host half of vtx_submit_bam / vtx_submit_bam_segments: the checks of a
caller's plan (the API's guard in front of kernels that trust the plan) and its rewrite into the device's layout — compiled for the host
by tests/ingestplancore/Makefile.

  * The planner's plans are the device's plans: what libvtxhost's vtxh_plan_ingest hands out (contiguous and segmented, .bai and .csi) is
    accepted, and the layout equals a model written here from the wording of include/vtx.h.
  * Every reject: one defect per case on an otherwise valid plan, the exact status and the message.  REJECTS has a row (or several: one
    per sub-condition) for each of the 13 `fail(...)` of the plan checks in the function these moved out of (submit_bam_impl, which had 21:
    the barcode-list state in front of them, and behind them the device's verdicts — five in ingest_error, the 2^32 records, the batch
    limits — stay in vtx_api.hip and with tests/test_gpu_ingest*.py, tests/test_gpu_crc32.py).  Two-defect plans pin the order of the checks.
  * Edges: the trailer at the very end of the file, ISIZE 65536 / 65537, offsets near 2^64 and spans across the int32 range (rejected,
    not wrapped), empty plans, a segment that ends on its last byte.
  * What the checks touch: every case of the tables again through a stand-alone program (tests/ingestplancore/main.cpp) whose arrays are
    heap allocations of exactly the stated sizes, plain and under AddressSanitizer and UBSan; nothing sanitized is loaded into Python."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from vartrix_amd import abi, hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)

DEV_BLOCK = np.dtype([("coff", "<u8"), ("uoff", "<u8"), ("clen", "<u4"), ("isize", "<u4")])
DEV_SEGMENT = np.dtype([("ubegin", "<u8"), ("ulimit", "<u8"), ("end_upos", "<u8"), ("seed_end", "<u4"), ("end_tid", "<i4"), ("end_pos", "<i4"),
                        ("flags", "<u4")])
PIECE = np.dtype([("file_off", "<u8"), ("dst_off", "<u8"), ("bytes", "<u8")])
FIGURES = ("n_blocks", "n_segs", "n_seed_seg", "n_pieces", "n_iv", "lo", "hi", "utotal", "comp_bytes", "end_upos")
ARRAYS = (("blocks", DEV_BLOCK, "n_blocks"), ("segs", DEV_SEGMENT, "n_segs"), ("seed_seg", np.dtype("<u4"), "n_seed_seg"), ("pieces", PIECE, "n_pieces"),
          ("iv", np.dtype("<u4"), "n_iv"))
OK, E_INVAL, E_UNSUPPORTED = abi.VTX_OK, abi.VTX_E_INVAL, abi.VTX_E_UNSUPPORTED
TRAILER = 8
U64 = 1 << 64


@pytest.fixture(scope="module")
def core():
    return load_core()


def load_core():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "ingestplancore"), "-s"])
    lib = C.CDLL(os.path.join(HERE, "ingestplancore", "libingestplan_host.so"))
    lib.ipc_plan.restype = C.c_void_p
    lib.ipc_plan.argtypes = [C.c_void_p, C.c_void_p]
    lib.ipc_status.argtypes = lib.ipc_why.argtypes = lib.ipc_free.argtypes = [C.c_void_p]
    lib.ipc_why.restype = C.c_char_p
    lib.ipc_figures.argtypes = [C.c_void_p, C.c_void_p]
    lib.ipc_array.restype = C.c_void_p
    lib.ipc_array.argtypes = [C.c_void_p, C.c_int]
    sizes = (C.c_uint32 * 3)()
    lib.ipc_sizes(sizes)
    assert list(sizes) == [DEV_BLOCK.itemsize, DEV_SEGMENT.itemsize, PIECE.itemsize] == [24, 40, 24]
    return lib


def run_core(core, g, sg=None):
    """-> (status, message, layout): layout = the figures, the five arrays and the interval sub-arrays as the accessors give them."""
    h = core.ipc_plan(C.byref(g) if g is not None else None, C.byref(sg) if sg is not None else None)
    try:
        status, why = core.ipc_status(h), core.ipc_why(h).decode()
        if status != OK:
            return status, why, None
        fig = (C.c_uint64 * 10)()
        core.ipc_figures(h, fig)
        lay = dict(zip(FIGURES, (int(v) for v in fig)))

        def arr(which, n, dt):
            return np.frombuffer(C.string_at(core.ipc_array(h, which), n * dt.itemsize), dtype=dt).copy() if n else np.zeros(0, dt)
        for k, (name, dt, count) in enumerate(ARRAYS):
            lay[name] = arr(k, lay[count], dt)
        base = sg.base if sg is not None else g
        ni, nref = int(base.n_intervals), int(base.n_ref)
        for k, (name, dt, n) in enumerate((("iv_start", "<i4", ni), ("iv_end", "<i4", ni), ("iv_locus", "<u4", ni), ("tid_begin", "<u4", nref + 1),
                                           ("tid_span", "<i4", nref))):
            lay[name] = arr(5 + k, n, np.dtype(dt))
        return status, why, lay
    finally:
        core.ipc_free(h)


def model(a, segments=None):
    """The device's layout of a plan, from the wording of include/vtx.h.  a: the plan's arrays (IngestPlan.arrays()'s names)."""
    blocks, iv = a["blocks"], a["intervals"]
    nb = len(blocks)
    coff, clen, isize = (blocks[k].astype(np.uint64) for k in ("coff", "clen", "isize"))
    want = dict(n_blocks=nb, utotal=int(isize.sum()), lo=int(coff[0]) if nb else 0, hi=int(coff[-1] + clen[-1]) if nb else 0)
    dev = np.zeros(nb, DEV_BLOCK)
    dev["clen"], dev["isize"] = blocks["clen"], blocks["isize"]
    dev["uoff"] = np.concatenate([[0], np.cumsum(isize)[:-1]]) if nb else []          # the inflated stream: the blocks' bytes back to back
    if segments is None:
        # "[blocks[0].coff, blocks[n - 1].coff + clen + 8): the blocks' payloads and the trailer behind each" travel as they are
        dev["coff"] = coff - np.uint64(want["lo"])
        want.update(comp_bytes=want["hi"] - want["lo"] + TRAILER if nb else 0, end_upos=min(int(a["end_upos"]), want["utotal"]),
                    n_segs=0, n_pieces=0, n_seed_seg=0)
    else:
        # "only those byte ranges travel, into one compact device buffer"; seeds and ends are offsets into the CONCATENATION of the
        # segments' inflated bytes; segment k owns blocks [block_begin, block_end) and seeds [seed_begin, seed_end)
        segs, pieces, seed_seg = np.zeros(len(segments), DEV_SEGMENT), np.zeros(len(segments), PIECE), np.zeros(len(a["seeds"]), "<u4")
        cb = ub = 0
        for k, S in enumerate(segments):
            b0, b1 = int(S["block_begin"]), int(S["block_end"])
            first, end = int(coff[b0]), int(coff[b1 - 1] + clen[b1 - 1]) + TRAILER
            dev["coff"][b0:b1] = np.uint64(cb) + (coff[b0:b1] - np.uint64(first))
            ul = ub + int(isize[b0:b1].sum())
            segs[k] = (ub, ul, S["end_upos"], S["seed_end"], S["end_tid"], S["end_pos"], S["flags"])
            pieces[k] = (first, cb, end - first)
            seed_seg[int(S["seed_begin"]):int(S["seed_end"])] = k
            cb, ub = cb + end - first, ul
        want.update(comp_bytes=cb, segs=segs, pieces=pieces, seed_seg=seed_seg, n_segs=len(segs), n_pieces=len(segs), n_seed_seg=len(seed_seg))
    want.update(blocks=dev, iv_start=iv["start"], iv_end=iv["end"], iv_locus=iv["locus"], tid_begin=a["tid_begin"], tid_span=a["tid_max_span"],
                iv=np.concatenate([np.ascontiguousarray(x).view("<u4") for x in (iv["start"], iv["end"], iv["locus"], a["tid_begin"], a["tid_max_span"])]))
    return want


def assert_layout(lay, want, where=""):
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert lay[k].dtype == v.dtype and np.array_equal(lay[k], v), "%s: %s" % (where, k)
        else:
            assert lay[k] == v, "%s: %s: %r, model %r" % (where, k, lay[k], v)
    # the pieces tile [0, comp_bytes) back to back
    p = lay["pieces"]
    if len(p):
        assert int(p["dst_off"][0]) == 0 and np.array_equal(p["dst_off"][1:], (p["dst_off"] + p["bytes"])[:-1]), where
        assert int(p["dst_off"][-1] + p["bytes"][-1]) == lay["comp_bytes"], where


# ---- the planner's plans ----------------------------------------------------------------------------------------------------------

def check_planned(core, inputs, want_kind, **kw):
    with hostlib.plan_ingest(**inputs, **kw) as plan:
        assert plan.reason is None, plan.reason
        assert plan.kind == want_kind
        a = plan.arrays()
        status, why, lay = run_core(core, plan.ingest if plan.segments is None else None, plan.segments)
    assert status == OK, why
    assert_layout(lay, model(a, a.get("segments")), "%s %r" % (want_kind, kw))
    return lay


def test_contiguous_plans_of_the_planner_are_the_devices(core, tmp_path):
    """The inputs of tests/test_ingest_plan.py: the reference fixture, and the authored BAM over the golden test_dna.* with BGZF blocks of
    20 000 / 3 000 / 700 bytes, whole and in ranges of rows."""
    from test_host import make_dna_bam
    lay = check_planned(core, dict(vcf=os.path.join(G, "test.vcf"), bam=os.path.join(G, "test.bam"), fasta=os.path.join(G, "test.fa"),
                                   cell_barcodes=os.path.join(G, "barcodes.tsv")), "contiguous")
    assert lay["n_blocks"] > 1 and lay["n_iv"] > 4
    for block in (20000, 3000, 700):
        bam = make_dna_bam(tmp_path, seed=4, n_reads=3000, block=block)
        inputs = dict(vcf=os.path.join(G, "test_dna.vcf"), bam=bam, fasta=os.path.join(G, "test_dna.fa"), cell_barcodes=os.path.join(G, "dna_barcodes.tsv"))
        check_planned(core, inputs, "contiguous")
        for rows in ((0, 10), (10, 30), (30, 46)):
            check_planned(core, inputs, "contiguous", rows=rows)


@pytest.fixture()
def sparse_planner(monkeypatch):
    # the planner's threshold knob exists in the developer build of the host library only
    import segments_util as su
    hostlib.use_variant("dev")
    monkeypatch.setenv("VTXH_SPARSE_KIB", su.SPARSE_KIB)
    yield su
    hostlib.use_variant("dev" if os.environ.get("VTX_LIB_VARIANT") == "dev" else "")


def test_segmented_plans_of_the_planner_are_the_devices(core, tmp_path, sparse_planner):
    """The CASES of tests/test_ingest_plan_segments.py (sparse loci; blocks of 700 / 4 000 / 20 000 bytes; .bai and .csi)."""
    from test_ingest_plan_segments import CASES
    for block, index in CASES:
        inputs = sparse_planner.author(tmp_path, block=block, index=index)
        lay = check_planned(core, inputs, "segmented", use_umi=True)
        assert lay["n_segs"] >= 3 and lay["n_pieces"] == lay["n_segs"] and lay["comp_bytes"] < lay["hi"] - lay["lo"]


# ---- authored plans ---------------------------------------------------------------------------------------------------------------

class Plan:
    """A plan as arrays; ctypes() and encode() hand it to the shared object and to the stand-alone program.  nulls: names of the pointers
    to hand over as NULL whatever the counts say."""
    NULL_BITS = ("file", "blocks", "seeds", "intervals", "tid_begin", "tid_max_span", "loci", "hap_arena", "segments")

    def __init__(self, **kw):
        self.file_bytes, self.end_upos, self.hap_bytes, self.n_loci, self.nulls, self.segments = 0, 0, 4, 0, (), None
        self.blocks, self.seeds, self.intervals, self.tid_begin, self.tid_max_span = [], [], [], [0], []
        self.__dict__.update(kw)

    def but(self, **kw):
        return Plan(**dict(self.__dict__, **kw))

    def arrays(self):
        a = dict(blocks=np.array([tuple(b) for b in self.blocks], abi.BGZF_BLOCK_DTYPE), seeds=np.array([s % U64 for s in self.seeds], np.uint64),
                 intervals=np.array([tuple(i) + (0,) for i in self.intervals], abi.BAM_INTERVAL_DTYPE), tid_begin=np.array(self.tid_begin, np.uint32),
                 tid_max_span=np.array(self.tid_max_span, np.int32), end_upos=self.end_upos)
        if self.segments is not None:
            a["segments"] = np.array([tuple(s) + (0,) for s in self.segments], abi.BAM_SEGMENT_DTYPE)
        return {k: (v.reshape(-1) if isinstance(v, np.ndarray) else v) for k, v in a.items()}

    def ctypes(self):
        """-> (g or None, sg or None, what must stay alive)"""
        a = self.arrays()
        a["loci"], a["file"], a["hap_arena"] = np.zeros(self.n_loci, abi.LOCUS_DTYPE), np.zeros(1, np.uint8), np.zeros(1, np.uint8)
        sg = abi.VtxBamSegments()
        g = sg.base

        def ptr(name):
            return None if name in self.nulls else a[name].ctypes.data
        g.file, g.file_bytes, g.blocks, g.n_blocks, g.n_ref = ptr("file"), self.file_bytes, ptr("blocks"), len(a["blocks"]), len(a["tid_max_span"])
        g.seeds, g.n_seeds, g.n_intervals, g.end_upos, g.intervals = ptr("seeds"), len(a["seeds"]), len(a["intervals"]), self.end_upos, ptr("intervals")
        g.tid_begin, g.tid_max_span, g.loci, g.n_loci = ptr("tid_begin"), ptr("tid_max_span"), ptr("loci"), self.n_loci
        g.hap_arena, g.hap_bytes, g.bam_tag = ptr("hap_arena"), self.hap_bytes, b"CB"
        if self.segments is None:
            return g, None, (a, sg)
        sg.segments, sg.n_segments = ptr("segments"), len(a["segments"])
        return None, sg, (a, sg)

    def encode(self):
        a = self.arrays()
        seg = a.get("segments", np.zeros(0, abi.BAM_SEGMENT_DTYPE))
        assert len(a["tid_begin"]) == len(a["tid_max_span"]) + 1
        mask = sum(1 << self.NULL_BITS.index(n) for n in self.nulls)
        head = struct.pack("<9I3Q", int(self.segments is not None), len(a["blocks"]), len(a["tid_max_span"]), len(a["seeds"]), len(a["intervals"]),
                           self.n_loci, len(seg), mask, 0, self.file_bytes, self.end_upos, self.hap_bytes)
        return head + b"".join(a[k].tobytes() for k in ("blocks", "seeds", "intervals", "tid_begin", "tid_max_span")) + seg.tobytes()


# Three blocks — the middle one of the largest ISIZE there is, the last one with its trailer ending exactly at file_bytes —, two contigs,
# three loci, three seeds.  Segmented: blocks {0, 1} and {2}; the first segment ends exactly 12 bytes in front of its blocks' end, the
# second (to the end of the file's records) on its last byte.
FILE_BYTES = 1000
BLOCKS = [(18, 100, 300), (144, 50, 65536), (220, FILE_BYTES - TRAILER - 220, 10)]
UTOTAL = 300 + 65536 + 10
CONTIG = Plan(file_bytes=FILE_BYTES, blocks=BLOCKS, seeds=[0, 400, 65000], end_upos=UTOTAL, n_loci=3, tid_begin=[0, 2, 3], tid_max_span=[50, 10],
              intervals=[(10, 60, 0), (10, 20, 1), (5, 15, 2)])
SEGS = [(0, 2, 0, 2, 65836 - 12, 0, 60, 0), (2, 3, 2, 3, UTOTAL, 1, 15, abi.SEGMENT_TO_EOF)]
SEGMENTED = CONTIG.but(seeds=[0, 400, 65840], end_upos=0, segments=SEGS)
SORTED = [(10, 60, 0), (10, 20, 1), (12, 15, 2)]                        # CONTIG's intervals, in order even when read as ONE contig's


def blocks_but(i, **kw):
    b = [dict(zip(("coff", "clen", "isize"), x)) for x in BLOCKS]
    b[i].update(kw)
    return [(x["coff"], x["clen"], x["isize"]) for x in b]


def segs_but(k, **kw):
    names = ("block_begin", "block_end", "seed_begin", "seed_end", "end_upos", "end_tid", "end_pos", "flags")
    s = [dict(zip(names, x)) for x in SEGS]
    s[k].update(kw)
    return [tuple(x[n] for n in names) for x in s]


ACCEPTS = {
    "contiguous": CONTIG,
    "segmented: an end 12 bytes in front of its blocks' end, a TO_EOF end on the last byte": SEGMENTED,
    "isize 65536 (the middle block) and a trailer that ends exactly at file_bytes (the last)": CONTIG,
    "end_upos beyond the stream is clamped": CONTIG.but(end_upos=U64 - 1),
    "no blocks, no seeds, no loci, no intervals": Plan(tid_begin=[0, 0], tid_max_span=[0], hap_bytes=0, nulls=("file", "blocks", "seeds", "intervals", "loci", "hap_arena")),
    "n_ref = 0": Plan(tid_begin=[0], nulls=("tid_max_span",)),
    "n_ref = 0, segmented, no segments": Plan(tid_begin=[0], segments=[], nulls=("tid_max_span", "segments")),
    "an interval as long as its contig's span, int32 end to end": CONTIG.but(intervals=[(-2**31, -2**31 + 50, 0), (10, 20, 1), (5, 15, 2)]),
    "a contig without intervals": CONTIG.but(tid_begin=[0, 3, 3], tid_max_span=[50, 0], intervals=SORTED),
}

NULL = "vtx_submit_bam: null array with non-zero count"
BLOCK = "vtx_submit_bam: block %d: out of order, outside the file or above 64 KiB"
TRAIL = "vtx_submit_bam: BGZF block %d: its trailer (CRC32, ISIZE) lies beyond the end of the file: the host packer decides"
IVAL = "vtx_submit_bam: interval %d: bad locus / order / span"
SEG = "vtx_submit_bam_segments: segment %d: its blocks / seeds do not follow the segment before, or are empty"
SEG_END = "vtx_submit_bam_segments: segment %d: its end (and the 12 bytes of the record there) lies outside its blocks"
SEED_SEG = "vtx_submit_bam_segments: seed %d: not ascending or outside segment %d"
SEED = "vtx_submit_bam: seed %d: not ascending or beyond the end"
BEHIND = "vtx_submit_bam_segments: blocks or seeds behind the last segment"

# name -> (plan, status, the whole message).  In the order of the checks; the branch of the parent's function each row belongs to is the
# message's.  "one past": the defect is an index one past an array of the plan (the stand-alone program's allocations end there).
REJECTS = {
    # 1: null arrays (seven sub-conditions)
    "null blocks": (CONTIG.but(nulls=("blocks",)), E_INVAL, NULL),
    "null file": (CONTIG.but(nulls=("file",)), E_INVAL, NULL),
    "null loci": (CONTIG.but(nulls=("loci",)), E_INVAL, NULL),
    "null hap_arena": (CONTIG.but(nulls=("hap_arena",)), E_INVAL, NULL),
    "null seeds": (CONTIG.but(nulls=("seeds",)), E_INVAL, NULL),
    "null intervals": (CONTIG.but(nulls=("intervals",)), E_INVAL, NULL),
    "null tid_begin (even with n_ref = 0)": (Plan(nulls=("tid_begin",)), E_INVAL, NULL),
    "null tid_max_span": (CONTIG.but(nulls=("tid_max_span",)), E_INVAL, NULL),
    # 2: the hap arena
    "hap arena of 4 GiB": (CONTIG.but(hap_bytes=1 << 32), E_UNSUPPORTED, "vtx_submit_bam: hap arena above 4 GiB"),
    # 3, 4: tid_begin
    "tid_begin starts behind 0": (CONTIG.but(tid_begin=[1, 2, 3]), E_INVAL, "vtx_submit_bam: tid_begin does not cover the intervals"),
    "tid_begin ends short of the intervals": (CONTIG.but(tid_begin=[0, 2, 2]), E_INVAL, "vtx_submit_bam: tid_begin does not cover the intervals"),
    "tid_begin ends one past the intervals": (CONTIG.but(tid_begin=[0, 2, 4]), E_INVAL, "vtx_submit_bam: tid_begin does not cover the intervals"),
    "tid_begin descends (one past the intervals in between)": (CONTIG.but(tid_begin=[0, 4, 3], intervals=SORTED), E_INVAL, "vtx_submit_bam: tid_begin not ascending at 1"),
    "tid_begin far beyond the intervals in between": (CONTIG.but(tid_begin=[0, 2**32 - 1, 3], intervals=SORTED), E_INVAL, "vtx_submit_bam: tid_begin not ascending at 1"),
    # 5: intervals (four sub-conditions)
    "interval of locus n_loci (one past)": (CONTIG.but(intervals=[(10, 60, 0), (10, 20, 3), (5, 15, 2)]), E_INVAL, IVAL % 1),
    "interval that ends in front of its start": (CONTIG.but(intervals=[(10, 60, 0), (10, 9, 1), (5, 15, 2)]), E_INVAL, IVAL % 1),
    "intervals of a contig not sorted by start": (CONTIG.but(intervals=[(10, 60, 0), (9, 20, 1), (5, 15, 2)]), E_INVAL, IVAL % 1),
    "interval longer than its contig's span": (CONTIG.but(intervals=[(10, 60, 0), (10, 20, 1), (5, 16, 2)]), E_INVAL, IVAL % 2),
    "end - start across the int32 range (2^32 - 1: -1 as an int32)": (CONTIG.but(intervals=[(-2**31, 2**31 - 1, 0), (10, 20, 1), (5, 15, 2)]), E_INVAL, IVAL % 0),
    # 6: blocks (three sub-conditions)
    "block that overlaps the one before": (CONTIG.but(blocks=blocks_but(1, coff=117)), E_INVAL, BLOCK % 1),
    "block that starts beyond the file": (CONTIG.but(blocks=blocks_but(2, coff=FILE_BYTES + 1, clen=0)), E_INVAL, BLOCK % 2),
    "block that ends beyond the file": (CONTIG.but(blocks=blocks_but(2, clen=FILE_BYTES - 220 + 1)), E_INVAL, BLOCK % 2),
    "isize 65537": (CONTIG.but(blocks=blocks_but(1, isize=65537)), E_INVAL, BLOCK % 1),
    "coff = 2^64 - 1 with clen = 2: the sum wraps to 1": (CONTIG.but(blocks=[(U64 - 1, 2, 10)], seeds=[0], end_upos=10), E_INVAL, BLOCK % 0),
    "coff + clen + 8 wraps": (CONTIG.but(blocks=blocks_but(2, coff=U64 - 12, clen=4)), E_INVAL, BLOCK % 2),
    # 7: the trailer
    "file_bytes near 2^64: coff + clen + 8 wraps to 2": (CONTIG.but(file_bytes=U64 - 1, blocks=[(U64 - 10, 4, 10)], seeds=[0], end_upos=10), E_UNSUPPORTED, TRAIL % 0),
    "trailer one byte short": (CONTIG.but(file_bytes=FILE_BYTES - 1), E_UNSUPPORTED, TRAIL % 2),
    "payload up to the end of the file": (CONTIG.but(file_bytes=FILE_BYTES - TRAILER), E_UNSUPPORTED, TRAIL % 2),
    # 8: segments at all
    "null segments": (SEGMENTED.but(nulls=("segments",)), E_INVAL, "vtx_submit_bam_segments: blocks or seeds without segments"),
    "blocks without segments": (SEGMENTED.but(segments=[]), E_INVAL, "vtx_submit_bam_segments: blocks or seeds without segments"),
    "seeds without segments": (Plan(tid_begin=[0], seeds=[0], segments=[]), E_INVAL, "vtx_submit_bam_segments: blocks or seeds without segments"),
    # 9: the segment table tiles the blocks and the seeds (six sub-conditions)
    "segment that skips a block": (SEGMENTED.but(segments=segs_but(1, block_begin=3, block_end=4)), E_INVAL, SEG % 1),
    "segment without blocks": (SEGMENTED.but(segments=segs_but(0, block_end=0)), E_INVAL, SEG % 0),
    "segment with a block one past the blocks": (SEGMENTED.but(segments=segs_but(1, block_end=4)), E_INVAL, SEG % 1),
    "segment that skips a seed": (SEGMENTED.but(segments=segs_but(1, seed_begin=3, seed_end=4)), E_INVAL, SEG % 1),
    "segment without seeds": (SEGMENTED.but(segments=segs_but(0, seed_end=0)), E_INVAL, SEG % 0),
    "segment with a seed one past the seeds": (SEGMENTED.but(segments=segs_but(1, seed_end=4)), E_INVAL, SEG % 1),
    # 10: a segment's end (three sub-conditions)
    "end beyond the segment's blocks": (SEGMENTED.but(segments=segs_but(1, end_upos=UTOTAL + 1)), E_INVAL, SEG_END % 1),
    "end 11 bytes in front of its blocks' end": (SEGMENTED.but(segments=segs_but(0, end_upos=65836 - 11)), E_INVAL, SEG_END % 0),
    "end at the segment's first byte": (SEGMENTED.but(segments=segs_but(1, end_upos=65836)), E_INVAL, SEG_END % 1),
    "end_upos = 2^64 - 4: + 12 wraps to 8": (SEGMENTED.but(segments=segs_but(0, end_upos=U64 - 4)), E_INVAL, SEG_END % 0),
    # 11: a segment's seeds (three sub-conditions)
    "seed in front of its segment": (SEGMENTED.but(seeds=[0, 400, 65835]), E_INVAL, SEED_SEG % (2, 1)),
    "seed at its segment's end": (SEGMENTED.but(seeds=[0, 65836 - 12, 65840]), E_INVAL, SEED_SEG % (1, 0)),
    "seeds of a segment not ascending": (SEGMENTED.but(seeds=[400, 400, 65840]), E_INVAL, SEED_SEG % (1, 0)),
    # 12: behind the last segment
    "block behind the last segment": (SEGMENTED.but(segments=SEGS[:1], seeds=[0, 400]), E_INVAL, BEHIND),
    "seed behind the last segment": (SEGMENTED.but(seeds=[0, 400, 65840, 65841]), E_INVAL, BEHIND),
    # 13: a contiguous plan's seeds (two sub-conditions)
    "seed at end_upos": (CONTIG.but(seeds=[0, 400, UTOTAL]), E_INVAL, SEED % 2),
    "seed beyond a clamped end_upos": (CONTIG.but(seeds=[0, 400, UTOTAL + 5], end_upos=U64 - 1), E_INVAL, SEED % 2),
    "seeds not ascending": (CONTIG.but(seeds=[0, 400, 400]), E_INVAL, SEED % 2),
}

# Two defects each: the one that is reported is the earlier check's (null arrays, hap arena, [the loci's haplotypes: vtx_api.hip,]
# tid_begin and intervals, blocks, segments, a contiguous plan's seeds; inside a loop, the smaller index)
ORDER = {
    "null array before the hap arena": (CONTIG.but(nulls=("seeds",), hap_bytes=1 << 32), E_INVAL, NULL),
    "hap arena before tid_begin": (CONTIG.but(hap_bytes=1 << 32, tid_begin=[1, 2, 3]), E_UNSUPPORTED, "vtx_submit_bam: hap arena above 4 GiB"),
    "tid_begin's cover before its order": (CONTIG.but(tid_begin=[0, 4, 2]), E_INVAL, "vtx_submit_bam: tid_begin does not cover the intervals"),
    "an interval of contig 0 before tid_begin's order at contig 1": (CONTIG.but(tid_begin=[0, 4, 3], intervals=[(10, 60, 0), (9, 20, 1), (5, 15, 2)]), E_INVAL, IVAL % 1),
    "intervals before blocks": (CONTIG.but(intervals=[(10, 60, 0), (10, 20, 1), (5, 16, 2)], blocks=blocks_but(0, isize=65537)), E_INVAL, IVAL % 2),
    "block 0's trailer before block 1's order": (CONTIG.but(file_bytes=120, blocks=blocks_but(1, coff=0)), E_UNSUPPORTED, TRAIL % 0),
    "block 1's order before block 2's trailer": (CONTIG.but(file_bytes=FILE_BYTES - 1, blocks=blocks_but(1, coff=117)), E_INVAL, BLOCK % 1),
    "blocks before segments": (SEGMENTED.but(file_bytes=FILE_BYTES - 1, segments=[]), E_UNSUPPORTED, TRAIL % 2),
    "blocks before a contiguous plan's seeds": (CONTIG.but(blocks=blocks_but(2, isize=65537), seeds=[5, 5, 5]), E_INVAL, BLOCK % 2),
    "segment 0's seeds before segment 1's table": (SEGMENTED.but(seeds=[400, 400, 65840], segments=segs_but(1, block_end=4)), E_INVAL, SEED_SEG % (1, 0)),
    "a segment's end before its seeds": (SEGMENTED.but(seeds=[400, 400, 65840], segments=segs_but(0, end_upos=65836 - 11)), E_INVAL, SEG_END % 0),
    "a segmented plan's seeds are not held against base.end_upos": (SEGMENTED.but(end_upos=1), OK, ""),
}


def test_authored_plans_are_accepted_with_the_models_layout(core):
    for name, plan in ACCEPTS.items():
        g, sg, keep = plan.ctypes()
        status, why, lay = run_core(core, g, sg)
        assert status == OK, (name, why)
        a = plan.arrays()
        want = model(a, a.get("segments"))
        if plan.segments is not None:
            want.pop("end_upos", None)                       # "base.end_upos is ignored"
        assert_layout(lay, want, name)
    # ... and spelled out once, for the plans above: what the device is handed
    g, sg, keep = CONTIG.ctypes()
    lay = run_core(core, g, sg)[2]
    assert lay["blocks"].tolist() == [(0, 0, 100, 300), (126, 300, 50, 65536), (202, 65836, 772, 10)]
    assert (lay["lo"], lay["hi"], lay["utotal"], lay["comp_bytes"], lay["end_upos"]) == (18, 992, UTOTAL, 982, UTOTAL)
    g, sg, keep = SEGMENTED.ctypes()
    lay = run_core(core, g, sg)[2]
    assert lay["blocks"]["coff"].tolist() == [0, 126, 184] and lay["pieces"].tolist() == [(18, 0, 184), (220, 184, 780)] and lay["comp_bytes"] == 964
    assert lay["seed_seg"].tolist() == [0, 0, 1]
    assert lay["segs"].tolist() == [(0, 65836, 65824, 2, 0, 60, 0), (65836, UTOTAL, UTOTAL, 3, 1, 15, 1)]


@pytest.mark.parametrize("table", ["REJECTS", "ORDER"])
def test_every_reject_branch_and_the_order_of_the_checks(core, table):
    for name, (plan, status, message) in globals()[table].items():
        g, sg, keep = plan.ctypes()
        got, why, lay = run_core(core, g, sg)
        assert (got, why) == (status, message), name


def through_the_program(name, plans):
    """plans through tests/ingestplancore/main.cpp in ONE process -> [(status, message or the layout's arrays)]"""
    import tempfile
    subprocess.check_call(["make", "-C", os.path.join(HERE, "ingestplancore"), "-s", name])
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in"), os.path.join(d, "out")
        open(src, "wb").write(struct.pack("<I", len(plans)) + b"".join(p.encode() for p in plans))
        r = subprocess.run([os.path.join(HERE, "ingestplancore", name), src, dst], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        out = open(dst, "rb").read()
    res, p = [], 0
    for _ in plans:
        status, = struct.unpack_from("<i", out, p)
        p += 4
        if status != OK:
            n, = struct.unpack_from("<I", out, p)
            res.append((status, out[p + 4:p + 4 + n].decode()))
            p += 4 + n
            continue
        lay = dict(zip(FIGURES, struct.unpack_from("<10Q", out, p)))
        p += 80
        for k, dt, count in ARRAYS:
            lay[k] = np.frombuffer(out, dt, lay[count], p)
            p += lay[count] * dt.itemsize
        res.append((status, lay))
    assert p == len(out)
    return res


@pytest.mark.parametrize("name", ["ingest_plan_host", "ingest_plan_host_san"])
def test_what_the_checks_touch(core, name):
    """Every plan of the tables above in heap allocations of exactly its arrays' sizes: the same verdicts, messages and layouts as through
    the shared object, and (the sanitizer build) no load outside an array — the rejects whose indices point one past theirs included."""
    cases = [(n, p, OK, None) for n, p in ACCEPTS.items()] + [(n,) + v for t in (REJECTS, ORDER) for n, v in t.items()]
    res = through_the_program(name, [c[1] for c in cases])
    for (case, plan, status, message), (got, what) in zip(cases, res):
        assert got == status, case
        if status != OK:
            assert what == message, case
            continue
        g, sg, keep = plan.ctypes()
        lay = run_core(core, g, sg)[2]
        for k in FIGURES:
            assert what[k] == lay[k], (case, k)
        for k, _, _ in ARRAYS:
            assert np.array_equal(what[k], lay[k]), (case, k)
