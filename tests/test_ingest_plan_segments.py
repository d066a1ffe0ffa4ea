"""The SEGMENTED plan of a device-side ingest (sparse loci: vtxh_plan_ingest -> the struct vtx_submit_bam_segments takes) without a GPU.

Where the planner used to say "sparse loci" it now hands out several stretches of the file.  With the planned blocks inflated by zlib
here: segments are ascending and disjoint in the file; every seed is a record start; every chain inside a segment lands on the next
seed of that segment and the last one on the segment's stated end, a record start whose (tid, pos) lies behind the segment's last
locus (what the device proves before it uses the segment); no segment ends inside a record; every record that overlaps a planned locus
is covered exactly once.  Inputs that get a contiguous plan keep it, array for array (recorded from the commit before this one).
The kernels are checked against the host packer on the device (tests/test_gpu_ingest_segments.py)."""
import json
import os
import struct
import sys

import numpy as np
import pytest

from oracle import refpipe
from vartrix_amd import abi, hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
import segments_util as su  # noqa: E402

CASES = [(700, "linear"), (4000, "linear"), (4000, "csi"), (20000, "linear"), (20000, "csi")]


@pytest.fixture(scope="module", autouse=True)
def dev_library():
    hostlib.use_variant("dev")
    if not os.path.exists(hostlib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    yield
    hostlib.use_variant("dev" if os.environ.get("VTX_LIB_VARIANT") == "dev" else "")


def check_segmented_plan(inputs, **kw):
    """-> dict of figures.  Every structural property of a segmented plan, against the file itself."""
    f, file_blocks = su.bgzf_blocks(inputs["bam"])
    with hostlib.plan_ingest(**inputs, **kw) as plan:
        assert plan.reason is None, plan.reason
        assert plan.kind == "segmented", plan.kind
        a = plan.arrays()
        planned, total = plan.blocks_planned, plan.blocks_total
    blocks, seeds, segs = a["blocks"], a["seeds"], a["segments"]
    assert len(segs) >= 1 and planned == len(blocks) and total == len(file_blocks)
    index_of = {c: k for k, (c, _, _) in enumerate(file_blocks)}
    data = su.inflate(f, blocks)
    bam = refpipe.read_bam(inputs["bam"])
    iv, tb = a["intervals"], a["tid_begin"]
    starts = []
    nb = ns = ub = 0
    last_file_block = -1
    for k, S in enumerate(segs):
        # the segment table tiles the blocks and the seeds; blocks are consecutive IN the segment, ascending and disjoint across
        assert int(S["block_begin"]) == nb and int(S["seed_begin"]) == ns and S["block_end"] > S["block_begin"] and S["seed_end"] > S["seed_begin"]
        fb = [index_of[int(b["coff"])] for b in blocks[nb:int(S["block_end"])]]
        assert fb == list(range(fb[0], fb[0] + len(fb))) and fb[0] > last_file_block, k
        for b, i in zip(blocks[nb:int(S["block_end"])], fb):
            assert (int(b["coff"]), int(b["clen"]), int(b["isize"])) == file_blocks[i]
        last_file_block = fb[-1]
        ul = ub + int(blocks["isize"][nb:int(S["block_end"])].sum())
        end = int(S["end_upos"])
        sd = [int(s) for s in seeds[ns:int(S["seed_end"])]]
        assert sd == sorted(set(sd)) and ub <= sd[0] and sd[-1] < end <= ul
        for i, s in enumerate(sd):
            p, stop = s, sd[i + 1] if i + 1 < len(sd) else end
            while p < stop:
                bs, = struct.unpack_from("<I", data, p)
                assert bs >= 32 and p + 4 + bs <= ul, "segment %d: a record is cut by the end of the segment's blocks" % k
                starts.append(p)
                p += 4 + bs
            assert p == stop, "segment %d: chain %d does not land on the next seed / the stated end" % (k, i)
        # the stated end: the end of the file's records, or a record start whose (tid, pos) proves that nothing behind it overlaps
        # a locus of the segment
        if int(S["flags"]) & abi.SEGMENT_TO_EOF:
            assert fb[-1] == len(file_blocks) - 1 and end == ul
        else:
            assert end + 12 <= ul
            bs, tid, pos = struct.unpack_from("<Iii", data, end)
            assert bs >= 32
            assert tid % (1 << 32) > int(S["end_tid"]) or (tid == int(S["end_tid"]) and pos >= int(S["end_pos"])), (k, tid, pos)
        nb, ns, ub = int(S["block_end"]), int(S["seed_end"]), ul
    assert nb == len(blocks) and ns == len(seeds) and ub == len(data)
    # every record that overlaps a planned locus is covered exactly once
    seen = {}
    for p in starts:
        tid, pos = struct.unpack_from("<ii", data, p + 4)
        key = (tid, pos, data[p + 36:p + 36 + data[p + 12]])
        seen[key] = seen.get(key, 0) + 1
    assert max(seen.values()) == 1
    need = 0
    for r in bam.recs:
        if r.tid < 0 or r.tid >= len(tb) - 1:
            continue
        s = iv[tb[r.tid]:tb[r.tid + 1]]
        if np.any((s["start"] < r.end) & (s["end"] > r.pos)):
            need += 1
            assert seen.get((r.tid, r.pos, r.qname + b"\x00")) == 1, (r.tid, r.pos, r.qname)
    return dict(segments=len(segs), blocks=len(blocks), contiguous_blocks=a["contiguous_blocks"], file_blocks=total, records=len(starts),
                need=need, inflated=len(data), contiguous_inflated=a["contiguous_inflated"])


@pytest.mark.parametrize("block,index", CASES)
def test_sparse_loci_get_a_segmented_plan(tmp_path, monkeypatch, block, index):
    """Loci far apart, two close together, reads spliced across 30 kb into a locus, a locus without reads, two contigs; BGZF blocks of
    700 / 4 000 / 20 000 bytes; .bai and .csi.

    Blocks to inflate, device plan against the host's own index-guided sweep of the same input (hostlib.last_ingest_stats).  The plan
    ends a segment at the index's record start four 16 kb windows behind the locus' last window, the sweep at the first record behind
    the locus: per segment up to five windows of reads more (four, and the rest of the locus' own window), and a block at either end.
    These inputs hold 3.76 inflated bytes of BAM per base (6.0 MB on 1.6 Mb), i.e. 308 kB per five windows.  Measured on these inputs
    (6 segments each; planned blocks; the host sweep's blocks; blocks of the file; of the contiguous stretch):
        block   700 linear: 2 234; 1 056; 8 582; 8 018   -> 197 per segment more than the sweep; asserted <= 442 per segment
        block  4000 linear:   397;   838; 1 503; 1 404   -> fewer than the sweep (a restart of the sweep over-reads ~64 blocks,
        block  4000 csi   :   477;   870; 1 503; 1 404      and reads on to the next locus where that is near); asserted <= 79
        block 20000 linear:    85;   302;   302;   281   -> the sweep inflates the whole file; asserted <= 18
        block 20000 csi   :   101;   302;   302;   281
    (.csi: its leaf bins give coarser record starts than the .bai's windows where a window is empty, so a stretch starts earlier.)
    Asserted: planned <= sweep + segments * (ceil(5 windows * 16 384 bases * inflated bytes per base / block size) + 2)."""
    monkeypatch.setenv("VTXH_SPARSE_KIB", su.SPARSE_KIB)
    inputs = su.author(tmp_path, block=block, index=index)
    fig = check_segmented_plan(inputs, use_umi=True)
    hostlib.pack_files(threads=2, use_umi=True, **inputs)
    sweep = dict(hostlib.last_ingest_stats)
    per_base = sum(isize for _, _, isize in su.bgzf_blocks(inputs["bam"])[1]) / sum(ln for _, ln in su.CONTIGS)      # inflated bytes of the file per base
    slack = int(np.ceil(5 * 16384 * per_base / block)) + 2
    print("block %d %s: segments %d, planned blocks %d, host sweep %d, file %d, contiguous stretch %d, slack per segment %d" %
          (block, index, fig["segments"], fig["blocks"], sweep["blocks_inflated"], fig["file_blocks"], fig["contiguous_blocks"], slack))
    assert fig["need"] > 100 and fig["records"] >= fig["need"]
    assert 3 <= fig["segments"] <= len(su.LOCI)                          # the close loci share a segment, the far ones do not
    assert fig["blocks"] < fig["contiguous_blocks"] <= fig["file_blocks"] and fig["inflated"] < fig["contiguous_inflated"]
    assert fig["blocks"] <= sweep["blocks_inflated"] + fig["segments"] * slack


def test_ranges_of_rows_may_be_segmented_or_not(tmp_path, monkeypatch):
    """Streamed ranges: the rows of the first three loci are two stretches far apart (segmented), a range of one locus is one stretch
    (contiguous: below the thresholds); each plan covers its own loci's reads."""
    monkeypatch.setenv("VTXH_SPARSE_KIB", su.SPARSE_KIB)
    inputs = su.author(tmp_path, block=4000)
    fig = check_segmented_plan(inputs, rows=(0, 3))
    assert fig["segments"] == 2
    with hostlib.plan_ingest(**inputs, rows=(3, 4)) as plan:
        assert plan.reason is None and plan.kind == "contiguous" and plan.segments is None


def test_production_library_keeps_the_contiguous_plan(tmp_path):
    """No knob, BAM below 64 MiB: the production library plans ONE stretch, and it is the plan the commit before the segmented one
    made — blocks (as ISIZEs from the first planned block of the file on: compressed sizes depend on the zlib that authors the file),
    seeds and end_upos recorded from that commit in tests/golden/ingest_plan_contiguous_parent.json."""
    want = json.load(open(os.path.join(G, "ingest_plan_contiguous_parent.json")))
    hostlib.use_variant("")
    try:
        for block, index in CASES:
            inputs = su.author(tmp_path, block=block, index=index)
            f, file_blocks = su.bgzf_blocks(inputs["bam"])
            index_of = {c: k for k, (c, _, _) in enumerate(file_blocks)}
            with hostlib.plan_ingest(**inputs, use_umi=True) as plan:
                assert plan.reason is None and plan.kind == "contiguous" and plan.segments is None
                a = plan.arrays()
            got = plan_digest(a, index_of)
            assert got == want["%d_%s" % (block, index)], (block, index)
    finally:
        hostlib.use_variant("dev")


def plan_digest(a, index_of):
    import hashlib
    blocks = a["blocks"]
    fb = [index_of[int(c)] for c in blocks["coff"]]
    assert fb == list(range(fb[0], fb[0] + len(fb)))
    return dict(first_block=fb[0], n_blocks=len(fb), isize_sha256=hashlib.sha256(blocks["isize"].astype("<u4").tobytes()).hexdigest(),
                n_seeds=len(a["seeds"]), seeds_sha256=hashlib.sha256(a["seeds"].astype("<u8").tobytes()).hexdigest(),
                seeds_head=[int(s) for s in a["seeds"][:8]], end_upos=int(a["end_upos"]))
