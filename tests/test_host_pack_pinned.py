"""The host packer's packs, plans and errors, pinned byte for byte (no GPU): tests/golden/host_pack_parent.json was recorded from the
commit before pack_impl was split into stages and must not change.

A pack's digest is a sha256 over, per batch, loci, records (or raw records), hap_arena, read_arena, tag_arena; then the metrics,
n_variants, the barcode list and the variant names (`pack_stream`).  Three inputs (the reference fixture, an authored DNA BAM of
700-byte blocks, the sparse two-contig input of segments_util) x raw / cooked x use_umi x nibbles / bytes x the developer hooks, each
at 1, 3 and 16 threads — the digest may not depend on the thread count — and one range of rows per input.  Plans: plan_digest of
tests/test_ingest_plan_segments.py (no compressed sizes: they depend on the zlib that authors the file) per stretch, over that file's
CASES, with and without VTXH_SPARSE_KIB and with a range of rows.  Errors: (code, message) of every cheap failure.

The same calls run as a stand-alone program under AddressSanitizer + UBSan and under ThreadSanitizer (tests/hostpack/): nothing is
preloaded, nothing runs inside this process; the program writes the stream the digest is taken over.

Re-record (from the library of the commit to compare against):  python tests/test_host_pack_pinned.py --record [--lib libvtxhost_dev.so]"""
import ctypes as C
import hashlib
import json
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import crc_util  # noqa: E402
import segments_util as su  # noqa: E402
from test_host import make_dna_bam  # noqa: E402
from test_ingest_plan_segments import CASES, plan_digest  # noqa: E402
from vartrix_amd import abi, hostlib  # noqa: E402

GOLDEN = os.path.join(G, "host_pack_parent.json")
HOOKS = {"none": {}, "chunk1": {"VTXH_CHUNK_BLOCKS": "1"}, "noindex": {"VTXH_NO_INDEX": "1"}, "batch60k": {"VTXH_BATCH_BYTES": "60000"}}
ALL_HOOKS = sorted({k for h in HOOKS.values() for k in h} | {"VTXH_SPARSE_KIB"})
THREADS = (1, 3, 16)
ROWS = {"ref": (1, 3), "dna": (10, 30), "seg": (0, 3)}
INPUTS = ("ref", "dna", "seg")


@pytest.fixture(scope="module", autouse=True)
def dev_library():
    hostlib.use_variant("dev")
    if not os.path.exists(hostlib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    yield
    hostlib.use_variant("dev" if os.environ.get("VTX_LIB_VARIANT") == "dev" else "")


def dna_inputs(bam):
    return dict(vcf=os.path.join(G, "test_dna.vcf"), bam=bam, fasta=os.path.join(G, "test_dna.fa"), cell_barcodes=os.path.join(G, "dna_barcodes.tsv"))


def make_inputs(d):
    """name -> dict(vcf=, bam=, fasta=, cell_barcodes=), authored once under d."""
    os.makedirs(os.path.join(d, "dna"))
    os.makedirs(os.path.join(d, "seg"))
    from pathlib import Path
    return {"ref": dict(vcf=os.path.join(G, "test.vcf"), bam=os.path.join(G, "test.bam"), fasta=os.path.join(G, "test.fa"),
                        cell_barcodes=os.path.join(G, "barcodes.tsv")),
            "dna": dna_inputs(make_dna_bam(Path(d) / "dna", seed=4, n_reads=3000, block=700)),
            "seg": su.author(os.path.join(d, "seg"), block=4000)}


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return make_inputs(str(tmp_path_factory.mktemp("pinned")))


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


class hooks:
    """The developer library's environment hooks for the calls inside (it reads them at every call)."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.keep = {k: os.environ.pop(k, None) for k in ALL_HOOKS}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def tail_stream(metrics, n_variants, barcodes, variants):
    return (b"metrics" + struct.pack("<9Q", *(metrics[n] for n in hostlib.METRIC_NAMES)) + struct.pack("<I", n_variants) +
            b"".join(b + b"\n" for b in barcodes) + b"".join(v.encode() + b"\n" for v in variants))


def pack_stream(inp, raw, **kw):
    """The bytes a pack's digest is taken over (tests/hostpack/harness.cpp writes the same), and the ingest statistics."""
    batches, metrics, nv, barcodes, variants = hostlib.pack_files(raw=raw, all_batches=True, **inp, **kw)
    out = []
    for b in batches:
        out += [b.loci.tobytes(), b.records.tobytes(), b.hap_arena.tobytes(), b.read_arena.tobytes()]
        if raw:
            out.append(b.tag_arena.tobytes())
    out.append(tail_stream(metrics, nv, barcodes, variants))
    return b"".join(out), len(batches), dict(hostlib.last_ingest_stats)


def pack_entry(inp, raw, **kw):
    s, nb, stats = pack_stream(inp, raw, **kw)
    return dict(sha256=hashlib.sha256(s).hexdigest(), batches=nb, **stats)


def pack_keys(name):
    """(key, hook, threads to run, keywords) of every pack of one input."""
    for raw in (False, True):
        for umi in (False, True):
            for nib in (False, True):
                for hook in HOOKS:
                    yield ("%s/%s/umi%d/%s/%s" % (name, "raw" if raw else "cooked", umi, "nibbles" if nib else "bytes", hook), hook, THREADS,
                           dict(raw=raw, use_umi=umi, nibbles=nib))
        for hook in HOOKS:      # the range of rows: both kinds of pack, every hook
            yield ("%s/%s/umi1/nibbles/%s/rows%d-%d" % ((name, "raw" if raw else "cooked", hook) + ROWS[name]), hook, (3,),
                   dict(raw=raw, use_umi=True, nibbles=True, rows=ROWS[name]))


def plan_stream(plan, a):
    """The bytes of a plan (harness.cpp writes the same): no compressed offsets or sizes."""
    kind = {None: 0, "contiguous": 1, "segmented": 2}[plan.kind]
    out = [struct.pack("<I", kind), (plan.reason or "").encode() + b"\n"]
    if a is not None:
        out += [a["blocks"]["isize"].astype("<u4").tobytes(), a["seeds"].astype("<u8").tobytes(), struct.pack("<Q", a["end_upos"])]
        if plan.kind == "segmented":
            out += [a["segments"].tobytes(), struct.pack("<IQ", a["contiguous_blocks"], a["contiguous_inflated"])]
        out += [a[k].tobytes() for k in ("intervals", "tid_begin", "tid_max_span", "loci", "hap_arena")]
    out.append(tail_stream(plan.metrics, plan.n_variants, plan.barcodes, plan.variants))
    return b"".join(out)


def plan_entry(inp, **kw):
    _, file_blocks = su.bgzf_blocks(inp["bam"])
    index_of = {c: k for k, (c, _, _) in enumerate(file_blocks)}
    with hostlib.plan_ingest(**inp, **kw) as plan:
        a = plan.arrays() if plan.reason is None else None
        e = dict(kind=plan.kind, reason=plan.reason, blocks_planned=plan.blocks_planned, blocks_total=plan.blocks_total,
                 sha256=hashlib.sha256(plan_stream(plan, a)).hexdigest())
    if a is None:
        return e
    if plan.kind == "segmented":        # plan_digest per stretch: the blocks of ONE stretch are consecutive in the file
        e["stretches"] = [plan_digest(dict(blocks=a["blocks"][int(S["block_begin"]):int(S["block_end"])],
                                           seeds=a["seeds"][int(S["seed_begin"]):int(S["seed_end"])], end_upos=S["end_upos"]), index_of)
                          for S in a["segments"]]
        e["ends"] = [[int(S["end_tid"]), int(S["end_pos"]), int(S["flags"])] for S in a["segments"]]
        e["contiguous"] = [a["contiguous_blocks"], a["contiguous_inflated"]]
    elif len(a["blocks"]):
        e["stretches"] = [plan_digest(a, index_of)]
    return e


def plan_cases(d, cases=CASES):
    """(key, inputs, hooks, keywords) of every pinned plan."""
    for block, index in cases:
        sub = os.path.join(d, "plan_%d_%s" % (block, index))
        os.makedirs(sub)
        inp = su.author(sub, block=block, index=index)
        for sparse in (False, True):
            for rows in (None, (0, 3), (3, 4)):
                yield ("seg/%d_%s/%s/%s" % (block, index, "sparse_kib" if sparse else "default", "rows%d-%d" % rows if rows else "all"), inp,
                       {"VTXH_SPARSE_KIB": su.SPARSE_KIB} if sparse else {}, dict(use_umi=True, rows=rows))


def call(mode, inp, bam_tag="CB", threads=3):
    """(code, message) of vtxh_pack_files / vtxh_pack_files_raw / vtxh_plan_ingest as the C interface gives them."""
    L = hostlib.load()
    args = hostlib.VtxhArgs(inp["vcf"].encode(), inp["bam"].encode(), inp["fasta"].encode(), inp["cell_barcodes"].encode(), 100, 0, 0, 0,
                            1, bam_tag.encode(), b"ATGCatgc", threads, abi.READS_NIBBLES)
    h = C.c_void_p()
    if mode == "plan":
        rc = L.vtxh_plan_ingest(C.byref(args), 0, 0xFFFFFFFF, C.byref(h))
    else:
        rc = (L.vtxh_pack_files_raw if mode == "raw" else L.vtxh_pack_files)(C.byref(args), C.byref(h))
    if rc == 0:
        L.vtxh_free(h)
        return [0, ""]
    return [int(rc), L.vtxh_last_error().decode()]


def error_cases(d, dna_bam):
    """name -> inputs (and keywords of `call`) of every cheap failure."""
    from oracle import bamwriter
    ref = dict(vcf=os.path.join(G, "test.vcf"), bam=os.path.join(G, "test.bam"), fasta=os.path.join(G, "test.fa"), cell_barcodes=os.path.join(G, "barcodes.tsv"))
    dna = dna_inputs(dna_bam)
    p = lambda n: os.path.join(d, n)  # noqa: E731
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
    open(p("empty.tsv"), "w").close()
    open(p("malformed.vcf"), "w").write(head + "1\t200\t.\tA\n")
    open(p("zz.vcf"), "w").write(head + "zz\t10\t.\tA\tC\t.\t.\t.\n")
    # a contig the FASTA has and the BAM has not
    fa = open(os.path.join(G, "test_dna.fa"), "rb").read()
    open(p("extra.fa"), "wb").write(fa + b">extra\nACGTACGTAC\n")
    open(p("extra.fa.fai"), "w").write(open(os.path.join(G, "test_dna.fa.fai")).read() + "extra\t10\t%d\t10\t11\n" % (len(fa) + 7))
    open(p("extra.vcf"), "w").write(head + "extra\t3\t.\tG\tT\t.\t.\t.\n")
    eof = bamwriter._bgzf_block(b"")
    open(p("magic.bam"), "wb").write(bamwriter._bgzf_block(b"BAX\x01" + bytes(60)) + eof)
    open(p("short.bam"), "wb").write(bamwriter._bgzf_block(b"BAM\x01" + struct.pack("<i", 5000) + b"@HD\tVN:1.6\n") + eof)
    shutil.copy(os.path.join(G, "test.bam"), p("x.cram"))
    with crc_util.stored_blocks():
        os.makedirs(p("stored"))
        from pathlib import Path
        stored = make_dna_bam(Path(p("stored")), seed=4, n_reads=900)
    raw = open(stored, "rb").read()
    blocks = crc_util.blocks_of(raw)
    crc = {}
    for which, b in crc_util.first_middle_last(blocks).items():
        for kind, flip in (("trailer", crc_util.flip_trailer), ("stored_payload", crc_util.flip_stored_payload)):
            bad = bytearray(raw)
            flip(bad, b)
            name = "crc_%s_%s.bam" % (which, kind)
            open(p(name), "wb").write(bytes(bad))
            shutil.copy(stored + ".bai", p(name) + ".bai")
            crc["damaged crc: %s block, %s" % (which, kind)] = (dict(dna, bam=p(name)), {})
    return {"two-character tag": (ref, dict(bam_tag="CBX")),
            "empty barcode file": (dict(ref, cell_barcodes=p("empty.tsv")), {}),
            "malformed VCF line": (dict(ref, vcf=p("malformed.vcf")), {}),
            "contig missing from the FASTA": (dict(ref, vcf=p("zz.vcf")), {}),
            "contig missing from the BAM": (dict(dna, vcf=p("extra.vcf"), fasta=p("extra.fa")), {}),
            "record end beyond the contig": (dict(ref, vcf=os.path.join(G, "test_dna.vcf"), cell_barcodes=os.path.join(G, "dna_barcodes.tsv")), {}),
            "bad BAM magic": (dict(ref, bam=p("magic.bam")), {}),
            "truncated header": (dict(ref, bam=p("short.bam")), {}),
            ".cram name": (dict(ref, bam=p("x.cram")), {}),
            "missing BAM": (dict(ref, bam=p("nothing.bam")), {}), **crc}


def error_entries(d, dna_bam):
    out = {}
    for name, (inp, kw) in error_cases(d, dna_bam).items():
        for mode in ("cooked", "raw", "plan"):
            for threads in (1, 3):
                code, msg = call(mode, inp, threads=threads, **kw)
                out["%s/%s/threads%d" % (name, mode, threads)] = [code, msg.replace(d, "<TMP>").replace(G, "<GOLDEN>")]
    return out


@pytest.mark.parametrize("umi", [False, True], ids=["umi0", "umi1"])
@pytest.mark.parametrize("raw", [False, True], ids=["cooked", "raw"])
@pytest.mark.parametrize("name", INPUTS)
def test_packs_are_the_parents_at_every_thread_count(inputs, golden, name, raw, umi):
    n = 0
    for key, hook, threads, kw in pack_keys(name):
        if kw["raw"] != raw or kw["use_umi"] != umi:
            continue
        with hooks(HOOKS[hook]):
            got = {t: pack_entry(inputs[name], threads=t, **kw) for t in threads}
        for t in threads:
            assert got[t] == golden["packs"][key], (key, t)
        n += 1
    assert n == (12 if umi else 8) and len(golden["packs"]) == 120
    # the batch cutter is covered
    assert golden["packs"]["ref/raw/umi1/nibbles/batch60k"]["batches"] == 2
    assert golden["packs"]["dna/cooked/umi1/nibbles/batch60k"]["batches"] == 3 and golden["packs"]["dna/raw/umi1/nibbles/batch60k"]["batches"] == 5


@pytest.mark.parametrize("block,index", CASES)
def test_plans_are_the_parents(tmp_path, golden, block, index):
    kinds = set()
    n = 0
    for key, inp, env, kw in plan_cases(str(tmp_path), [(block, index)]):
        with hooks(env):
            got = plan_entry(inp, **kw)
        assert got == golden["plans"][key], key
        kinds.add(got["kind"])
        n += 1
    assert n == 6 and len(golden["plans"]) == 6 * len(CASES) and kinds == {"contiguous", "segmented"}


def test_errors_are_the_parents(tmp_path, inputs, golden):
    got = error_entries(str(tmp_path), inputs["dna"]["bam"])
    assert got == golden["errors"]
    assert all(code != 0 for key, (code, _) in got.items() if "plan" not in key)
    assert sum("CRC32" in msg for _, msg in got.values()) >= 6 * 4


@pytest.fixture(scope="module")
def sanitizer_programs():
    d = os.path.join(ROOT, "tests", "hostpack")
    subprocess.check_call(["make", "-C", d, "-s", "-j2", "all"])
    return [os.path.join(d, "host_pack_asan"), os.path.join(d, "host_pack_tsan")]


@pytest.mark.parametrize("name", ["dna", "seg"])
def test_stages_run_clean_under_the_sanitizers(inputs, sanitizer_programs, name):
    """AddressSanitizer + UBSan, and ThreadSanitizer (the sweep's two overlaps of threads share the stages' state), on the stand-alone
    program: exit 0, no report, and the bytes of the call made from Python."""
    inp = inputs[name]
    for env in ({}, {"VTXH_CHUNK_BLOCKS": "1"}):
        want = {}
        with hooks(env):
            want["cooked"] = pack_stream(inp, False, use_umi=True, nibbles=True, threads=4)[0]
            want["raw"] = pack_stream(inp, True, use_umi=True, nibbles=True, threads=4)[0]
            with hostlib.plan_ingest(**inp, use_umi=True, threads=4) as plan:
                want["plan"] = plan_stream(plan, plan.arrays() if plan.reason is None else None)
        clean = {k: v for k, v in os.environ.items() if k not in ALL_HOOKS}
        for prog in sanitizer_programs:
            for mode in ("cooked", "raw", "plan"):
                r = subprocess.run([prog, inp["vcf"], inp["bam"], inp["fasta"], inp["cell_barcodes"], mode, "4"], capture_output=True,
                                   env=dict(clean, **env), timeout=300)
                err = r.stderr.decode(errors="replace")
                assert r.returncode == 0, (prog, mode, err[-3000:])
                assert "Sanitizer" not in err and "runtime error" not in err, (prog, mode, err[-3000:])
                assert hashlib.sha256(r.stdout).hexdigest() == hashlib.sha256(want[mode]).hexdigest(), (prog, mode, env)


def record(lib):
    import tempfile
    hostlib.use_variant("dev")
    if lib:
        hostlib.LIB_PATH = os.path.abspath(lib)
    out = dict(packs={}, plans={}, errors={})
    with tempfile.TemporaryDirectory() as d:
        inp = make_inputs(os.path.join(d, "in"))
        for name in INPUTS:
            for key, hook, threads, kw in pack_keys(name):
                with hooks(HOOKS[hook]):
                    got = [pack_entry(inp[name], threads=t, **kw) for t in threads]
                assert all(g == got[0] for g in got), "the pack depends on the thread count: %s" % key
                out["packs"][key] = got[0]
        os.makedirs(os.path.join(d, "plans"))
        for key, pin, env, kw in plan_cases(os.path.join(d, "plans")):
            with hooks(env):
                out["plans"][key] = plan_entry(pin, **kw)
        os.makedirs(os.path.join(d, "err"))
        out["errors"] = error_entries(os.path.join(d, "err"), inp["dna"]["bam"])
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d packs, %d plans, %d errors from %s" % (len(out["packs"]), len(out["plans"]), len(out["errors"]), hostlib.LIB_PATH))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true")
    ap.add_argument("--lib", default="")
    a = ap.parse_args()
    if a.record:
        record(a.lib)
