"""The authored cases of tests/prep_cases.py through ``vtx_submit_raw`` on the PRODUCTION library: barcodes and UMIs whose 64-bit
hashes collide by construction, tags at every length around the word edges, key widths at every power of two and beside it, group
heads on workgroup edges.  For every case the counters and ``hash_rounds`` are the ledger's, the prepared records are those of
oracle/prep.py (reference src/main.rs:697-718, :737-750, :867-888, :932, :1047-1057) and of the CPU harness built from the kernels'
own header (tests/prepcore/), and the matrix after ``vtx_run`` is the host-prepared path's, bit for bit.  Then the validation of raw
records at the arena's last byte and one behind it, ``vtx_submit``'s five record codes with the record they name, and two child
processes: the dev library's forced hash collisions, and a BAM whose CB / UB tags are printable colliding pairs through the device
ingest against oracle/refpipe.py.  Everything compared is integers or bytes."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import prep_cases as PC
import prep_hash as ph
import prep_util as PU
from oracle import oracle, prep
from vartrix_amd import lib
from vartrix_amd.abi import (READS_NIBBLES, TAG_MISSING, VTX_E_INVAL, VTX_E_UNSUPPORTED, PackedBatch, RawBatch, default_config, pack_nibbles)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = os.path.join(HERE, "golden")
RAN = set()
NIBBLE_CASE = "n_kept_257"


@pytest.fixture(scope="module")
def core():
    return PU.load()


@pytest.fixture(scope="module")
def contexts():
    """one context per (n_barcodes, use_umi) for the raw path and one for the host-prepared path: the cases differ in their lists"""
    made = {}

    def get(n_barcodes, use_umi):
        key = (n_barcodes, use_umi)
        if key not in made:
            cfg = default_config(scoring_mode="alt_frac", use_umi=use_umi, n_barcodes=n_barcodes)
            made[key] = (lib.Context(cfg), lib.Context(cfg))
        return made[key]
    yield get
    for pair in made.values():
        for ctx in pair:
            ctx.close()


def canon(recs, begin, count):
    return prep.canonical_records(recs, begin, count)


def run_case(c, contexts, core, nibbles=False):
    raw = c.raw
    want, wstats = prep.prep_raw(raw, c.barcodes, bool(c.use_umi))
    if nibbles:
        raw = RawBatch(raw.loci, raw.records, raw.hap_arena, pack_nibbles(raw.read_arena), raw.tag_arena, READS_NIBBLES)
        want = want.to_nibbles()
    ctx, host_ctx = contexts(len(c.barcodes), c.use_umi)
    ctx.set_barcodes(c.barcodes)
    stats = ctx.submit_raw(raw)
    recs, begin, count = ctx.fetch_records()
    got = (int(stats.num_not_cell_bc), int(stats.num_non_umi), int(stats.kept), int(stats.hash_rounds))
    print(c.name, got)
    # the ledger
    assert got == (c.not_cell_bc, c.non_umi, c.kept, c.hash_rounds), c.name
    assert {int(r["read_off"]): int(r["cell_index"]) for r in recs} == c.expected_cells(), c.name
    # the oracle and the CPU harness
    assert (wstats["num_not_cell_bc"], wstats["num_non_umi"], want.n_records) == got[:3], c.name
    assert np.array_equal(begin, want.loci["rec_begin"]) and np.array_equal(count, want.loci["rec_count"]), c.name
    assert canon(recs, begin, count) == canon(want.records, want.loci["rec_begin"], want.loci["rec_count"]), c.name
    hrc, hst, hrecs, hbegin, hcount = PU.prepare(core, c.raw, c.barcodes, c.use_umi)
    assert hrc == 0 and hst["hash_rounds"] == got[3] and np.array_equal(hbegin, begin) and np.array_equal(hcount, count), c.name
    assert canon(hrecs, hbegin, hcount) == canon(recs, begin, count), c.name
    # the order vtx_submit demands of a host: (cell, UMI group) non-decreasing inside every locus
    for b0, n in zip(begin, count):
        r = recs[int(b0):int(b0) + int(n)]
        assert np.all(np.diff(r["cell_index"].astype(np.int64) << 32 | r["umi_id"].astype(np.int64)) >= 0), c.name
    # the matrix
    ctx.run()
    coo = ctx.fetch_coo()
    host_ctx.submit(want)
    host_ctx.run()
    wcoo = host_ctx.fetch_coo()
    for k in ("row", "col", "alt", "ref", "unk"):
        assert np.array_equal(coo[k], wcoo[k]), (c.name, k)
    assert np.array_equal(coo["value"].view(np.uint64), wcoo["value"].view(np.uint64)), c.name
    assert np.array_equal(coo["ref_value"].view(np.uint64), wcoo["ref_value"].view(np.uint64)), c.name
    return len(coo["row"])


GROUPS = ("barcode", "order", "umi", "boundary") + tuple("width_b%d" % b for b in PC.WIDTH_BARCODES)


def group_of(c):
    return c.name[:8] if c.name.startswith("width_b") else ("width_b4" if c.group == "width" else c.group)


@pytest.mark.parametrize("group", GROUPS)
def test_cases_through_vtx_submit_raw(contexts, core, group):
    cases = [c for c in PC.CASES if group_of(c) == group]
    assert cases
    entries = 0
    for c in cases:
        entries += run_case(c, contexts, core)
        RAN.add(c.name)
    assert entries > 0


def test_one_case_with_reads_as_nibbles(contexts, core):
    assert run_case(PC.BY_NAME[NIBBLE_CASE], contexts, core, nibbles=True) > 0
    RAN.add(NIBBLE_CASE + "@nibbles")


def test_the_cases_run_are_the_ledger():
    """(behind the tests above, which every run of this file includes: no case is left out, none is run that the ledger lacks)"""
    assert RAN == set(PC.LEDGER) | {NIBBLE_CASE + "@nibbles"}, sorted(set(PC.LEDGER) - RAN)[:10]


# ---------------------------------------------------------------- raw validation ----------------------------------------------------------------
def test_raw_records_at_the_arena_edge_and_one_byte_beyond(core):
    """Each of the five conditions of prep_resolve_kernel: offset + length == arena size is accepted, one more is VTX_E_INVAL, and
    the context prepares the next batch as if nothing had happened."""
    c = PC.BY_NAME["umi_interleaved"]
    reads = np.concatenate([c.raw.read_arena, np.frombuffer(b"ACGT" * 7501, np.uint8)])       # room for a read of the hard limit, and one base more
    n_tag, n_read, big = int(c.raw.tag_arena.size), int(reads.size), int(c.raw.read_arena.size)
    assert n_read - big == PU.MAX_READ_LEN + 4
    want = canon(*PU.prepare(core, c.raw, c.barcodes, 1)[2:])
    # (fields of record 2, nibbles, accepted)
    edges = [
        (dict(bc_off=n_tag - 9, bc_len=9), False, True), (dict(bc_off=n_tag - 8, bc_len=9), False, False),
        (dict(bc_off=n_tag, bc_len=0), False, True), (dict(bc_off=n_tag + 1, bc_len=0), False, False),
        (dict(umi_off=n_tag - 10, umi_len=10), False, True), (dict(umi_off=n_tag - 9, umi_len=10), False, False),
        (dict(umi_off=n_tag, umi_len=0), False, True), (dict(umi_off=n_tag + 1, umi_len=0), False, False),
        (dict(umi_off=0xffffffff, umi_len=TAG_MISSING), False, True),
        (dict(read_off=n_read - 32, read_len=32), False, True), (dict(read_off=n_read - 31, read_len=32), False, False),
        (dict(read_off=n_read, read_len=0), False, True), (dict(read_off=n_read + 1, read_len=0), False, False),
        (dict(read_off=big, read_len=PU.MAX_READ_LEN), False, True), (dict(read_off=big, read_len=PU.MAX_READ_LEN + 1), False, False),
        (dict(read_off=big + 2, read_len=32), True, True), (dict(read_off=big + 1, read_len=32), True, False),
    ]
    cfg = default_config(scoring_mode="alt_frac", use_umi=1, n_barcodes=len(c.barcodes))
    with lib.Context(cfg) as ctx:
        ctx.set_barcodes(c.barcodes)
        for fields, nibbles, ok in edges:
            recs = c.raw.records.copy()
            for k, v in fields.items():
                recs[k][2] = v
            arena = pack_nibbles(reads) if nibbles else reads
            raw = RawBatch(c.raw.loci, recs, c.raw.hap_arena, arena, c.raw.tag_arena, READS_NIBBLES if nibbles else 0)
            assert (PU.prepare(core, RawBatch(c.raw.loci, recs, c.raw.hap_arena, reads, c.raw.tag_arena), c.barcodes, 1, nibbles=nibbles)[0] == 0) == ok, fields
            if ok:
                st = ctx.submit_raw(raw)
                assert int(st.kept) + int(st.num_not_cell_bc) + int(st.num_non_umi) == 5, fields
            else:
                with pytest.raises(lib.VtxError) as e:
                    ctx.submit_raw(raw)
                assert e.value.status == VTX_E_INVAL, fields
                with pytest.raises(lib.VtxError):
                    ctx.run()                                         # the failed submit left nothing resident
            st = ctx.submit_raw(c.raw)                                # usable afterwards
            assert int(st.kept) == 5 and canon(*ctx.fetch_records()) == want, fields


# ---------------------------------------------------------------- vtx_submit validation ----------------------------------------------------------------
def packed(name):
    c = PC.BY_NAME[name]
    want, _ = prep.prep_raw(c.raw, c.barcodes, True)
    return c, want


def expect_code(ctx, core, batch, n_barcodes, use_umi, record, code, status, nibbles=False):
    assert PU.check_word(core, batch, n_barcodes, use_umi, nibbles) == (record, code)        # the core's verdict ...
    with pytest.raises(lib.VtxError) as e:
        ctx.submit(batch)
    assert e.value.status == status, str(e.value)                                            # ... is the device's
    m = re.search(r"vtx_submit: record (\d+):", str(e.value))
    assert m and int(m.group(1)) == record, str(e.value)
    return str(e.value)


def test_vtx_submit_names_the_smallest_offending_record_and_its_code(core):
    c, good = packed("n_kept_513")
    nb = len(c.barcodes)
    assert good.n_records == 513 and good.n_loci == 3
    reads = np.concatenate([good.read_arena, np.frombuffer(b"ACGT" * 7502, np.uint8)])
    n_read, big = int(reads.size), int(good.read_arena.size)

    def variant(edits, arena=reads, fmt=0):
        recs = good.records.copy()
        for rec, fields in edits.items():
            for k, v in fields.items():
                recs[k][rec] = v
        return PackedBatch(good.loci, recs, good.hap_arena, arena, fmt)

    cfg = default_config(scoring_mode="alt_frac", use_umi=1, n_barcodes=nb)
    with lib.Context(cfg) as ctx:
        def ok(batch, run=True, **kw):
            assert PU.check_word(core, batch, nb, 1, **kw) is None
            ctx.submit(batch)
            if run:
                ctx.run()
        ok(variant({}))
        ok(variant({300: dict(read_off=n_read - 32)}))                                        # flush against the arena's end
        ok(variant({300: dict(read_off=big, read_len=PU.MAX_READ_LEN)}), run=False)           # the hard limit itself
        msg = expect_code(ctx, core, variant({300: dict(read_off=n_read - 31)}), nb, 1, 300, 1, VTX_E_INVAL)
        assert "read outside read_arena" in msg
        msg = expect_code(ctx, core, variant({301: dict(read_off=big, read_len=PU.MAX_READ_LEN + 1)}), nb, 1, 301, 2, VTX_E_UNSUPPORTED)
        assert "read length 30001 above 30000" in msg
        msg = expect_code(ctx, core, variant({0: dict(cell_index=nb)}), nb, 1, 0, 3, VTX_E_INVAL)
        assert "cell_index %d >= n_barcodes %d" % (nb, nb) in msg
        ok(variant({512: dict(cell_index=nb - 1)}))
        # order: (cell, umi) descending inside a locus; record j is named, not j - 1
        cell, umi = good.records["cell_index"].astype(np.int64), good.records["umi_id"].astype(np.int64)
        lo, hi = int(good.loci["rec_begin"][1]), int(good.loci["rec_begin"][2])
        j = next(i for i in range(lo + 1, hi) if cell[i] == cell[i - 1] and umi[i] > umi[i - 1])      # a UMI boundary inside a cell: swap the two ids
        msg = expect_code(ctx, core, variant({j - 1: dict(umi_id=umi[j]), j: dict(umi_id=umi[j - 1])}), nb, 1, j, 4, VTX_E_INVAL)
        assert "not sorted by (cell_index, umi_id)" in msg
        k = next(i for i in range(lo + 1, hi) if cell[i] > cell[i - 1])                               # a cell boundary inside a locus: swap the two cells
        expect_code(ctx, core, variant({k - 1: dict(cell_index=cell[k]), k: dict(cell_index=cell[k - 1])}), nb, 1, k, 4, VTX_E_INVAL)
        # code 5: an odd read_off when the reads are nibbles
        nib = pack_nibbles(reads)
        ok(variant({}, nib, READS_NIBBLES), nibbles=True)
        msg = expect_code(ctx, core, variant({7: dict(read_off=big + 1)}, nib, READS_NIBBLES), nb, 1, 7, 5, VTX_E_INVAL, nibbles=True)
        assert "read_off %d is odd" % (big + 1) in msg
        # two offenders in different workgroups (records 100 and 400; 256 records each): the smaller record, with ITS code
        expect_code(ctx, core, variant({400: dict(read_off=n_read), 100: dict(cell_index=nb + 7)}), nb, 1, 100, 3, VTX_E_INVAL)
        expect_code(ctx, core, variant({100: dict(read_off=n_read), 400: dict(cell_index=nb + 7)}), nb, 1, 100, 1, VTX_E_INVAL)
        expect_code(ctx, core, variant({511: dict(read_off=n_read), 255: dict(cell_index=nb), 256: dict(cell_index=nb)}), nb, 1, 255, 3, VTX_E_INVAL)
        # the first condition in the sequence 1, 2, 3, 5, 4 names a record that meets several
        expect_code(ctx, core, variant({9: dict(read_off=n_read, read_len=PU.MAX_READ_LEN + 1, cell_index=nb)}), nb, 1, 9, 1, VTX_E_INVAL)
        expect_code(ctx, core, variant({9: dict(read_off=big, read_len=PU.MAX_READ_LEN + 1, cell_index=nb)}), nb, 1, 9, 2, VTX_E_UNSUPPORTED)
        ok(variant({}))                                                                      # usable afterwards


def test_legal_neighbours_pass_vtx_submit(core):
    """The cell index may fall from one locus to the next — here with the locus boundary at record 256, the first of a workgroup —
    and without --umi nothing orders umi_id."""
    c, good = packed("boundary_locus_at_256")
    nb = len(c.barcodes)
    assert list(good.loci["rec_begin"]) == [0, 256] and good.records["cell_index"][255] > good.records["cell_index"][256]
    assert PU.check_word(core, good, nb, 1) is None
    with lib.Context(default_config(scoring_mode="alt_frac", use_umi=1, n_barcodes=nb)) as ctx:
        ctx.submit(good)
        ctx.run()
        want = ctx.fetch_coo()
        moved = good.loci.copy()                                   # the same records with the boundary one record later: 256 now descends INSIDE a locus
        moved["rec_count"] = [257, good.n_records - 257]
        moved["rec_begin"] = [0, 257]
        expect_code(ctx, core, PackedBatch(moved, good.records, good.hap_arena, good.read_arena), nb, 1, 256, 4, VTX_E_INVAL)
    recs = good.records.copy()
    recs["umi_id"] = recs["umi_id"].max() - recs["umi_id"]         # descending wherever it was ascending
    down = PackedBatch(good.loci, recs, good.hap_arena, good.read_arena)
    assert PU.check_word(core, down, nb, 1) is not None and PU.check_word(core, down, nb, 0) is None
    with lib.Context(default_config(scoring_mode="alt_frac", use_umi=0, n_barcodes=nb)) as ctx:
        ctx.submit(down)
        ctx.run()
        a = ctx.fetch_coo()
        ctx.submit(good)
        ctx.run()
        b = ctx.fetch_coo()
    for k in ("row", "col", "alt", "ref", "unk"):
        assert np.array_equal(a[k], b[k]), k
    assert len(want["row"]) > 0


# ---------------------------------------------------------------- child processes ----------------------------------------------------------------
def child(code, env_extra, timeout=600):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, HERE]), **env_extra)
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


def test_forced_collisions_on_the_dev_library():
    """A fresh process on the dev library.  VTX_PREP_WEAK_ROUNDS=1: every UMI hashes to 0 in the first round, so the byte and length
    compares of prep_finalize_kernel alone keep the molecules of the last-byte cases apart, and the second round gives the exact
    grouping.  =8: no round has a hash, VTX_E_STATE after 8 seeds; the next submit on the same context succeeds."""
    code = r"""
import os
import numpy as np
import prep_cases as PC
from oracle import prep
from vartrix_amd import lib
from vartrix_amd.abi import VTX_E_STATE, default_config
assert lib.DEFAULT_VARIANT == "dev"
canon = prep.canonical_records
cfg = default_config(scoring_mode="alt_frac", use_umi=1, n_barcodes=len(PC.C))
with lib.Context(cfg) as ctx:
    ctx.set_barcodes(PC.C)
    os.environ["VTX_PREP_WEAK_ROUNDS"] = "1"
    for name in PC.WEAK_ROUND_CASES:
        c = PC.BY_NAME[name]
        assert c.barcodes == PC.C
        st = ctx.submit_raw(c.raw)
        recs, begin, count = ctx.fetch_records()
        want, _ = prep.prep_raw(c.raw, c.barcodes, True)
        assert st.hash_rounds == 2, (name, st.hash_rounds)
        assert canon(recs, begin, count) == canon(want.records, want.loci["rec_begin"], want.loci["rec_count"]), name
        print("WEAK", name, st.hash_rounds)
    os.environ["VTX_PREP_WEAK_ROUNDS"] = "8"
    c = PC.BY_NAME["umi_collide_one_cell"]
    try:
        ctx.submit_raw(c.raw)
        raise SystemExit("no error")
    except lib.VtxError as e:
        assert e.status == VTX_E_STATE and "8 different seeds" in str(e), str(e)
        print("STATE", e)
    os.environ["VTX_PREP_WEAK_ROUNDS"] = "0"
    st = ctx.submit_raw(c.raw)
    recs, begin, count = ctx.fetch_records()
    want, _ = prep.prep_raw(c.raw, c.barcodes, True)
    assert st.hash_rounds == 2 and canon(recs, begin, count) == canon(want.records, want.loci["rec_begin"], want.loci["rec_count"])
    ctx.run()
    print("NEXT", st.hash_rounds, len(ctx.fetch_coo()["row"]))
"""
    out = child(code, dict(VTX_LIB_VARIANT="dev"))
    assert out.count("WEAK ") == len(PC.WEAK_ROUND_CASES) and "STATE " in out and "NEXT 2 " in out, out


def colliding_bam(tmp_path):
    """A BAM over the DNA fixture whose CB and UB tags are printable colliding pairs, and its barcode list.  Listed: A, A' (one hash:
    two cells), B.  In the reads: those, T (B's hash, not listed) and the UMIs U, U' (one hash under the first UMI seed).  At every
    SNV, cell A has one REF read with U and one ALT read with U': two molecules, alt 1 and ref 1; merged they would be one UNKNOWN."""
    from oracle import bamwriter, refpipe
    rng = random.Random(20261021)
    a, b, u = b"ACGTACGTACGTAC-1", b"TTGACCAGGTCATG-1", b"AACCGGTTAC"
    a2, t = ph.collide_printable(a, rng), ph.collide_printable(b, rng)
    u16 = u + b"-umi01"
    u2 = ph.collide_printable(u16, rng, PC.SEED0)
    assert ph.hash_bytes(a) == ph.hash_bytes(a2) and ph.hash_bytes(b) == ph.hash_bytes(t) and len({a, a2, b, t}) == 4
    assert ph.hash_bytes(u16, PC.SEED0) == ph.hash_bytes(u2, PC.SEED0) and u16 != u2 and ph.hash_bytes(u16, PC.SEED1) != ph.hash_bytes(u2, PC.SEED1)
    fa = refpipe.read_fasta(os.path.join(G, "test_dna.fa"))["1"].upper()
    vcf = refpipe.read_vcf(os.path.join(G, "test_dna.vcf"))
    rows = []                                                      # SNVs with no other variant within 300 bases: a locus sees its own reads only
    for i, v in enumerate(vcf):
        if len(v.alleles) == 2 and len(v.alleles[0]) == len(v.alleles[1]) == 1 and v.pos > 200 and \
                all(abs(w.pos - v.pos) > 300 for w in vcf if w is not v) and len(rows) < 6:
            rows.append(i)
    assert len(rows) >= 3
    recs = []
    for v in (vcf[i] for i in rows):
        for k, (cb, ub, alt) in enumerate([(a, u16, False), (a, u2, True), (a2, u16, True), (a2, u16, True), (t, u16, True), (b, u2, False),
                                           (b, u16, False), (t, u2, False), (a2, u2, False)]):
            start = v.pos - 40 - k
            seq = fa[start:v.pos] + (v.alleles[1].upper() if alt else fa[v.pos:v.pos + 1]) + fa[v.pos + 1:start + 90]
            recs.append((start, bamwriter.record(0, start, "q%d_%d" % (v.pos, k), seq.decode(), "90M", tags=[("CB", "Z", cb), ("UB", "Z", ub)])))
    recs.sort(key=lambda x: x[0])
    bam = str(tmp_path / "collide.bam")
    bamwriter.write_bam(bam, [("1", len(fa))], [r for _, r in recs], block=4000)
    bcs = str(tmp_path / "barcodes.tsv")
    with open(bcs, "wb") as f:
        f.write(b"\n".join([a, a2, b]) + b"\n")
    return dict(vcf=os.path.join(G, "test_dna.vcf"), bam=bam, fasta=os.path.join(G, "test_dna.fa"), cell_barcodes=bcs), rows


def test_a_bam_with_colliding_tags_through_the_device_ingest(tmp_path):
    """End to end in a fresh process: vartrix_amd.api.run with ingest="device" on the production library must give what
    oracle/refpipe.py's pack and the C oracle give — colliding barcodes in their own columns, the unlisted one counted, colliding
    UMIs as two molecules."""
    from oracle import refpipe
    files, rows = colliding_bam(tmp_path)
    bcs = refpipe.load_barcodes(files["cell_barcodes"])
    vcf = refpipe.read_vcf(files["vcf"])
    batch, wm = refpipe.pack(vcf, refpipe.read_fasta(files["fasta"]), refpipe.read_bam(files["bam"]), bcs, refpipe.Args(use_umi=True))
    cfg = default_config(aligner="banded", scoring_mode="coverage", use_umi=1, n_barcodes=len(bcs))
    r, a = oracle.batch_scores(batch, cfg, threads=4)
    coo = oracle.batch_reduce(batch, cfg, r, a)
    dense = {k: np.zeros((len(vcf), len(bcs)), np.int64) for k in ("alt", "ref", "unk")}
    for k in dense:
        dense[k][coo["row"], coo["col"]] = coo[k]
    # what the construction promises, of the ORACLE: A has two molecules (alt 1, ref 1), A' two (alt 1, ref 1), B two REF ones
    assert wm["num_not_cell_bc"] == 2 * len(rows) and wm["num_non_umi"] == 0
    for i in rows:
        assert [dense[k][i].tolist() for k in ("alt", "ref", "unk")] == [[1, 1, 0], [1, 1, 2], [0, 0, 0]], i
    np.savez(str(tmp_path / "want.npz"), n=len(coo["row"]), not_bc=wm["num_not_cell_bc"], non_umi=wm["num_non_umi"], reads=wm["num_reads"], **dense)
    code = r"""
import sys
import numpy as np
from vartrix_amd import api, lib
assert lib.DEFAULT_VARIANT == ""
files = dict(vcf=sys.argv[1], bam=sys.argv[2], fasta=sys.argv[3], cell_barcodes=sys.argv[4])
want = np.load(sys.argv[5])
got = api.run(**files, scoring_method="coverage", umi=True, ingest="device")
assert got.metrics["num_not_cell_bc"] == int(want["not_bc"]) and got.metrics["num_non_umi"] == int(want["non_umi"]), got.metrics
assert got.metrics["num_reads"] == int(want["reads"]), got.metrics
for k, m in (("alt", got.alt_counts), ("ref", got.ref_counts), ("unk", got.unknown_counts)):
    assert m.nnz == int(want["n"]) and np.array_equal(m.toarray().astype(np.int64), want[k]), k
assert np.array_equal(got.matrix.toarray().astype(np.int64), want["alt"]) and np.array_equal(got.ref_matrix.toarray().astype(np.int64), want["ref"])
print("E2E", int(want["n"]), got.metrics["num_not_cell_bc"])
"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, HERE]))
    env.pop("VTX_LIB_VARIANT", None)
    out = subprocess.run([sys.executable, "-c", code, files["vcf"], files["bam"], files["fasta"], files["cell_barcodes"], str(tmp_path / "want.npz")],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "E2E " in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
