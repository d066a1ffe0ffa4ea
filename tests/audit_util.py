"""Helpers of the audit tests: the oracle over a SUBSET of a batch's records, and the stage invariant."""
import os

import numpy as np

from oracle import oracle
from vartrix_amd import abi
from vartrix_amd.abi import PackedBatch, default_config


def sub_batch(batch, record_ids):
    """The same loci and arenas, only the listed records (ascending ids)."""
    ids = np.unique(np.asarray(record_ids, np.int64))
    rec_locus = np.repeat(np.arange(batch.n_loci), batch.loci["rec_count"])
    loci = batch.loci.copy()
    cnt = np.bincount(rec_locus[ids], minlength=batch.n_loci).astype(np.uint32)
    loci["rec_count"] = cnt
    loci["rec_begin"] = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.uint32)
    return PackedBatch(loci, np.ascontiguousarray(batch.records[ids]), batch.hap_arena, batch.read_arena), ids


def oracle_scores_of(batch, record_ids, aligner, n_barcodes):
    sub, ids = sub_batch(batch, record_ids)
    if len(ids) == 0:
        return ids, np.zeros(0, np.int32), np.zeros(0, np.int32)
    r, a = oracle.batch_scores(sub, default_config(aligner=aligner, n_barcodes=n_barcodes), threads=os.cpu_count() or 8)
    return ids, r, a


def stage_report(stage):
    return {abi.STAGE_NAMES.get(int(k), str(k)): int(v) for k, v in zip(*np.unique(stage, return_counts=True))}


def assert_stage_invariant(stage, banded, full, label=""):
    """banded = (ref, alt) of the banded flavour, full = of the full flavour, stage = vtx_fetch_stage of the banded run.
    cert <= banded <= full: an alignment whose two scores differ must have been decided by a DP stage or by the
    band-restricted certificate (abi.BANDED_STAGES)."""
    b = np.empty(2 * len(banded[0]), np.int32)
    f = np.empty_like(b)
    b[0::2], b[1::2] = banded
    f[0::2], f[1::2] = full
    assert np.all(b <= f), "%s: a banded score above the full-matrix score" % label
    known = np.isin(stage, list(abi.STAGE_NAMES))
    assert np.all(known), "%s: unknown stage byte %d" % (label, int(stage[~known][0]))
    differ = b != f
    by_cert = differ & ~np.isin(stage, abi.BANDED_STAGES)
    assert not by_cert.any(), "%s: task %d has banded %d != full %d but was decided by stage %d" % (
        label, int(np.nonzero(by_cert)[0][0]), int(b[by_cert][0]), int(f[by_cert][0]), int(stage[by_cert][0]))
    return differ


# ---- full-size stage audits (tests/test_gpu_properties.py, tools/full_audit.py): one table of workloads, one helper ----
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUDIT_SEED = 20260926                      # bench.py's sensitivity cases: test, tool and bench audit the same batches
# name -> SynthSpec keywords (over config 3: 100 k loci x 10 k barcodes x 256 reads, 150 bases, padding 100, 0.5 % errors), scoring
# mode, UMI.  e8 and real at full size (48.6 M alignments); the others at 24 k loci (11.7 M alignments), the budget of -m gpu.
# "adversarial" is tests/stress_batches.py's adversarial_batch, every family mixed, 20 k loci x 256 reads (10.2 M alignments);
# "adversarial_long" the excursion and read-indel families with haplotypes of 257 - 421 bases: such a batch is scored on round 3's
# path, where band_refine_kernel prices joins with join_gap3_far (within 255 bases band_corridor_kernel takes those tasks).
AUDIT_WORKLOADS = {
    "config3": (dict(), "consensus", 0),
    "e8": (dict(sub_error=0.08), "consensus", 0),
    "e3": (dict(sub_error=0.03, n_loci=24_000), "consensus", 0),
    "real": (dict(genome_fasta=os.path.join(ROOT, "tests", "golden", "test_dna.fa")), "consensus", 0),
    "config5": (dict(indel_frac=0.30, use_umi=True, n_loci=24_000), "alt_frac", 1),
    "reads250": (dict(read_len=250, n_loci=24_000), "consensus", 0),
    "padding150": (dict(padding=150, n_loci=24_000), "consensus", 0),
    "adversarial": (None, "consensus", 0),
    "adversarial_long": (None, "consensus", 0),
}
BANDED_BOUND_CERTS = (abi.STAGE_BAND_CERT, abi.STAGE_CORRIDOR_CERT)      # certificates of the BANDED score: the full run cannot check them


def audit_batch(name):
    """(batch, n_barcodes, label) of a workload of AUDIT_WORKLOADS, built the same way in every process."""
    from vartrix_amd import synth
    kw, _mode, _umi = AUDIT_WORKLOADS[name]
    if kw is None:
        import stress_batches as SB
        if name == "adversarial_long":
            return (SB.adversarial_batch(20_000, 256, AUDIT_SEED, ("excursion", "read_indels"), n_barcodes=10_000, pads=(138, 200)), 10_000,
                    "adversarial batches, excursions and read indels, haplotypes of 257 - 421 bases, 20 k loci x 256 reads")
        return SB.adversarial_batch(20_000, 256, AUDIT_SEED, n_barcodes=10_000), 10_000, "adversarial batches, every family, 20 k loci x 256 reads"
    spec = synth.SynthSpec(**dict(dict(n_loci=100_000, n_barcodes=10_000, reads_per_locus=256, seed=AUDIT_SEED), **kw))
    return synth.make_batch(spec), spec.n_barcodes, spec.name + (", padding %d" % spec.padding if spec.padding != 100 else "")


def audit_config(name, aligner, n_barcodes):
    _kw, mode, umi = AUDIT_WORKLOADS[name]
    return default_config(aligner=aligner, scoring_mode=mode, use_umi=umi, n_barcodes=n_barcodes)


_NO_DIAG_CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from audit_util import audit_batch, audit_config
from vartrix_amd import lib
name, out = sys.argv[1], sys.argv[2]
batch, nb, _ = audit_batch(name)
with lib.Context(audit_config(name, "banded", nb)) as ctx:
    ctx.submit(batch)
    ctx.set_stage_trace(True)
    ctx.set_poison(-4242)
    ctx.run()
    r, a = ctx.fetch_scores()
    st = ctx.fetch_stage()
np.save(os.path.join(out, "ref.npy"), r)
np.save(os.path.join(out, "alt.npy"), a)
np.save(os.path.join(out, "stage.npy"), st)
'''


def no_diag_run(name, tmp_dir, timeout=900):
    """The banded flavour of workload `name` through libvtx_dev.so with VTX_BAND_NO_DIAG=1 (the round-2 path: band_run_kernel takes
    every task, neither band_diag_kernel nor band_corridor_kernel runs), in a child process — the hook is read once per process.
    The child rebuilds the batch from the same spec and seed; returns its (ref, alt, stage)."""
    import subprocess
    import sys
    code = _NO_DIAG_CHILD % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, VTX_LIB_VARIANT="dev", VTX_BAND_NO_DIAG="1")
    r = subprocess.run([sys.executable, "-c", code, name, str(tmp_dir)], capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, "no-diag run of %s: exit status %d\n%s" % (name, r.returncode, r.stderr[-3000:])
    return tuple(np.load(os.path.join(str(tmp_dir), f + ".npy")) for f in ("ref", "alt", "stage"))


def _interleave(r, a):
    x = np.empty(2 * len(r), np.int32)
    x[0::2], x[1::2] = r, a
    return x


def full_size_audit(name, tmp_dir, per_stage=40_000, record_frac=0.01, oracle_records=None, log=print):
    """Every alignment of workload `name` (AUDIT_WORKLOADS) through the stage checks of the audit:
      1  production run: the banded flavour with libvtx.so, the stage trace on, the scores poisoned before each of two runs of the
         context — no poison left, and the second run (what a warm context computes) gives the first one's scores;
      2  full run: the full flavour (stage FULL_DP everywhere); assert_stage_invariant on EVERY alignment (banded <= full, and
         banded != full only under a stage of abi.BANDED_STAGES);
      3  independent banded reference: the no-diag run (no_diag_run) must give the production scores on EVERY alignment — the
         certificates of the banded score (BANDED_BOUND_CERTS) are checked there; what such a certificate decided in BOTH runs
         was not checked independently and goes to the oracle;
      4  oracle: the records of every alignment where the two device runs disagree, of up to `per_stage` random alignments of every
         stage that occurs (production and no-diag run), of the alignments above, and a `record_frac` random sample of the records
         (oracle_records(stage, differ): more record ids the caller wants checked).
    Returns a dict of what it saw, for the workload's premise."""
    from vartrix_amd import lib
    batch, nb, label = audit_batch(name)
    out = {}
    for aligner in ("banded", "full"):
        with lib.Context(audit_config(name, aligner, nb)) as ctx:
            ctx.submit(batch)
            ctx.set_stage_trace(True)
            ctx.set_poison(-4242)
            ctx.run()
            if aligner == "banded":
                first = ctx.fetch_scores()
                ctx.run()
            out[aligner] = ctx.fetch_scores() + (ctx.fetch_stage(), ctx.timing())
    assert np.array_equal(first[0], out["banded"][0]) and np.array_equal(first[1], out["banded"][1]), \
        "%s: the second run of the banded context differs from the first" % name
    del first
    rb, ab, stage, t = out["banded"]
    rf, af, fstage, _ = out["full"]
    del out
    assert not (rb == -4242).any() and not (ab == -4242).any(), "%s: a banded score was never written" % name
    assert not (rf == -4242).any() and not (af == -4242).any(), "%s: a full-matrix score was never written" % name
    assert np.all(fstage == abi.STAGE_FULL_DP), "%s: the full flavour reports stage %s" % (name, stage_report(fstage))
    differ = assert_stage_invariant(stage, (rb, ab), (rf, af), name)
    del rf, af, fstage
    # 3: the no-diag run (production contexts closed above)
    import time
    t0 = time.time()
    nr, na, nstage = no_diag_run(name, tmp_dir)
    t_child = time.time() - t0
    prod, ref_nd = _interleave(rb, ab), _interleave(nr, na)
    disagree = np.nonzero(prod != ref_nd)[0]
    # (the no-diag run runs neither band_corridor_kernel nor band_refine_kernel, so it never reports a certificate of the banded score:
    #  both_cert is empty by construction today, and every such certificate of the production run is checked against a DP or a
    #  certificate of the full score.  It is kept so that the audit stays right if the reference run ever gains one.)
    both_cert = np.nonzero(np.isin(stage, BANDED_BOUND_CERTS) & np.isin(nstage, BANDED_BOUND_CERTS))[0]
    cert_checked = int(np.isin(stage, BANDED_BOUND_CERTS).sum()) - len(both_cert)
    # 4: the oracle
    rng = np.random.default_rng(7)
    pick = [disagree >> 1, both_cert >> 1, rng.choice(batch.n_records, int(batch.n_records * record_frac), replace=False)]
    for st_arr in (stage, nstage):
        for s in np.unique(st_arr):
            idx = np.nonzero(st_arr == s)[0]
            pick.append((idx if len(idx) <= per_stage else rng.choice(idx, per_stage, replace=False)) >> 1)
    if oracle_records is not None:
        pick.append(np.asarray(oracle_records(stage, differ), np.int64))
    ids, oref, oalt = oracle_scores_of(batch, np.concatenate(pick), "banded", nb)
    want = _interleave(oref, oalt)
    tasks = (2 * ids[:, None] + np.arange(2)[None, :]).reshape(-1)
    bad_p = np.nonzero(prod[tasks] != want)[0]
    bad_n = np.nonzero(ref_nd[tasks] != want)[0]
    res = dict(label=label, alignments=len(stage), stages=stage_report(stage), no_diag_stages=stage_report(nstage), differ=int(differ.sum()),
               disagree=len(disagree), banded_certs_checked_by_no_diag=cert_checked, banded_certs_in_both=len(both_cert),
               oracle_alignments=len(tasks), stage=stage, timing=t, batch=batch, n_barcodes=nb, banded=prod, differ_mask=differ)
    log("%s (%s): %d alignments; banded != full on %d\n  production stages %s\n  no-diag stages    %s\n"
        "  no-diag run (child process, batch rebuilt): %.1f s\n"
        "  banded-score certificates checked against the no-diag run: %d; decided by one in both runs (to the oracle; none by construction): %d\n"
        "  the two device runs disagree on %d; oracle: %d alignments compared, %d production / %d no-diag mismatches" % (
            name, label, len(stage), res["differ"], res["stages"], res["no_diag_stages"], t_child, cert_checked, len(both_cert), len(disagree),
            len(tasks), len(bad_p), len(bad_n)))
    if bad_p.size or bad_n.size:
        k = (bad_p if bad_p.size else bad_n)[0]
        tk = tasks[k]
        raise AssertionError("%s: task %d: production %d (%s), no-diag %d (%s), oracle %d" % (
            name, tk, prod[tk], abi.STAGE_NAMES.get(int(stage[tk])), ref_nd[tk], abi.STAGE_NAMES.get(int(nstage[tk])), want[k]))
    assert disagree.size == 0, "%s: the production and the no-diag run disagree on %d alignments, first task %d: %d (stage %s) vs %d (stage %s)" % (
        name, disagree.size, disagree[0], prod[disagree[0]], abi.STAGE_NAMES.get(int(stage[disagree[0]])), ref_nd[disagree[0]],
        abi.STAGE_NAMES.get(int(nstage[disagree[0]])))
    return res
