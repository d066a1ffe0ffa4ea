"""vtx_write_mtx_f64: alt_frac's Matrix-Market text formatted on the device (mtx_len_kernel<true> / mtx_text_kernel<true>,
vartrix_amd/csrc/vtx_ingest.hip, per-lane formatter vtx_f64_text.h) — the bytes sprs::io::write_matrix_market writes
(src/main.rs:381-389, values from :1131-1145: Rust's `{}` of an f64, shortest round-trip digits, NaN), i.e. what vtxh_write_mtx writes
from the fetched triplets.  The per-value logic is covered exhaustively on the CPU (tests/test_f64_text.py, same source); here the
kernels, the slab loop, the C-ABI, the binding and the command line.  An out-of-domain value cannot be produced by vtx_run: the decline
path is the CPU suite's (length 0) and tests/test_gpu_ingest.py's (vtx_write_mtx on alt_frac)."""
import math
import os
import subprocess

import numpy as np
import pytest

from vartrix_amd import hostlib, lib, synth
from vartrix_amd.abi import default_config

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def text_spec():
    """The batch of tests/test_gpu_ingest.py::test_matrix_market_text_from_the_device."""
    return synth.SynthSpec(n_loci=700, n_barcodes=900, reads_per_locus=40, indel_frac=0.2, use_umi=True, seed=5)


def config5_spec():
    """BASELINE.json configs[4]'s shape (30 % indel loci <= 20 bp, UMIs, 256 reads per locus) over few cells — several UMIs per (locus, cell)
    group, so that the fractions are not only 0 and 1 — and with reads down to 15 bases: a group whose reads all score under the
    threshold of 25 is 0 / 0 = NaN."""
    return synth.SynthSpec(n_loci=3000, n_barcodes=40, indel_frac=0.30, use_umi=True, read_len_jitter=135)


@pytest.fixture(scope="module")
def config5_batch():
    spec = config5_spec()
    return spec, synth.make_batch(spec)


def check_sum(s, values):
    """*sum: NaN when a value is NaN (the host's `sum += v`), else the sum of the values, added up in no fixed order."""
    values = np.asarray(values)
    if np.isnan(values).any():
        assert math.isnan(s)
    else:
        assert s == pytest.approx(float(values.sum()), rel=1e-9, abs=0.0)


def test_alt_frac_text_equals_the_host_writer(tmp_path):
    spec = text_spec()
    batch = synth.make_batch(spec)
    with lib.Context(default_config(scoring_mode="alt_frac", use_umi=1, n_barcodes=spec.n_barcodes)) as ctx:
        ctx.submit(batch)
        ctx.run()
        coo = ctx.fetch_coo()
        p, q = str(tmp_path / "dev.mtx"), str(tmp_path / "host.mtx")
        s = ctx.write_mtx(p, spec.n_loci, spec.n_barcodes, 0, real=True)
        hostlib.write_mtx(q, spec.n_loci, spec.n_barcodes, coo["row"], coo["col"], coo["value"])
        assert open(p, "rb").read() == open(q, "rb").read()
        v = coo["value"]
        assert len(v) > 5000 and ((v > 0) & (v < 1)).any() and (v == 0).any() and (v == 1).any()
        check_sum(s, v)
        # which = 1: alt_frac's ref_value column (zeros)
        s1 = ctx.write_mtx(p, spec.n_loci, spec.n_barcodes, 1, real=True)
        hostlib.write_mtx(q, spec.n_loci, spec.n_barcodes, coo["row"], coo["col"], coo["ref_value"])
        assert open(p, "rb").read() == open(q, "rb").read()
        check_sum(s1, coo["ref_value"])


def test_config5_shape_text_equals_the_host_writer(tmp_path, config5_batch):
    """>= 10^5 triplets with NaN, 0, 1, thirds and sevenths among them; then the same matrix through libvtx_dev.so in passes of a few
    thousand lines (VTX_MTX_SLAB: the slab loop, several passes): identical file."""
    spec, batch = config5_batch
    assert len(np.unique(batch.loci["ref_len"].astype(np.int64) - batch.loci["alt_len"])) > 10      # indels both ways
    cfg = default_config(scoring_mode="alt_frac", use_umi=1, n_barcodes=spec.n_barcodes)
    p, q, d = str(tmp_path / "dev.mtx"), str(tmp_path / "host.mtx"), str(tmp_path / "slab.mtx")
    with lib.Context(cfg) as ctx:
        ctx.submit(batch)
        ctx.run()
        coo = ctx.fetch_coo()
        s = ctx.write_mtx(p, spec.n_loci, spec.n_barcodes, 0, real=True)
    v = coo["value"]
    assert len(v) >= 100_000
    assert np.isnan(v).any() and (v == 0).any() and (v == 1).any()
    for den in (3, 7):
        assert any((v == a / den).any() for a in range(1, den)), den
    hostlib.write_mtx(q, spec.n_loci, spec.n_barcodes, coo["row"], coo["col"], v)
    want = open(q, "rb").read()
    assert open(p, "rb").read() == want
    assert b" NaN\n" in want and b" 0.3333333333333333\n" in want
    check_sum(s, v)
    old = os.environ.get("VTX_MTX_SLAB")
    os.environ["VTX_MTX_SLAB"] = "4099"                  # (read by libvtx_dev.so at every call)
    try:
        with lib.Context(cfg, variant="dev") as ctx:
            ctx.submit(batch)
            ctx.run()
            s2 = ctx.write_mtx(d, spec.n_loci, spec.n_barcodes, 0, real=True)
    finally:
        if old is None:
            del os.environ["VTX_MTX_SLAB"]
        else:
            os.environ["VTX_MTX_SLAB"] = old
    assert len(v) > 20 * 4099 and open(d, "rb").read() == want
    check_sum(s2, v)


@pytest.mark.parametrize("mode", ["consensus", "coverage"])
def test_integral_matrices_are_unchanged(tmp_path, mode):
    """consensus / coverage through vtx_write_mtx_f64: the bytes and the sum of vtx_write_mtx."""
    spec = text_spec()
    batch = synth.make_batch(spec)
    with lib.Context(default_config(scoring_mode=mode, use_umi=1, n_barcodes=spec.n_barcodes)) as ctx:
        ctx.submit(batch)
        ctx.run()
        for which in (0, 1):
            p, q = str(tmp_path / ("real%d.mtx" % which)), str(tmp_path / ("int%d.mtx" % which))
            s = ctx.write_mtx(p, spec.n_loci, spec.n_barcodes, which, real=True)
            t = ctx.write_mtx(q, spec.n_loci, spec.n_barcodes, which)
            a = open(p, "rb").read()
            assert a == open(q, "rb").read() and a.count(b"\n") > 5000 and s == t


def test_cli_alt_frac_is_written_from_the_device(tmp_path):
    """`vartrix -s alt_frac` (one GPU, one batch): the matrix comes from vtx_write_mtx_f64 — the log says so — and equals the reference's
    test_frac.mtx (src/main.rs:1236-1263) byte for byte."""
    if not (os.path.exists(hostlib.CLI_PATH) and os.path.exists(hostlib.LIB_PATH) and os.path.exists(lib.LIB_PATH)):
        import __graft_entry__
        __graft_entry__.build()
    out = str(tmp_path / "out.mtx")
    r = subprocess.run([hostlib.CLI_PATH, "-v", os.path.join(G, "test.vcf"), "-b", os.path.join(G, "test.bam"), "-f", os.path.join(G, "test.fa"),
                        "-c", os.path.join(G, "barcodes.tsv"), "-o", out, "-s", "alt_frac", "--log-level", "info"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Matrix written from the device (vtx_write_mtx_f64)" in r.stderr, r.stderr
    assert "host formatter" not in r.stderr
    assert open(out, "rb").read() == open(os.path.join(G, "test_frac.mtx"), "rb").read()
