#!/usr/bin/env python3
"""The gzip-compressed Matrix-Market output (vtx_write_mtx_gz): compressed size against zlib level 1, and time against the plain
device writer and the host's gzip writer.  Results: profiles/r10_mtx_gz.json.

  python tools/mtx_gz_bench.py --size --merge profiles/r10_mtx_gz.json
      (1) CPU only.  The HOST build of the encoder (tests/deflatecore/deflate_host; the device's bytes are identical, pinned by
          tests/test_gpu_mtx_gz.py) against zlib's raw deflate at level 1 over the same 65 280-byte chunks of three texts: the consensus
          and the coverage text of a model of BASELINE.json configs[2]'s matrix (--size-loci rows, 10 000 barcodes, 256 reads per locus
          spread over the cells as synth.py spreads them: ~250 lines per row, columns ascending), and 200 000 lines of alt_frac-like text
          with NaN, thirds and 7-digit row numbers.
  python tools/mtx_gz_bench.py --merge profiles/r10_mtx_gz.json [--parent-variant parent]
      (2) on the GPU, one process, synth.config3 (consensus): vtx_write_mtx, vtx_write_mtx_gz and vtx_fetch_coo + vtxh_write_mtx_gz
          (16 threads), one warm-up each, then --runs rounds in that order; median / min / max.  --parent-variant NAME: also
          vtx_write_mtx of vartrix_amd/libvtx_NAME.so, a build of the parent commit, in the same rounds.  Files go to --dir (default
          /dev/shm: page-cache copies).  The real text's sizes (gz file, zlib level 1 over the same chunks) are recorded too.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o gz -- python tools/mtx_gz_bench.py --kernels-only
  python tools/mtx_gz_bench.py --stats DIR/gz_kernel_stats.csv --merge profiles/r10_mtx_gz.json
      (3) a run of its own under the profiler: mtx_deflate_kernel's and mtx_gz_compact_kernel's device time."""
import argparse
import csv
import gzip
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK = 65280


def zlib1_bytes(text):
    total = 0
    for i in range(0, len(text), CHUNK):
        z = zlib.compressobj(1, zlib.DEFLATED, -15)
        total += len(z.compress(text[i:i + CHUNK])) + len(z.flush())
    return total


def host_encoder_bytes(text, td):
    """DEFLATE bytes (members without their 26 bytes of framing) of the host build of vtx_deflate_core.h."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "deflatecore"), "-s", "deflate_host"])
    src, dst = os.path.join(td, "t.bin"), os.path.join(td, "t.gz")
    open(src, "wb").write(text)
    subprocess.check_call([os.path.join(ROOT, "tests", "deflatecore", "deflate_host"), "--file", src, dst])
    z = open(dst, "rb").read()
    assert gzip.decompress(z) == text
    n_members = (len(text) + CHUNK - 1) // CHUNK
    return len(z) - 28 - 26 * n_members


def size_texts(n_loci, td):
    import numpy as np
    from vartrix_amd import hostlib
    rng = np.random.default_rng(3)
    n_bc, reads = 10_000, 256
    cells = rng.integers(0, n_bc, (n_loci, reads))
    key = np.unique(np.repeat(np.arange(n_loci, dtype=np.int64), reads) * n_bc + cells.ravel(), return_counts=True)
    row, col, cnt = (key[0] // n_bc).astype(np.uint32), (key[0] % n_bc).astype(np.uint32), key[1]
    geno = rng.integers(0, 3, len(row))                         # a cell is hom-ref, het or hom-alt at a locus
    alt = np.where(geno == 0, 0, np.where(geno == 2, cnt, rng.binomial(cnt, 0.5)))
    consensus = np.where(alt == 0, 1.0, np.where(alt == cnt, 2.0, 3.0))
    out = {}
    for name, val in (("consensus", consensus), ("coverage", alt.astype(np.float64))):
        p = os.path.join(td, name + ".mtx")
        hostlib.write_mtx(p, n_loci, n_bc, row, col, val)
        out[name] = open(p, "rb").read()
    n = 200_000
    r2 = np.sort(rng.integers(0, 3_000_000, n)).astype(np.uint32)
    c2 = rng.integers(0, n_bc, n).astype(np.uint32)
    den = rng.integers(1, 8, n)
    v2 = rng.integers(0, 8, n) % (den + 1) / den
    v2[rng.random(n) < 0.02] = np.nan
    v2[rng.random(n) < 0.3] = 1.0 / 3.0
    p = os.path.join(td, "frac.mtx")
    hostlib.write_mtx(p, 3_000_000, n_bc, r2, c2, v2)
    out["alt_frac_200k"] = open(p, "rb").read()
    return out


class ParentWriter:
    """vtx_create / vtx_submit / vtx_run / vtx_write_mtx of ANOTHER build of the library (the parent commit's, which lacks the entry
    points lib.load binds): just these entry points, bound by hand."""

    def __init__(self, path, cfg, batch):
        import ctypes as C
        from vartrix_amd import abi
        self.C, L = C, C.CDLL(path)
        self.L, self.h = L, C.c_void_p()
        for f in (L.vtx_create, L.vtx_set_read_format, L.vtx_submit, L.vtx_run, L.vtx_write_mtx):
            f.restype = C.c_int
        L.vtx_create.argtypes = [C.POINTER(abi.VtxConfig), C.POINTER(C.c_void_p)]
        L.vtx_set_read_format.argtypes = [C.c_void_p, C.c_int]
        L.vtx_submit.argtypes = [C.c_void_p, C.POINTER(abi.VtxBatch)]
        L.vtx_run.argtypes = [C.c_void_p]
        L.vtx_write_mtx.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_double)]
        L.vtx_destroy.restype, L.vtx_destroy.argtypes = None, [C.c_void_p]
        L.vtx_strerror.restype, L.vtx_strerror.argtypes = C.c_char_p, [C.c_void_p]
        self.check(L.vtx_create(C.byref(cfg), C.byref(self.h)))
        st = batch.as_struct()
        self.check(L.vtx_set_read_format(self.h, int(getattr(batch, "read_format", 0))))
        self.check(L.vtx_submit(self.h, C.byref(st)))
        self.check(L.vtx_run(self.h))

    def check(self, rc):
        if rc != 0:
            raise RuntimeError("parent build: %s" % self.L.vtx_strerror(self.h).decode())

    def write_mtx(self, path, n_rows, n_cols):
        s = self.C.c_double(0.0)
        self.check(self.L.vtx_write_mtx(self.h, path.encode(), n_rows, n_cols, 0, self.C.byref(s)))

    def close(self):
        self.L.vtx_destroy(self.h)


def merge(path, key, value):
    doc = json.load(open(path)) if path and os.path.exists(path) else {}
    doc[key] = value
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
    print(json.dumps({key: value}))


def stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", action="store_true")
    ap.add_argument("--size-loci", type=int, default=10_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--loci", type=int, default=100_000)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None)
    ap.add_argument("--merge", default=None)
    ap.add_argument("--parent-variant", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()

    if a.stats:
        out = {}
        with open(a.stats, newline="") as fh:
            for r in csv.DictReader(fh):
                for k in ("mtx_deflate_kernel", "mtx_gz_compact_kernel", "mtx_text_kernel", "mtx_len_kernel"):
                    if k in r["Name"]:
                        out[k] = {"calls": int(r["Calls"]), "average_ns": float(r["AverageNs"]), "min_ns": float(r["MinNs"]), "max_ns": float(r["MaxNs"])}
        merge(a.merge, "kernels", out)
        return

    if a.size:
        with tempfile.TemporaryDirectory() as td:
            res = {}
            for name, text in size_texts(a.size_loci, td).items():
                ours, ref = host_encoder_bytes(text, td), zlib1_bytes(text)
                res[name] = {"lines": text.count(b"\n") - 3, "text_bytes": len(text), "encoder_deflate_bytes": ours, "zlib_level1_deflate_bytes": ref,
                             "encoder_over_zlib1": ours / ref, "encoder_over_text": ours / len(text)}
        merge(a.merge, "compressed_size", {"what": "host build of vtx_deflate_core.h (= the device's bytes) vs zlib raw deflate level 1, same 65 280-byte chunks",
                                           "command": "python tools/mtx_gz_bench.py --size --size-loci %d" % a.size_loci, "texts": res})
        return

    from vartrix_amd import hostlib, lib, synth
    from vartrix_amd.abi import default_config
    spec = synth.config3()
    if a.loci != spec.n_loci:
        spec = synth.SynthSpec(n_loci=a.loci, n_barcodes=spec.n_barcodes)
    t0 = time.perf_counter()
    batch = synth.make_batch(spec)
    print("batch: %d records (%.1f s)" % (batch.n_records, time.perf_counter() - t0), file=sys.stderr, flush=True)
    cfg = default_config(aligner="banded", scoring_mode="consensus", n_barcodes=spec.n_barcodes)
    with tempfile.TemporaryDirectory(dir=a.dir) as td, lib.Context(cfg) as ctx:
        plain, gz, hostgz, pplain = (os.path.join(td, n) for n in ("plain.mtx", "dev.mtx.gz", "host.mtx.gz", "parent.mtx"))
        ctx.submit(batch)
        ctx.run()
        if a.kernels_only:
            for _ in range(3):
                ctx.write_mtx_gz(gz, spec.n_loci, spec.n_barcodes, 0)
            return
        pctx = None
        if a.parent_variant:
            pctx = ParentWriter(lib.lib_path(a.parent_variant), cfg, batch)

        def timed(f):
            t = time.perf_counter()
            f()
            return time.perf_counter() - t

        def host_side():
            coo = ctx.fetch_coo()
            hostlib.write_mtx_gz(hostgz, spec.n_loci, spec.n_barcodes, coo["row"], coo["col"], coo["value"])

        sides = {"vtx_write_mtx": lambda: ctx.write_mtx(plain, spec.n_loci, spec.n_barcodes, 0),
                 "vtx_write_mtx_gz": lambda: ctx.write_mtx_gz(gz, spec.n_loci, spec.n_barcodes, 0),
                 "vtx_fetch_coo+vtxh_write_mtx_gz": host_side}
        if pctx:
            sides["vtx_write_mtx (parent build)"] = lambda: pctx.write_mtx(pplain, spec.n_loci, spec.n_barcodes)
        times = {k: [] for k in sides}
        for k, f in sides.items():
            f()                                                    # warm: code objects, pinned buffers, device buffers, page cache
        for _ in range(a.runs):
            for k, f in sides.items():
                times[k].append(timed(f))
        text = open(plain, "rb").read()
        z = open(gz, "rb").read()
        same = gzip.decompress(z) == text and gzip.decompress(open(hostgz, "rb").read()) == text
        if pctx:
            same = same and open(pplain, "rb").read() == text
            pctx.close()
        n_members = (len(text) + CHUNK - 1) // CHUNK
        doc = {"what": "config-3 consensus matrix of one resident batch, files on %s, %d threads for the host side" % (td, min(16, os.cpu_count() or 1)),
               "command": "python tools/mtx_gz_bench.py --loci %d --runs %d%s" % (a.loci, a.runs, " --parent-variant " + a.parent_variant if a.parent_variant else ""),
               "lines": text.count(b"\n") - 3, "text_bytes": len(text), "gz_file_bytes": len(z), "host_gz_file_bytes": os.path.getsize(hostgz),
               "device_deflate_bytes": len(z) - 28 - 26 * n_members, "zlib_level1_deflate_bytes": zlib1_bytes(text), "decompressed_equal": bool(same),
               "order": "one warm-up each, then rounds in the order listed", "seconds": {k: stat(v) for k, v in times.items()}}
        doc["device_over_zlib1"] = doc["device_deflate_bytes"] / doc["zlib_level1_deflate_bytes"]
        assert same
    merge(a.merge, "time", doc)


if __name__ == "__main__":
    main()
