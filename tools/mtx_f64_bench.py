#!/usr/bin/env python3
"""alt_frac's Matrix-Market text: the device writer (vtx_write_mtx_f64) against the host path it replaces in the CLI (vtx_fetch_coo +
vtxh_write_mtx), same matrix, same process, same filesystem.

  python tools/mtx_f64_bench.py --out profiles/r08_mtx_f64.json
      (1) wall time per side: one warm-up each, then --runs alternating pairs; median / min / max.  The files go to --dir (default:
          /dev/shm when it exists — page-cache copies, so that a disk is not what is compared).  The bytes of both files are compared.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mtx -- python tools/mtx_f64_bench.py --kernels-only
  python tools/mtx_f64_bench.py --stats DIR/mtx_kernel_stats.csv --merge profiles/r08_mtx_f64.json
      (2) a run of its own under the profiler: the real-value kernels (alt_frac's `value`) next to the integral kernels on the integral
          matrix of the same batch (alt_frac's `ref_value`: the same rows and columns, every value 0) -> ns per line, text bytes per second.

The batch is BASELINE.json configs[4]'s shape (synth.config5: 30 % indel loci <= 20 bp, UMIs, 10 000 barcodes, 256 reads per locus);
--loci sets its size (alt_frac emits every (locus, cell) group: ~240 lines per locus)."""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_stats(path, nnz_lines, real_bytes, int_bytes):
    """rocprofv3's <prefix>_kernel_stats.csv -> per-kernel calls / average ns / ns per line / text bytes per second."""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Name"]
            for key, pat, nbytes in (("mtx_len_kernel<real>", "mtx_len_kernel<true>", real_bytes), ("mtx_text_kernel<real>", "mtx_text_kernel<true>", real_bytes),
                                     ("mtx_len_kernel<integral>", "mtx_len_kernel<false>", int_bytes), ("mtx_text_kernel<integral>", "mtx_text_kernel<false>", int_bytes)):
                if pat in name:
                    avg = float(row["AverageNs"])
                    out[key] = {"calls": int(row["Calls"]), "average_ns": avg, "min_ns": float(row["MinNs"]), "max_ns": float(row["MaxNs"]),
                                "ns_per_line": avg / nnz_lines, "text_bytes_per_s": nbytes / (avg * 1e-9)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--loci", type=int, default=60000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="three calls per writer and nothing else: the run under rocprofv3")
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of a --kernels-only run")
    ap.add_argument("--merge", default=None, help="JSON of a timing run to add the --stats digest to")
    a = ap.parse_args()

    if a.stats:
        doc = json.load(open(a.merge))
        doc["kernels"] = kernel_stats(a.stats, doc["nnz"], doc["text_bytes"] - doc["header_bytes"], doc["integral_text_bytes"] - doc["header_bytes"])
        doc["kernels_command"] = "rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mtx -- python tools/mtx_f64_bench.py --kernels-only --loci %d" % doc["loci"]
        json.dump(doc, open(a.merge, "w"), indent=1)
        print(json.dumps(doc["kernels"]))
        return

    import numpy as np
    from vartrix_amd import hostlib, lib, synth
    from vartrix_amd.abi import default_config

    spec = synth.config5(a.loci)
    t0 = time.perf_counter()
    batch = synth.make_batch(spec)
    print("batch: %s, %d records (%.1f s)" % (spec.name, batch.n_records, time.perf_counter() - t0), file=sys.stderr)
    cfg = default_config(aligner="banded", scoring_mode="alt_frac", use_umi=1, n_barcodes=spec.n_barcodes)
    with tempfile.TemporaryDirectory(dir=a.dir) as td, lib.Context(cfg) as ctx:
        dev, host, integral = (os.path.join(td, n) for n in ("dev.mtx", "host.mtx", "int.mtx"))
        ctx.submit(batch)
        ctx.run()

        def device_side():
            t = time.perf_counter()
            ctx.write_mtx(dev, spec.n_loci, spec.n_barcodes, 0, real=True)          # (returns after the last pwrite: synchronous)
            return time.perf_counter() - t

        def host_side():
            t = time.perf_counter()
            coo = ctx.fetch_coo()
            t1 = time.perf_counter()
            hostlib.write_mtx(host, spec.n_loci, spec.n_barcodes, coo["row"], coo["col"], coo["value"])
            return time.perf_counter() - t, t1 - t

        if a.kernels_only:
            for _ in range(3):
                ctx.write_mtx(dev, spec.n_loci, spec.n_barcodes, 0, real=True)
                ctx.write_mtx(integral, spec.n_loci, spec.n_barcodes, 1)
            return
        device_side(); host_side()                                                  # warm: code objects, pinned buffers, page cache
        nnz = len(ctx.fetch_coo()["row"])
        same = open(dev, "rb").read() == open(host, "rb").read()
        td_, th_, tf_ = [], [], []
        for _ in range(a.runs):
            td_.append(device_side())
            h, f = host_side()
            th_.append(h); tf_.append(f)
        ctx.write_mtx(integral, spec.n_loci, spec.n_barcodes, 1)
        v = ctx.fetch_coo()["value"]
        head = len(("%%%%MatrixMarket matrix coordinate real general\n%% written by sprs\n%u %u %u\n" % (spec.n_loci, spec.n_barcodes, nnz)).encode())
        doc = {
            "what": "alt_frac Matrix-Market text of one resident batch: vtx_write_mtx_f64 (device) vs vtx_fetch_coo + vtxh_write_mtx (host, the parent commit's path)",
            "command": "python tools/mtx_f64_bench.py --loci %d --runs %d" % (a.loci, a.runs),
            "workload": spec.name, "loci": a.loci, "nnz": int(nnz), "text_bytes": os.path.getsize(dev), "integral_text_bytes": os.path.getsize(integral),
            "header_bytes": head, "files_on": td, "byte_identical": bool(same),
            "values": {"nan": int(np.isnan(v).sum()), "zero": int((v == 0).sum()), "one": int((v == 1).sum()), "fractions": int(((v > 0) & (v < 1)).sum())},
            "runs_per_side": a.runs, "order": "alternating, device first, after one warm-up per side",
            "device_s": {"median": statistics.median(td_), "min": min(td_), "max": max(td_), "all": td_},
            "host_s": {"median": statistics.median(th_), "min": min(th_), "max": max(th_), "all": th_, "fetch_median": statistics.median(tf_)},
            "host_over_device": statistics.median(th_) / statistics.median(td_),
        }
        assert same, "device and host files differ"
    line = json.dumps(doc)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(doc, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
