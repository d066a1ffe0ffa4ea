#!/usr/bin/env python3
"""The host packer, this tree's libvtxhost.so against another build's (the parent commit's): vtxh_pack_files_raw, vtxh_pack_files and
vtxh_plan_ingest on one authored input (author_fast of tools/e2e_cli_bench.py; config 3 = --loci 100000 --reads 256 --barcodes 10000
where the machine has the memory, else a stated fraction of the loci).

Every run is a fresh process that loads ONE library, times the C call alone (no copy of the pack into numpy) with VTXH_PROFILE on and
prints the seconds and the phases; the runs alternate between the two libraries.  Per call and build: the median, the spread
(max - min) and the phases' medians; `within` says whether this tree's median lies within the other build's own spread of its median.
With --parent-cli (a GPU at hand): the CLI of both builds on the same input, main() to exit, and the sha256 of their .mtx files.

    python tools/host_pack_bench.py --parent-lib /path/to/parent/libvtxhost.so --json profiles/r12_host_pack_stages.json"""
import argparse
import ctypes as C
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CALLS = ("pack_files_raw", "pack_files", "plan_ingest")


def granted_threads():
    n = len(os.sched_getaffinity(0))
    for k in ("OMP_NUM_THREADS", "MAX_JOBS"):
        if os.environ.get(k, "").isdigit():
            n = min(n, int(os.environ[k]))
    return max(1, min(n, 16))


def child(lib, call, vcf, bam, fasta, bcs, threads):
    from vartrix_amd import abi, hostlib
    hostlib.LIB_PATH = lib
    L = hostlib.load()
    args = hostlib.VtxhArgs(vcf.encode(), bam.encode(), fasta.encode(), bcs.encode(), 100, 0, 0, 0, 0, b"CB", b"ATGCatgc", threads,
                            abi.READS_NIBBLES if call == "plan_ingest" else abi.READS_BYTES)
    h = C.c_void_p()
    t0 = time.perf_counter()
    if call == "plan_ingest":
        rc = L.vtxh_plan_ingest(C.byref(args), 0, 0xFFFFFFFF, C.byref(h))
    else:
        rc = (L.vtxh_pack_files_raw if call == "pack_files_raw" else L.vtxh_pack_files)(C.byref(args), C.byref(h))
    dt = time.perf_counter() - t0
    if rc != 0:
        sys.exit("%s: %s" % (call, L.vtxh_last_error().decode()))
    st = (C.c_uint64 * 3)()
    L.vtxh_get_ingest_stats(h, C.byref(st))
    kind = int(L.vtxh_plan_kind(h)) if call == "plan_ingest" else None
    L.vtxh_free(h)
    print("RESULT " + json.dumps(dict(seconds=dt, blocks_inflated=int(st[0]), blocks_total=int(st[1]), plan_kind=kind)), flush=True)


def one_run(lib, call, inputs, threads):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, call] + list(inputs) + [str(threads)],
                       capture_output=True, text=True, env=dict(os.environ, VTXH_PROFILE="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(re.search(r"^RESULT (.*)$", r.stdout, re.M).group(1))
    res["phases"] = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"^\[vtxh\] (.+?)\s+([\d.]+) s$", r.stderr, re.M)}
    m = re.search(r"record index ([\d.]+) s \(one thread\), parse ([\d.]+) s", r.stderr)
    if m:
        res["side_by_side"] = dict(record_index=float(m.group(1)), parse=float(m.group(2)))
    return res


def summary(runs):
    s = [r["seconds"] for r in runs]
    names = sorted({k for r in runs for k in r["phases"]})
    out = dict(median=statistics.median(s), spread=max(s) - min(s), seconds=s,
               phases={k: statistics.median([r["phases"].get(k, 0.0) for r in runs]) for k in names})
    if all("side_by_side" in r for r in runs):
        out["side_by_side"] = {k: statistics.median([r["side_by_side"][k] for r in runs]) for k in ("record_index", "parse")}
    for k in ("blocks_inflated", "blocks_total", "plan_kind"):
        out[k] = runs[0][k]
    return out


def cli_runs(clis, inputs, threads, runs, out_dir):
    fa, vcf, bam, bcs = inputs
    res = {name: dict(seconds=[], sha256=None) for name in clis}
    for _ in range(runs):
        for name, cli in clis.items():
            out = os.path.join(out_dir, "out_%s.mtx" % name)
            t0 = time.perf_counter()
            r = subprocess.run([cli, "-v", vcf, "-b", bam, "-f", fa, "-c", bcs, "-o", out, "--threads", str(threads)], cwd=out_dir,
                               capture_output=True, text=True)
            res[name]["seconds"].append(time.perf_counter() - t0)
            assert r.returncode == 0, r.stdout + r.stderr
            res[name]["sha256"] = hashlib.sha256(open(out, "rb").read()).hexdigest()
            os.remove(out)
    for v in res.values():
        v["median"], v["spread"] = statistics.median(v["seconds"]), max(v["seconds"]) - min(v["seconds"])
    res["same_mtx"] = len({v["sha256"] for v in res.values()}) == 1
    return res


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3], *sys.argv[4:8], int(sys.argv[8]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libvtxhost.so of the commit to compare with")
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--parent-cli", default=None, help="its bin/vartrix (next to its libraries): also time the CLI of both builds (needs a GPU)")
    ap.add_argument("--loci", type=int, default=100000)
    ap.add_argument("--reads", type=int, default=256)
    ap.add_argument("--barcodes", type=int, default=10000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=granted_threads())
    ap.add_argument("--out", default="/tmp/vtx_host_pack_bench", help="the authored input is kept there and used again")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert a.runs >= 5
    from vartrix_amd import hostlib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from e2e_cli_bench import author_fast
    # the raw pack of config 3 holds ~10 GB (reads as bytes, tags, hits, the window's buffers) beside 0.9 GB of page cache
    avail = next(int(ln.split()[1]) for ln in open("/proc/meminfo") if ln.startswith("MemAvailable")) >> 20
    need = 24 * a.loci * a.reads / 2.56e7
    fraction = 1.0 if avail >= need else max(0.01, avail / need)
    loci = int(a.loci * fraction)
    os.makedirs(a.out, exist_ok=True)
    tag = os.path.join(a.out, "authored_%d_%d_%d" % (loci, a.reads, a.barcodes))
    names = [os.path.join(a.out, n) for n in ("g.fa", "v.vcf", "r.bam", "bcs.tsv")]
    if not os.path.exists(tag):
        author_fast(a.out, loci, a.reads, a.barcodes, procs=a.threads)
        open(tag, "w").close()
    fa, vcf, bam, bcs = names
    inputs = (vcf, bam, fa, bcs)
    hostlib.use_variant("")
    libs = {"parent": os.path.abspath(a.parent_lib), "this": hostlib.LIB_PATH}
    result = dict(input=dict(loci=loci, reads_per_locus=a.reads, barcodes=a.barcodes, fraction_of_the_loci_asked_for=fraction,
                             bam_bytes=os.path.getsize(bam)), threads=a.threads, runs=a.runs, parent_commit=a.parent_commit, calls={})
    for call in CALLS:
        one_run(libs["this"], call, inputs, a.threads)                    # (page cache and the allocator's first pages: not counted)
        runs = {k: [] for k in libs}
        for _ in range(a.runs):
            for k in ("parent", "this"):
                runs[k].append(one_run(libs[k], call, inputs, a.threads))
        c = {k: summary(v) for k, v in runs.items()}
        c["within"] = abs(c["this"]["median"] - c["parent"]["median"]) <= c["parent"]["spread"]
        result["calls"][call] = c
        print("%-15s parent %.3f s (spread %.3f)   this %.3f s (spread %.3f)   within the parent's spread: %s" %
              (call, c["parent"]["median"], c["parent"]["spread"], c["this"]["median"], c["this"]["spread"], c["within"]), flush=True)
    if a.parent_cli:
        result["cli"] = cli_runs({"parent": os.path.abspath(a.parent_cli), "this": hostlib.cli_path()}, (fa, vcf, bam, bcs), a.threads, a.runs, a.out)
        print("CLI main() to exit: parent %.3f s, this %.3f s, same .mtx: %s" %
              (result["cli"]["parent"]["median"], result["cli"]["this"]["median"], result["cli"]["same_mtx"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
