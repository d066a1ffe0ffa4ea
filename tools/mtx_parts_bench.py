"""The output stage of a STREAMED run, this build against a build of the parent commit, at config-3 scale: tools/e2e_cli_bench.py's
authored BAM (--fast --loci 100000 --reads 256 --barcodes 10000), consensus mode, --ingest device, --stream-loci 25000 (four ranges) plain
and with --gzip — where this build writes the matrix from the device in parts (vtx_mtx_part / vtx_mtx_join) and the parent fetches the
triplets and formats on the host — and --stream-loci 0 (one range: the unchanged vtx_write_mtx path) as the control.  tools/e2e_ab.py's
rules: a 3 s pause in front of every run, the two binaries alternating, `Total since launch` (main() to exit) and the log's
`Merge + output files` per run, after one unrecorded run that warms the page cache.  Expectations, evaluated and written down, never tuned:
the streamed --gzip median is below the parent's by more than the parent's own max - min; the streamed plain median and the whole-input
median do not exceed the parent's by more than the parent's max - min; the .mtx sha256 is equal per configuration (with --gzip: of the
decompressed bytes — the compressed bytes differ by design, the parent's come from zlib).
GPU box:   python tools/mtx_parts_bench.py --baseline-cli <parent build>/vartrix_amd/bin/vartrix --json profiles/r11_mtx_parts.json"""
import argparse, gzip, hashlib, json, os, re, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import e2e_cli_bench as E

ap = argparse.ArgumentParser()
ap.add_argument("--baseline-cli", required=True, help="bin/vartrix of a build of the parent commit (next to its libraries)")
ap.add_argument("--baseline-commit", default=None, help="that commit's name, for the record")
ap.add_argument("--json", required=True)
ap.add_argument("--out", default="/tmp/e2e")
ap.add_argument("--runs", type=int, default=5, help="recorded runs per side and configuration")
ap.add_argument("--procs", type=int, default=16)
args = ap.parse_args()
out_dir = args.out
os.makedirs(out_dir, exist_ok=True)
t0 = time.time()
fa, vcf, bam, bcs, n_reads = E.author_fast(out_dir, 100000, 256, 10000, procs=args.procs)
print("authored %d reads in %.1f s (%.1f MB BAM)" % (n_reads, time.time() - t0, os.path.getsize(bam) / 1e6), flush=True)
clis = {"parent": os.path.abspath(args.baseline_cli), "feature": os.path.join(ROOT, "vartrix_amd", "bin", "vartrix")}
CONFIGS = {"streamed_gzip": ["--ingest", "device", "--stream-loci", "25000", "--gzip"],
           "streamed_plain": ["--ingest", "device", "--stream-loci", "25000"],
           "whole_plain": ["--ingest", "device", "--stream-loci", "0"]}
res = {k: {"parent": [], "feature": []} for k in CONFIGS}


def run(side, key, record=True):
    extra = CONFIGS[key]
    out = os.path.join(out_dir, "out.mtx.gz" if "--gzip" in extra else "out.mtx")
    for f in (out, os.path.join(out_dir, "ref_matrix.mtx")):
        if os.path.exists(f):
            os.remove(f)
    time.sleep(3.0)
    r = subprocess.run(["timeout", "-k", "10", "120", clis[side], "-v", vcf, "-b", bam, "-f", fa, "-c", bcs, "-o", out, "--threads", "16", "--log-level", "info"] + extra,
                       cwd=out_dir, capture_output=True, text=True)
    if r.returncode != 0:
        print(side, extra, "rc", r.returncode, (r.stdout + r.stderr)[-800:], flush=True)
        sys.exit(1)
    data = open(out, "rb").read()
    one = {"total_s": float(re.search(r"Total since launch: ([\d.]+) s", r.stderr).group(1)),
           "output_s": float(re.search(r"Merge \+ output files: ([\d.]+) s", r.stderr).group(1)),
           "device_s": float(re.search(r"Device \(create \+ submit \+ run \+ fetch\) on 1 GPU\(s\): ([\d.]+) s", r.stderr).group(1)),
           "ranges": len(re.findall(r"Plan of range \d+", r.stderr)),
           "writer": re.search(r"Matrix written (.*)", r.stderr).group(1),
           "file_bytes": len(data), "sha256_16": hashlib.sha256(data).hexdigest()[:16]}
    if "--gzip" in extra:
        one["decompressed_sha256_16"] = hashlib.sha256(gzip.decompress(data)).hexdigest()[:16]
    if record:
        res[key][side].append(one)
    print("%s %s: total %.3f s, output %.3f s, device %.3f s, %d range(s), %s, sha %s" % (side, key, one["total_s"], one["output_s"], one["device_s"], one["ranges"],
                                                                                          one["writer"], one.get("decompressed_sha256_16", one["sha256_16"])), flush=True)


run("feature", "whole_plain", record=False)                     # page cache, not recorded as a run of either side
for key in CONFIGS:
    for k in range(args.runs):
        for side in (("parent", "feature") if k % 2 == 0 else ("feature", "parent")):
            run(side, key)
summary = {"what": "streamed output stage, this build (matrix written from the device in parts) against the parent commit (triplets fetched, host formatter): "
                   "drop-in CLI on the authored config-3-scale BAM, consensus, --ingest device --threads 16; seconds from main() to exit ('Total since launch'), the "
                   "log's 'Merge + output files' and 'Device (create + submit + run + fetch)'; alternating runs, 3 s pause in front of each (tools/mtx_parts_bench.py)",
           "baseline_commit": args.baseline_commit, "bam_bytes": os.path.getsize(bam), "reads": n_reads, "runs_per_side": args.runs, "configs": {}}
for key, sides in res.items():
    c = {"flags": " ".join(CONFIGS[key])}
    for side, runs in sides.items():
        for f in ("total_s", "output_s", "device_s"):
            c["%s_%s" % (side, f)] = [x[f] for x in runs]
            c["%s_%s_median" % (side, f[:-2])] = statistics.median(x[f] for x in runs)
        c["%s_writer" % side] = sorted({x["writer"] for x in runs})
        c["%s_file_bytes" % side] = sorted({x["file_bytes"] for x in runs})
    sha_key = "decompressed_sha256_16" if "--gzip" in CONFIGS[key] else "sha256_16"
    shas = {x[sha_key] for runs in sides.values() for x in runs}
    c[sha_key] = sorted(shas)
    c["sha256_equal"] = len(shas) == 1
    p = c["parent_total_s"]
    c["parent_total_spread_s"] = round(max(p) - min(p), 4)
    c["total_median_difference_s"] = round(c["feature_total_median"] - c["parent_total_median"], 4)
    if key == "streamed_gzip":
        c["expectation"] = "feature median below the parent's by more than the parent's max - min"
        c["expectation_met"] = -c["total_median_difference_s"] > c["parent_total_spread_s"]
    else:
        c["expectation"] = "feature median does not exceed the parent's by more than the parent's max - min"
        c["expectation_met"] = c["total_median_difference_s"] <= c["parent_total_spread_s"]
    summary["configs"][key] = c
print("summary: " + json.dumps(summary), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
json.dump(summary, open(args.json, "w"), indent=1)
