"""Two builds of the drop-in CLI against each other at config-3 scale: tools/e2e_cli_bench.py's authored BAM (--fast --loci 100000
--reads 256 --barcodes 10000), its 3 s pause in front of every run, the two binaries alternating, `Total since launch` (main() to
exit) per run: six runs per side with --ingest device (after one unrecorded run that warms the page cache), three per side with
--ingest host.  Criterion for a change that should cost nothing: this build's median does not exceed the baseline's by more than the
baseline's own max - min.  GPU box:   python tools/e2e_ab.py --baseline-cli <other build>/vartrix_amd/bin/vartrix --json OUT.json"""
import argparse, hashlib, json, os, re, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import e2e_cli_bench as E

ap = argparse.ArgumentParser()
ap.add_argument("--baseline-cli", required=True, help="bin/vartrix of the build to compare with (next to its libraries)")
ap.add_argument("--json", required=True)
ap.add_argument("--out", default="/tmp/e2e")
args = ap.parse_args()
out_dir = args.out
os.makedirs(out_dir, exist_ok=True)
t0 = time.time()
fa, vcf, bam, bcs, n_reads = E.author_fast(out_dir, 100000, 256, 10000, procs=16)
print("authored %d reads in %.1f s (%.1f MB BAM)" % (n_reads, time.time() - t0, os.path.getsize(bam) / 1e6), flush=True)
clis = {"parent": os.path.abspath(args.baseline_cli), "feature": os.path.join(ROOT, "vartrix_amd", "bin", "vartrix")}
res = {}


def run(side, extra, key):
    out = os.path.join(out_dir, "out.mtx")
    for f in (out, os.path.join(out_dir, "ref_matrix.mtx")):
        if os.path.exists(f):
            os.remove(f)
    time.sleep(3.0)
    r = subprocess.run(["timeout", "-k", "10", "120", clis[side], "-v", vcf, "-b", bam, "-f", fa, "-c", bcs, "-o", out, "--threads", "16", "--log-level", "info"] + extra,
                       cwd=out_dir, capture_output=True, text=True)
    if r.returncode != 0:
        print(side, extra, "rc", r.returncode, (r.stdout + r.stderr)[-800:], flush=True)
        sys.exit(1)
    total = float(re.search(r"Total since launch: ([\d.]+) s", r.stderr).group(1))
    sha = hashlib.sha256(open(out, "rb").read()).hexdigest()[:16]
    ing = [ln.strip() for ln in r.stderr.splitlines() if "inflate" in ln and "ms" in ln][:1]
    res.setdefault(key, {}).setdefault(side, []).append(total)
    res.setdefault("sha", set()).add(sha)
    print("%s %s: %.3f s  sha %s  %s" % (side, " ".join(extra), total, sha, ing[0][-160:] if ing else ""), flush=True)


run("feature", ["--ingest", "device"], "warm")                     # page cache, not recorded as a run of either side
for k in range(6):
    for side in (("parent", "feature") if k % 2 == 0 else ("feature", "parent")):
        run(side, ["--ingest", "device"], "device")
for k in range(3):
    for side in (("parent", "feature") if k % 2 == 0 else ("feature", "parent")):
        run(side, ["--ingest", "host"], "host")
summary = {"bam_bytes": os.path.getsize(bam), "reads": n_reads, "mtx_sha256_16": sorted(res.pop("sha"))}
for key in ("device", "host"):
    for side, v in res[key].items():
        summary["%s_%s_s" % (key, side)] = v
        summary["%s_%s_median_s" % (key, side)] = statistics.median(v)
p = summary["device_parent_s"]
summary["device_parent_spread_s"] = round(max(p) - min(p), 4)
summary["device_median_difference_s"] = round(summary["device_feature_median_s"] - summary["device_parent_median_s"], 4)
summary["criterion_met"] = summary["device_median_difference_s"] <= summary["device_parent_spread_s"]
print("summary: " + json.dumps(summary), flush=True)
json.dump(summary, open(args.json, "w"), indent=1)
