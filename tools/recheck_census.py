"""Census of the recheck (vtx_fast_core.h: recheck_rest; band_tail_kernel's recheck mode) on batches of bench.py's generator, from the
CPU build of the first stage's per-task logic (tests/fastcore/recheck_host.cpp, compiled here): why the tasks that band_diag_kernel
does not decide leave it, and what the tight harmless test on the same list makes of those that failed the coarse one.
TEST / MEASUREMENT INFRASTRUCTURE (the product never loads it).
    python tools/recheck_census.py [n_loci] [key=value ...]        (keys of synth.SynthSpec, e.g. sub_error=0.03)"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vartrix_amd import synth  # noqa: E402

WHY = ["ok", "shape", "no-diagonal", "pieces", "matches", "not-harmless", "-", "generic", "not-tight", "no-main"]
LOOSE_FAILED, CLEARED, CLEARED_DIRECT, DECIDED, BAND, CORRIDOR = 1, 2, 4, 8, 16, 32


def load(tmp):
    so = os.path.join(tmp, "librecheck_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "fastcore", "recheck_host.cpp")])
    L = C.CDLL(so)
    L.vtxt_recheck_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vtxt_recheck_batch.restype = C.c_int
    return L


def run(L, batch, recheck):
    n = 2 * batch.n_records
    score, why, route, pack = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    st = batch.as_struct()
    rc = L.vtxt_recheck_batch(C.byref(st), int(recheck), score.ctypes.data, why.ctypes.data, route.ctypes.data, pack.ctypes.data)
    assert rc == 0, rc
    return score, why, route, pack


def main():
    # the headline workload of bench.py (config 3) unless the arguments say otherwise
    kw = dict(n_loci=int(sys.argv[1]) if len(sys.argv) > 1 else 1500, n_barcodes=10000, reads_per_locus=256, read_len=150, padding=100,
              sub_error=0.005, seed=20260926)
    for a in sys.argv[2:]:
        k, v = a.split("=")
        kw[k] = float(v) if "." in v else int(v)
    batch = synth.make_batch(synth.SynthSpec(**kw))
    with tempfile.TemporaryDirectory() as tmp:
        L = load(tmp)
        _, why0, route0, _ = run(L, batch, 0)
        _, why1, route1, _ = run(L, batch, 1)
    n = why0.size
    # the first stage's leftovers for the sweep: everything without a certificate (a task with one — bit BAND — has its one-diagonal band)
    left0 = (why0 != 0) & ((route0 & BAND) == 0)
    left1 = (why1 != 0) & ((route1 & BAND) == 0)
    failed = (route1 & LOOSE_FAILED) != 0
    cleared = (route1 & CLEARED) != 0
    assert np.array_equal(cleared, (route1 & CLEARED_DIRECT) != 0)
    print("batch: %s" % ", ".join("%s=%s" % kv for kv in kw.items()))
    print("tasks %d; left without a certificate: %d (%.3f %%) without the recheck, %d (%.3f %%) with it" % (
        n, left0.sum(), 100.0 * left0.sum() / n, left1.sum(), 100.0 * left1.sum() / n))
    print("why the first stage left the task (without the recheck)")
    for k in np.unique(why0[left0]):
        print("  %-13s %8d  %5.1f %%" % (WHY[k], int((why0[left0] == k).sum()), 100.0 * (why0[left0] == k).sum() / max(left0.sum(), 1)))
    print("rechecked (failed the coarse harmless test): %d = %.3f %% of the tasks" % (failed.sum(), 100.0 * failed.sum() / n))
    dec = cleared & ((route1 & DECIDED) != 0)
    corr = cleared & ((route1 & CORRIDOR) != 0)
    band = cleared & ((route1 & BAND) != 0) & ~corr
    print("  cleared by the tight test   %8d  %5.1f %% of the rechecked, %5.1f %% of the leftovers" % (
        cleared.sum(), 100.0 * cleared.sum() / max(failed.sum(), 1), 100.0 * cleared.sum() / max(left0.sum(), 1)))
    print("    scored (cert == ub)       %8d" % dec.sum())
    print("    scored by the corridor    %8d" % corr.sum())
    print("    one-diagonal band (DP)    %8d" % band.sum())
    print("  still not harmless          %8d" % (failed & ~cleared).sum())


if __name__ == "__main__":
    main()
