"""Census of band_diag_kernel's deferral to band_tail_kernel on a synthetic batch, from the CPU build of its per-task logic
(tests/fastcore/tail_host.cpp): the share of tasks whose closure must grow the generic set (rule 1: they leave a record), and per
wavefront of 64 consecutive tasks the largest closure scan count, piece pairs of one fixpoint pass and match visits, with and without
those lanes; the share of tasks above a match count and the sort's largest ns^2 per wavefront without them (a deferral before the sort).
TEST / MEASUREMENT INFRASTRUCTURE (the product never loads it).
    g++ -O2 -std=c++17 -fPIC -shared -o /tmp/libtail_host.so tests/fastcore/tail_host.cpp && python tools/tail_census.py [n_loci] [key=value ...]"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vartrix_amd import synth  # noqa: E402

L = C.CDLL(os.environ.get("TAIL_HOST_LIB", "/tmp/libtail_host.so"))
L.vtxt_tail_census.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
kw = dict(n_loci=int(sys.argv[1]) if len(sys.argv) > 1 else 300, n_barcodes=10000, reads_per_locus=256, seed=3)
for a in sys.argv[2:]:
    k, v = a.split("=")
    kw[k] = float(v) if "." in v else int(v)
b = synth.make_batch(synth.SynthSpec(**kw))
st = b.as_struct()
out = np.zeros(64, np.uint64)
L.vtxt_tail_census(C.byref(st), 0, out.ctypes.data)
o = out.astype(float)
wf = max(o[5], 1)
print("batch: %s" % ", ".join("%s=%s" % kv for kv in kw.items()))
print("tasks %d, in the sort %d, in the closure %d; deferred (rule 1) %d = %.2f %% of the tasks, %.2f %% of those in the closure"
      % (out[0], out[30], out[1], out[2], 100 * o[2] / o[0], 100 * o[2] / max(o[1], 1)))
print("outcomes that differ from an uninterrupted back_rest: %d; deferred tasks with aux set: %d" % (out[3], out[4]))
print("wavefronts %d, with a deferred lane %.1f %%" % (out[5], 100 * o[10] / wf))
print("per wavefront, mean of the largest          all lanes   without the deferred")
print("  closure scans                             %8.2f   %8.2f" % (o[6] / wf, o[7] / wf))
print("  piece pairs of a fixpoint pass (r+ng)^2   %8.2f   %8.2f" % (o[8] / wf, o[9] / wf))
print("  closure match visits (scans x ns)         %8.2f   %8.2f" % (o[11] / wf, o[12] / wf))
print("rule 5 (defer before the sort when ns > T): share of the tasks in the sort; the sort's largest ns^2 per wavefront (all: %.0f)" % (o[23] / wf))
for i, t in enumerate((8, 12, 16, 20, 24, 28)):
    print("  T = %2d   %6.2f %%   %8.0f" % (t, 100 * o[16 + i] / max(o[30], 1), o[24 + i] / wf))
