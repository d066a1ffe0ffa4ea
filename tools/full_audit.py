#!/usr/bin/env python3
"""Full audit of a workload of tests/audit_util.py's AUDIT_WORKLOADS (the table the -m gpu audits of tests/test_gpu_properties.py
run, so that tool and tests cannot drift apart): the checks of audit_util.full_size_audit, and then EVERY alignment of the
production run against the oracle.

    python tools/full_audit.py [config3|e8|e3|real|config5|reads250|padding150|adversarial] ...   (GPU box; ~2.5 min of 16 CPU threads
                                                                                                  per 48.6 M alignments)

The oracle (oracle.batch_scores: the restated reference CPU path, bio 0.30.0's banded::Aligner::local per read and haplotype,
src/main.rs:898-901) scores the whole batch on the host's cores; every mismatch — none is expected — is broken down by the stage
that decided it."""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle                                                   # noqa: E402
from audit_util import AUDIT_WORKLOADS, audit_config, full_size_audit, stage_report   # noqa: E402


def main():
    for name in (sys.argv[1:] or ["config3", "real"]):
        assert name in AUDIT_WORKLOADS, "unknown workload %s (%s)" % (name, ", ".join(AUDIT_WORKLOADS))
        with tempfile.TemporaryDirectory() as td:
            res = full_size_audit(name, td)
        batch, stage, t = res["batch"], res["stage"], res["timing"]
        t0 = time.time()
        threads = len(os.sched_getaffinity(0))
        oref, oalt = oracle.batch_scores(batch, audit_config(name, "banded", res["n_barcodes"]), threads=threads)
        dt = time.time() - t0
        b = res["banded"]
        o = np.empty_like(b)
        o[0::2], o[1::2] = oref, oalt
        bad = b != o
        print("  oracle: all %d alignments in %.0f s on %d threads (%.3g alignments/s)" % (len(o), dt, threads, len(o) / dt))
        print("  MISMATCHES device vs oracle: %d%s" % (int(bad.sum()), "" if not bad.any() else
              "  by stage %s, first at task %d: device %d oracle %d" % (stage_report(stage[bad]), int(np.nonzero(bad)[0][0]),
                                                                        int(b[bad][0]), int(o[bad][0]))))
        print("  left by the first certificate stage %d, second stage looked at %d (scored %d, %d through band_stream_kernel), one-diagonal bands %d, swept %d, general kernel %d" % (
            t.diag_left, t.diag2_tasks, t.diag2_scored, t.diag2_streamed, t.checked_tasks, t.swept_tasks, t.overflow_tasks), flush=True)
        assert not bad.any()


if __name__ == "__main__":
    main()
