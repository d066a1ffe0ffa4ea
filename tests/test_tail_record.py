"""The deferral of band_diag_kernel's rare last-phase path to band_tail_kernel, on the CPU build of the per-task logic
(tests/fastcore/tail_host.cpp over vtx_fast_core.h): every task that reaches the closure is finished twice — uninterrupted, and
the way the two kernels finish it (closure_first; a deferred task packed into a record, unpacked into a poisoned lane, back_rest
again).  Score, why, aux, band word, certificate and far rows (what the routing reads) must agree for every task, on clean, 3 %,
8 %, real-sequence and adversarial batches, with two-byte and four-byte match entries."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from vartrix_amd import synth

import stress_batches as SB

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def tail_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tail") / "libtail_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "fastcore", "tail_host.cpp")])
    L = C.CDLL(so)
    L.vtxt_tail_census.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.vtxt_tail_census.restype = C.c_int
    return L


def census(L, batch, wide):
    out = np.zeros(64, np.uint64)
    st = batch.as_struct()
    assert L.vtxt_tail_census(C.byref(st), int(wide), out.ctypes.data) == 0
    return out


def batches():
    yield "clean", synth.make_batch(synth.SynthSpec(n_loci=60, n_barcodes=1000, reads_per_locus=48, seed=21))
    yield "3 %", synth.make_batch(synth.SynthSpec(n_loci=60, n_barcodes=1000, reads_per_locus=48, sub_error=0.03, seed=22))
    yield "8 %", synth.make_batch(synth.SynthSpec(n_loci=60, n_barcodes=1000, reads_per_locus=48, sub_error=0.08, seed=23))
    yield "real sequence", next(iter(SB.real_sequence_batches(trials=1, n_loci=120, reads=24)))[1]
    yield "adversarial", SB.adversarial_batch(160, 24, seed=24)


@pytest.mark.parametrize("wide", [False, True], ids=["two-byte", "four-byte"])
def test_deferred_tasks_end_as_uninterrupted(tail_lib, wide):
    deferred = closure = 0
    for label, batch in batches():
        out = census(tail_lib, batch, wide)
        assert out[3] == 0, "%s: %d tasks end differently when deferred" % (label, out[3])
        assert out[4] == 0, "%s: a deferred task left aux set (band_tail_kernel routes them without it)" % label
        deferred += int(out[2]); closure += int(out[1])
    assert closure > 2000 and deferred > 50, (closure, deferred)
