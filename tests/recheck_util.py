"""What tests/test_recheck_core.py and tests/test_gpu_recheck.py share: the host mirror of the first stage with the recheck
(tests/fastcore/recheck_host.cpp, compiled on demand) and the GPU test's batches, built from fixed seeds so that the test process (the
mirror) and its child processes (the device) hold the same bytes."""
import ctypes as C
import os
import subprocess

import numpy as np

from vartrix_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
DNA = os.path.join(HERE, "golden", "test_dna.fa")
LOOSE_FAILED, CLEARED, CLEARED_DIRECT, DECIDED, BAND, CORRIDOR = 1, 2, 4, 8, 16, 32
NB = 500


def load_mirror(tmp_dir):
    so = os.path.join(str(tmp_dir), "librecheck_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "fastcore", "recheck_host.cpp")])
    L = C.CDLL(so)
    L.vtxt_recheck_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vtxt_recheck_batch.restype = C.c_int
    return L


def mirror(L, batch, recheck=True):
    """(rc, score, why, route, pack) per task t = 2 * record + haplotype; rc -1: a haplotype above 255 bases (no recheck on the device either)."""
    n = 2 * batch.n_records
    score, why, route, pack = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    st = batch.as_struct()
    rc = L.vtxt_recheck_batch(C.byref(st), int(recheck), score.ctypes.data, why.ctypes.data, route.ctypes.data, pack.ctypes.data)
    return rc, score, why, route, pack


# 64 loci x 64 reads each (8 192 tasks).  Not-harmless tasks are common on real sequence (chance matches by the dozen) and at 3 % errors.
GPU_LABELS = ("real sequence", "3 % errors", "real sequence, 3 % errors, 230-base reads", "haplotypes of 261 bases")


def gpu_batches():
    return [
        synth.make_batch(synth.SynthSpec(n_loci=64, n_barcodes=NB, reads_per_locus=64, genome_fasta=DNA, seed=1601)),                 # reads <= 192 bases: three mask words
        synth.make_batch(synth.SynthSpec(n_loci=64, n_barcodes=NB, reads_per_locus=64, sub_error=0.03, seed=1612)),
        synth.make_batch(synth.SynthSpec(n_loci=64, n_barcodes=NB, reads_per_locus=64, read_len=230, padding=125, sub_error=0.03,
                                         genome_fasta=DNA, seed=1603)),                                                                # reads of 193 - 256 bases: four mask words
        synth.make_batch(synth.SynthSpec(n_loci=64, n_barcodes=NB, reads_per_locus=64, padding=130, sub_error=0.03, genome_fasta=DNA, seed=1604)),   # no two-byte entries: no recheck
    ]
