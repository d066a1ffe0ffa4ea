"""Mutation checks of the certificate stages on the host mirror (tests/fastcore): each libfastcore_host_mut<n>.so is the kernel logic
with ONE bound made unsound on purpose (#if VTXF_MUTANT == n in vartrix_amd/csrc/vtx_fast_core.h / vtx_band_trim.h).  On the
adversarial batches of tests/stress_batches.py every mutant must decide at least one alignment wrongly — against the oracle's
full-matrix score for the bounds of the full score, its banded score for the bounds of the banded score — and the real header must
decide every alignment of the same batches rightly.  A suite that cannot tell a mutant from the header would not notice the bug.

Caught here (mirror modes in which the bound decides; batches; the wrong decisions are counted over all of them):
  1  join_gap3_far returns join_gap3(D): round 6's bug, blind to an excursion over a far piece     refine, trim; excursion, excursion_long
  3  join_free prices D + 11 where the closed form has D + 10                                      plain, refine, trim; edges, excursion
  5  harmless_item keeps a match one base closer than its bound allows                           corridor, trim; excursion
  6  the far-piece condition takes a piece three diagonals out as far                            refine, trim; excursion
  7  join_same's J_gap(6 i) = 8 instead of 7                                                     plain, refine, corridor; excursion
excursion_long has haplotypes of 241 - 421 bases: the mirror's four-byte path, and on the device band_refine_kernel — the one kernel
that prices joins with join_gap3_far (batches of haplotypes within 255 bases take band_corridor_kernel instead).
Open gaps (no wrong decision in 512 k alignments of each family, 2 M in all, in any mirror mode):
  2  join_gap3's floor of 11 above D = 22 raised to 12.  A catch needs a join of two main runs over D >= 23 bases whose cheapest
     crossing leaves the corridor with gaps of >= 3 bases each way at the true J_gap3(D) = 11 (not 12), while the corridor DP and every
     other chain price it higher, and the shorter run is worth 11 - 12 bases; a quarter of the excursions span D = 23 - 30, and none of
     them met all of it.  Round 6's full e8 audit, where the floor was in force on every join, found nothing at 48.6 M alignments either.
  4  band_rows one row narrower: needs a task decided by the band-restricted bound whose certificate is a run that starts in the band's
     first row.  One row WIDER is sound: more in-band runs only raise the bound.  On the device this bound (vtx_band_trim.h, stage
     BAND_CERT) runs only in band_refine_kernel with a tight list, behind the dev library's VTX_BAND_NO_CORRIDOR.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle
from vartrix_amd.abi import VtxBatch, default_config

import stress_batches as SB

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = {"plain": 1024, "refine": 1024 | (1 << 30), "corridor": 1024 | (1 << 29), "twins": 1024 | (1 << 29) | (1 << 28)}
CAUGHT = {1: (("refine", "trim"), ("excursion", "excursion_long")), 3: (("plain", "refine", "trim"), ("edges", "excursion")),
          5: (("corridor", "trim"), ("excursion",)), 6: (("refine", "trim"), ("excursion",)),
          7: (("plain", "refine", "corridor"), ("excursion",))}
BATCHES = {"excursion": (4000, 64, 100, ("excursion",), (20, 110)), "edges": (500, 64, 103, ("edges",), (20, 110)),
           "excursion_long": (2000, 64, 100, ("excursion",), (130, 200))}          # loci, reads per locus, seed, families, paddings


def _load(n):
    L = C.CDLL(os.path.join(HERE, "fastcore", "libfastcore_host%s.so" % ("_mut%d" % n if n else "")))
    L.vtxt_fastcore_batch.argtypes = [C.POINTER(VtxBatch), C.c_uint32, C.c_void_p, C.c_void_p]
    L.vtxt_fastcore_batch.restype = C.c_int
    L.vtxt_fastcore_trim_batch.argtypes = [C.POINTER(VtxBatch), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vtxt_fastcore_trim_batch.restype = C.c_int
    return L


def _oracle(batch, aligner):
    r, a = oracle.batch_scores(batch, default_config(aligner=aligner, n_barcodes=500), threads=os.cpu_count() or 8)
    out = np.empty(2 * batch.n_records, np.int32)
    out[0::2], out[1::2] = r, a
    return out


@pytest.fixture(scope="module")
def batches():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "fastcore"), "-s"])
    out = {}
    for name, (nl, reads, seed, fams, pads) in BATCHES.items():
        b = SB.adversarial_batch(nl, reads, seed, fams, pads=pads)
        out[name] = (b, _oracle(b, "banded"), _oracle(b, "full"))
    return out


def _long(batch):
    return max(int(batch.loci["ref_len"].max()), int(batch.loci["alt_len"].max())) > 255


def wrong_decisions(L, batch, banded, full, mode):
    """Alignments the mirror decides at a score that is not the one its bound promises."""
    st = batch.as_struct()
    n = 2 * batch.n_records
    sc, why = np.zeros(n, np.int32), np.zeros(n, np.uint32)
    if mode == "trim":                                   # the band-trimmed bound: banded score where it decided, full elsewhere
        if _long(batch):                                 # (the narrow path only, as band_refine_kernel's tight list)
            return np.zeros(0, np.int64), 0.0
        tr = np.zeros(n, np.uint8)
        assert L.vtxt_fastcore_trim_batch(C.byref(st), 1024, sc.ctypes.data, why.ctypes.data, tr.ctypes.data) == 0
        want = np.where(tr == 1, banded, full)
    else:
        assert L.vtxt_fastcore_batch(C.byref(st), FLAGS[mode], sc.ctypes.data, why.ctypes.data) == 0
        want = banded if mode in ("corridor", "twins") else full        # the corridor certificate bounds the banded score
    decided = sc >= 0
    return np.nonzero(decided & (sc != want))[0], float(decided.mean())


def test_real_header_is_clean_on_the_mutant_batches(batches):
    L = _load(0)
    for name, (b, banded, full) in batches.items():
        for mode in list(FLAGS) + ([] if _long(b) else ["trim"]):
            bad, frac = wrong_decisions(L, b, banded, full, mode)
            assert bad.size == 0, "%s, %s: task %d decided wrongly by the real header" % (name, mode, bad[0])
            assert frac > (0.02 if _long(b) else 0.15), (name, mode, frac)


@pytest.mark.parametrize("mutant", sorted(CAUGHT))
def test_mutant_is_caught(batches, mutant):
    modes, names = CAUGHT[mutant]
    L = _load(mutant)
    found = {}
    for name in names:
        b, banded, full = batches[name]
        wrong = set()
        for mode in modes:
            wrong.update(wrong_decisions(L, b, banded, full, mode)[0].tolist())
        found[name] = len(wrong)
    print("mutant %d: alignments decided wrongly %s (modes %s)" % (mutant, found, ", ".join(modes)))
    assert sum(found.values()) > 0, "mutant %d decides every alignment rightly: the tests cannot see it" % mutant
