"""The recheck of the tasks that fail band_diag_kernel's harmless test, on the CPU build of the per-task logic (tests/fastcore/
recheck_host.cpp over vtx_fast_core.h: tail_pack, tail_unpack, LaneSR, recheck_rest — the source the kernels compile).  Such a task
leaves the tail's record; the tight form of the test runs on the record's list, and a task it clears goes on as one the first test
cleared.  Against the oracle, per batch:
  * every task the stage decides by cert == ub scores the oracle's banded score AND its full score (cert <= banded <= full <= ub),
    every task the corridor certificate decides the banded score;
  * a cleared task's one-diagonal band (vtxf::band_pack) is the band the oracle builds, column by column, and its certificate is a
    lower bound of the banded score;
  * the verdict through the record equals back_harmless<TIGHT> run directly on the lane's own list;
  * the recheck changes nothing for a task that passed the first test.
Each batch holds at least 20 tasks that fail the coarse test and at least 5 the tight test clears (asserted)."""
import numpy as np
import pytest

from oracle import oracle
from vartrix_amd import synth
from vartrix_amd.abi import default_config

import recheck_util as RU
import stress_batches as SB


def batches():
    yield "clean", synth.make_batch(synth.SynthSpec(n_loci=200, n_barcodes=500, reads_per_locus=128, seed=31)), 500
    yield "3 % errors", synth.make_batch(synth.SynthSpec(n_loci=150, n_barcodes=500, reads_per_locus=64, sub_error=0.03, seed=32)), 500
    yield "8 % errors", synth.make_batch(synth.SynthSpec(n_loci=100, n_barcodes=500, reads_per_locus=64, sub_error=0.08, seed=33)), 500
    for label, b, nb in list(SB.synthetic_batches(per_model=1))[1:3]:          # 2 % errors with indels in 30 % of the loci; 5 % with 50 %
        yield "indels: " + label, b, nb
    yield list(SB.adversarial_batches(n_loci=120, reads=32, families=("repeats",)))[0]       # tandem repeats planted in the window
    yield list(SB.near_repeat_batches(trials=4, loci=320))[3]                                   # near repeats, 8 planted per locus
    yield next(iter(SB.real_sequence_batches(trials=1)))                                        # loci drawn from tests/golden/test_dna.fa


CASES = list(range(8))
_batches = {}


def case(i):
    if not _batches:
        for k, b in enumerate(batches()):
            _batches[k] = b
        assert len(_batches) == len(CASES)
    return _batches[i]


@pytest.fixture(scope="module")
def mirror_lib(tmp_path_factory):
    return RU.load_mirror(tmp_path_factory.mktemp("recheck"))


def oracle_tasks(batch, nb, aligner):
    r, a = oracle.batch_scores(batch, default_config(aligner=aligner, n_barcodes=nb), threads=8)
    t = np.empty(2 * batch.n_records, np.int32)
    t[0::2], t[1::2] = r, a
    return t


def band_from_pack(pk, m, n):
    """The band sw_banded_kernel<.., 2> expands from vtxf::band_pack: one diagonal stretch widened by w = 20 (vtx_fast_core.h)."""
    dd, ca, cb = (pk >> 16) - 256, (pk >> 8) & 0xff, pk & 0xff
    lo, hi = np.full(n + 1, m + 1, np.int64), np.zeros(n + 1, np.int64)
    for j in range(n + 1):
        if ca - 20 <= j <= cb + 20:
            lo[j] = max(0, max(j - 20, ca) - dd - 20)
            hi[j] = min(m + 1, min(j + 20, cb) - dd + 21)
    return lo, hi


@pytest.mark.parametrize("i", CASES)
def test_recheck_against_the_oracle(mirror_lib, i):
    label, batch, nb = case(i)
    rc, score, why, route, pack = RU.mirror(mirror_lib, batch, recheck=True)
    assert rc == 0, (label, rc)
    failed, cleared = (route & RU.LOOSE_FAILED) != 0, (route & RU.CLEARED) != 0
    print("%s: %d tasks, %d fail the coarse test, %d cleared by the tight one" % (label, route.size, failed.sum(), cleared.sum()))
    assert failed.sum() >= 20 and cleared.sum() >= 5, (label, int(failed.sum()), int(cleared.sum()))
    assert np.array_equal(cleared, (route & RU.CLEARED_DIRECT) != 0), "%s: the verdict through the record differs from back_harmless<TIGHT> on the list" % label
    assert not np.any(cleared & ~failed)

    banded, full = oracle_tasks(batch, nb, "banded"), oracle_tasks(batch, nb, "full")
    decided = (route & RU.DECIDED) != 0
    bad = np.nonzero(decided & ((score != banded) | (score != full)))[0]
    assert bad.size == 0, "%s: task %d decided at %d, oracle banded %d, full %d" % (label, bad[0], score[bad[0]], banded[bad[0]], full[bad[0]])
    assert (decided & cleared).sum() > 0, label                                  # (the recheck itself decides some)
    corr = (route & RU.CORRIDOR) != 0
    bad = np.nonzero(corr & (score != banded))[0]
    assert bad.size == 0, "%s: task %d scored %d by the corridor, oracle banded %d" % (label, bad[0], score[bad[0]], banded[bad[0]])
    band = (route & RU.BAND) != 0
    assert np.all(score[band & ~corr] <= banded[band & ~corr]), label               # the certificate: a lower bound of the banded score
    assert np.all((why == 0) == (decided | corr)), label

    # a cleared task that keeps its certificate: the one-diagonal band is the oracle's
    rec_locus = np.repeat(np.arange(batch.n_loci), batch.loci["rec_count"])
    hb, rb = batch.hap_arena.tobytes(), batch.read_arena.tobytes()
    todo = np.nonzero(cleared & band)[0]
    if todo.size > 150:
        todo = np.random.default_rng(16).choice(todo, 150, replace=False)
    for t in todo:
        rec, loc = batch.records[t >> 1], batch.loci[rec_locus[t >> 1]]
        x = rb[int(rec["read_off"]):int(rec["read_off"]) + int(rec["read_len"])]
        off, ln = (int(loc["alt_off"]), int(loc["alt_len"])) if t & 1 else (int(loc["ref_off"]), int(loc["ref_len"]))
        y = hb[off:off + ln]
        lo, hi = band_from_pack(int(pack[t]), len(x), len(y))
        olo, ohi, _ = oracle.band_create(x, y)
        empty = ohi <= olo
        assert np.array_equal(lo[~empty], olo[~empty]) and np.array_equal(hi[~empty], ohi[~empty]) and not hi[empty].any(), (label, int(t))

    # without the recheck: the same for every task that passed the first test, W_NOT_HARMLESS for the others
    rc0, score0, why0, route0, pack0 = RU.mirror(mirror_lib, batch, recheck=False)
    assert rc0 == 0 and np.array_equal(failed, (route0 & RU.LOOSE_FAILED) != 0)
    keep = ~failed
    assert np.array_equal(score[keep], score0[keep]) and np.array_equal(why[keep], why0[keep]) and np.array_equal(route[keep], route0[keep]) \
        and np.array_equal(pack[keep], pack0[keep]), label
    assert np.all(why0[failed] == 5) and np.all(score0[failed] == -1)
    assert np.all(why[failed & ~cleared] == 5)
