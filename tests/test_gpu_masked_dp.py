"""sw_banded_kernel (vartrix_amd/csrc/vtx_kernels.hip) on its own, all 27 instances — 9 (rows per lane, lanes per record) shapes x
3 modes — against the oracle's range-restricted DP, oracle.sw_ranges: equal integers, no tolerance.  The kernel is launched through
libvtx_dev.so's vtxk_dev_sw_pairs (host arrays in and out, the production launcher in between), so the bands are whatever a test
writes, not only the staircases the band kernels build.

  mode 0  per-column row ranges: the families of tests/masked_dp_util.py (tests/test_masked_dp_model.py shows, from the oracle
          alone, that those bands decide the scores), the degenerate bands, the launch edges (list lengths, a device-side length),
          unlike partners in one register, unlike records in one wave, haplotypes long enough for the launcher's smaller workgroups.
  mode 2  the band expanded in LDS from one band_pack word, against sw_ranges over the squares model, in production's domain.
  mode 1  the full-matrix check: which tasks reach the recheck list, with their packs; stage bytes; no score written.

Every run also checks what must NOT change: scores and stage bytes of tasks that are not listed, or listed at or beyond the
device-side length, keep their poison."""
import functools

import numpy as np
import pytest

import masked_dp_util as U
from oracle import oracle

pytestmark = pytest.mark.gpu
ALL_SHAPES = pytest.mark.parametrize("shape", U.SHAPES, ids=[U.shape_id(s) for s in U.SHAPES])
EDGE_SHAPES = pytest.mark.parametrize("shape", [(10, 16), (8, 64)], ids=["R10xGL16", "R8xGL64"])


@functools.lru_cache(maxsize=None)
def shape_problem(shape):
    return U.Problem([(r, h) for r, h, _ in U.shape_cases(shape)])


def check(res, prob, order, want, stage=None, active=None, what=""):
    """The listed tasks order[:active] hold `want` (one score per list entry) and stage byte `stage` (None: untouched); every
    other task — not listed, listed behind `active`, the decoy haplotypes — still holds the poison in both arrays."""
    assert res.rc == 0, "%s: hipError %d" % (what, res.rc)
    order = np.asarray(order, np.int64)
    active = len(order) if active is None else min(active, len(order))
    live = order[:active]
    got = res.score[live]
    want = np.asarray(want, np.int32)[:active]
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%s: %d of %d scores differ from the oracle; first: list entry %d (case %d, read %d, haplotype %d bases): got %d, want %d" % (
        what, len(bad), active, bad[0], live[bad[0]], len(prob.reads[live[bad[0]]]), len(prob.haps[live[bad[0]]]), got[bad[0]], want[bad[0]])
    rest = np.ones(prob.n, bool)
    rest[live] = False
    assert (res.score[rest] == U.SCORE_POISON).all(), "%s: a task outside the list got a score" % what
    assert (res.decoy_score == U.SCORE_POISON).all(), "%s: the other haplotype of a record got a score" % what
    assert (res.task_stage[rest] == U.STAGE_POISON).all() and (res.decoy_stage == U.STAGE_POISON).all(), "%s: stage byte outside the list" % what
    assert (res.task_stage[live] == (U.STAGE_POISON if stage is None else stage)).all(), "%s: stage bytes of the listed tasks" % what


# ---------------------------------------------------------------- mode 0
@ALL_SHAPES
@pytest.mark.parametrize("family", U.FAMILIES)
def test_mode0_families(shape, family):
    """Every case of the shape under one family of bands, in a shuffled list (odd for three of the families)."""
    prob = shape_problem(shape)
    bands, want = U.family_bands(shape, family), U.family_scores(shape, family)
    rng = np.random.default_rng(U.FAMILIES.index(family))
    order = rng.permutation(prob.n)[:prob.n - (U.FAMILIES.index(family) % 2 == 0)]
    res = U.run_pairs(prob, order, 0, shape, 255, bands=[bands[i] for i in order])
    check(res, prob, order, want[order], what="%s %s" % (U.shape_id(shape), family))
    if family == "full":
        assert np.array_equal(res.score[order], U.full_scores(shape)[order])


@ALL_SHAPES
def test_mode0_degenerate_bands(shape):
    """All columns empty, one cell, row 0 only, column 0 only, row 0 in band in every other column, the band from row 1, the last
    row only: on reads of the shape's capacity, one less, 1, 7 and a short one."""
    cases = U.shape_cases(shape)
    cap = U.capacity(shape)
    picks = []
    for want_m in (cap, cap - 1, 1, 7):
        picks.append(next(c for c in cases if len(c[0]) == want_m))
    picks.append(next(c for c in cases if 20 <= len(c[0]) <= 40 and len(c[0]) < cap - 1))
    picks.append(next(c for c in cases if len(c[1]) == 255))
    dup, bands, names = [], [], []
    for r, h, _ in picks:
        for name, band in U.degenerate_bands(r, h).items():
            dup.append((r, h)), bands.append(band), names.append(name)
    prob = U.Problem(dup)
    want = np.array([U.ranges_score(r, h, lo, hi) for (r, h), (lo, hi) in zip(dup, bands)], np.int32)
    for name, w in zip(names, want):
        if name in ("all_empty", "row0_only", "col0_only", "one_cell", "one_matching_cell"):
            assert w == 0
        if name == "two_cells_on_a_diagonal":
            assert w == 1
    order = np.arange(prob.n)
    res = U.run_pairs(prob, order, 0, shape, 255, bands=bands)
    check(res, prob, order, want, what="%s degenerate (%s)" % (U.shape_id(shape), ", ".join(sorted(set(names)))))


@EDGE_SHAPES
def test_launch_edges(shape):
    """List lengths around a pair and around a workgroup; a device-side length below, at and above the list length.  A workgroup
    of 256 threads holds 256 / GL record slots of two tasks each."""
    prob = shape_problem(shape)
    bands, want = U.family_bands(shape, "shifted"), U.family_scores(shape, "shifted")
    per_wg = 2 * (256 // shape[1])
    rng = np.random.default_rng(5)
    big = 3 * per_wg + 1
    assert big <= prob.n
    for L in (1, 2, 5, per_wg, per_wg + 1, big):
        order = rng.permutation(prob.n)[:L]
        res = U.run_pairs(prob, order, 0, shape, 255, bands=[bands[i] for i in order])
        check(res, prob, order, want[order], what="%s list of %d" % (U.shape_id(shape), L))
    order = rng.permutation(prob.n)[:big]
    for n_dev in (0, 1, 7, per_wg - 1, per_wg + 1, big - 1, big, big + 5):
        res = U.run_pairs(prob, order, 0, shape, 255, bands=[bands[i] for i in order], n_dev=n_dev)
        check(res, prob, order, want[order], active=n_dev, what="%s list of %d, device-side length %d" % (U.shape_id(shape), big, n_dev))


def mixed_band(rng, r, h, shape):
    return U.family_band(("shifted", "random", "oracle", "stripe")[int(rng.integers(0, 4))], rng, r, h, shape)


@EDGE_SHAPES
def test_partners_do_not_see_each_other(shape):
    """The two tasks of a record slot share every VGPR, half each.  The same tasks in three list orders, so that each meets
    another partner: 1-base haplotypes beside 255-base ones, 1-base reads beside reads of the shape's capacity."""
    rng = np.random.default_rng(17)
    cap = U.capacity(shape)
    kinds = ((cap, 1), (1, 255), (1, 1), (cap, 255), (cap // 2, 100), (cap - 1, 254))
    cases = [U.make_case(rng, m, n) for m, n in kinds for _ in range(4)]
    prob = U.Problem([(r, h) for r, h, _ in cases])
    bands = [mixed_band(rng, r, h, shape) for r, h, _ in cases]
    want = np.array([U.ranges_score(r, h, lo, hi) for (r, h, _), (lo, hi) in zip(cases, bands)], np.int32)
    by_kind = np.arange(prob.n)                                        # partners of one kind
    interleaved = by_kind.reshape(len(kinds), 4).T.reshape(-1)         # kind 0 beside kind 1, 2 beside 3, 4 beside 5
    crossed = np.concatenate([interleaved[::2], interleaved[1::2][::-1]])

    def partners(order):
        p = {}
        for s in range(0, len(order) - 1, 2):
            p[order[s]], p[order[s + 1]] = order[s + 1], order[s]
        return p
    pa, pb, pc = partners(by_kind), partners(interleaved), partners(crossed)
    assert all(pa[i] != pb[i] and pb[i] != pc[i] and pa[i] != pc[i] for i in range(prob.n))
    assert any({len(prob.haps[i]), len(prob.haps[pb[i]])} == {1, 255} for i in range(prob.n))
    assert any({len(prob.reads[i]), len(prob.reads[pb[i]])} == {1, cap} for i in range(prob.n))
    runs = []
    for name, order in (("by kind", by_kind), ("interleaved", interleaved), ("crossed", crossed)):
        res = U.run_pairs(prob, order, 0, shape, 255, bands=[bands[i] for i in order])
        check(res, prob, order, want[order], what="%s partners %s" % (U.shape_id(shape), name))
        runs.append(res.score.copy())
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


@pytest.mark.parametrize("shape", [(2, 16), (10, 16), (16, 16)], ids=["R2xGL16", "R10xGL16", "R16xGL16"])
def test_wave_of_unlike_records(shape):
    """GL = 16: a wave carries four record slots and runs as many steps as its longest haplotype needs.  Haplotypes of 1, 60, 200
    and 255 bases in one wave — first with both tasks of a slot alike, then with the two halves unlike as well."""
    rng = np.random.default_rng(23)
    cap = U.capacity(shape)
    lens = (1, 60, 200, 255)
    slots = [(lens[q % 4], lens[q % 4]) for q in range(16)] + [(lens[q % 4], lens[3 - q % 4]) for q in range(16)]
    reads = (cap, cap - 1, max(cap // 3, 1), 7)
    cases = [U.make_case(rng, reads[int(rng.integers(0, 4))], n) for pair in slots for n in pair]
    prob = U.Problem([(r, h) for r, h, _ in cases])
    bands = [mixed_band(rng, r, h, shape) for r, h, _ in cases]
    want = np.array([U.ranges_score(r, h, lo, hi) for (r, h, _), (lo, hi) in zip(cases, bands)], np.int32)
    order = np.arange(prob.n)
    res = U.run_pairs(prob, order, 0, shape, 255, bands=bands)
    check(res, prob, order, want, what="%s waves of haplotypes 1 / 60 / 200 / 255" % U.shape_id(shape))


@EDGE_SHAPES
@pytest.mark.parametrize("max_hap", [700, 800, 1500, 1600, 2400])
def test_long_haplotypes(shape, max_hap):
    """Three LDS arrays per record slot: with 16 lanes per record the launcher halves the workgroup above ~760 bases and again
    above ~1 560 (launch_sw_pairs); with 64 lanes it never has to.  Families full and shifted, a handful of tasks."""
    rng = np.random.default_rng(max_hap)
    cap = U.capacity(shape)
    cases = [U.make_case(rng, m, n) for m, n in ((cap, max_hap), (cap - 1, max_hap - 1), (37, max_hap // 2), (cap, 300), (7, max_hap))]
    prob = U.Problem([(r, h) for r, h, _ in cases])
    order = np.arange(prob.n)
    for family in ("full", "shifted"):
        bands = [U.family_band(family, rng, r, h, shape) for r, h, _ in cases]
        want = np.array([U.ranges_score(r, h, lo, hi) for (r, h, _), (lo, hi) in zip(cases, bands)], np.int32)
        if family == "full":
            assert np.array_equal(want, [oracle.sw_full(r, h) for r, h, _ in cases])
        else:
            assert (want != [oracle.sw_full(r, h) for r, h, _ in cases]).any()
        res = U.run_pairs(prob, order, 0, shape, max_hap, bands=bands)
        check(res, prob, order, want, what="%s haplotypes up to %d, %s" % (U.shape_id(shape), max_hap, family))


# ---------------------------------------------------------------- mode 2
@functools.lru_cache(maxsize=None)
def diag_cases(shape):
    """Mode 2's domain: reads of 6 .. 256 bases (and within the shape), haplotypes of 6 .. 255; (read, hap, d, ca, cb) with
    d in [-(m - 6), n - 6] and 0 <= ca <= cb <= n."""
    rng = np.random.default_rng(400 + 100 * shape[0] + shape[1])
    top = min(U.capacity(shape), 256)
    prev = U.prev_capacity(shape) + 1
    out = []
    for i in range(64):
        m = (top, top - 1, 7, int(rng.integers(20, min(40, top - 2) + 1)), prev if 6 <= prev <= 256 else top, int(rng.integers(6, top + 1)))[i % 6]
        n = int(rng.integers(6, 256)) if i % 9 else (255, 6)[(i // 9) % 2]
        r, h, d0 = U.make_case(rng, m, n)
        dmin, dmax = -(m - 6), n - 6
        d = min(max(d0, dmin), dmax)
        v = i % 8
        ca = int(rng.integers(0, n + 1))
        cb = int(rng.integers(ca, n + 1))
        if v == 0:                                       # the stretch production would find: the cells of the read's diagonal inside the matrix
            ca, cb = max(d + 1, 0), min(d + m, n)
            ca, cb = min(ca + int(rng.integers(0, 8)), cb), max(cb - int(rng.integers(0, 8)), ca)
            cb = max(cb, ca)
        elif v == 1:
            cb = ca
        elif v == 2:
            ca = 0
        elif v == 3:
            cb = n
        elif v == 4:
            d = dmin
        elif v == 5:
            d = dmax
        elif v == 6:                                     # the one square above the matrix (from 27 bases: rows 0 - d + w < 0): an empty band
            d, ca, cb = dmax, 0, 0
        assert dmin <= d <= dmax and 0 <= ca <= cb <= n
        out.append((r, h, d, ca, cb))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def diag_reference(shape):
    cases = diag_cases(shape)
    prob = U.Problem([(c[0], c[1]) for c in cases])
    packs = np.array([U.band_pack(d, ca, cb) for _, _, d, ca, cb in cases], np.uint32)
    want = np.array([U.ranges_score(r, h, *U.squares_band(d, ca, cb, len(r), len(h))) for r, h, d, ca, cb in cases], np.int32)
    return prob, packs, want


@ALL_SHAPES
def test_mode2_band_from_one_word(shape):
    prob, packs, want = diag_reference(shape)
    assert (want > 0).mean() >= 0.5
    rng = np.random.default_rng(3)
    for order, n_dev in ((rng.permutation(prob.n)[:prob.n - 1], None), (rng.permutation(prob.n), prob.n - 5)):
        res = U.run_pairs(prob, order, 2, shape, 255, packs=packs[order], n_dev=n_dev)
        check(res, prob, order, want[order], stage=U.STAGE_DIAG_DP, active=n_dev,
              what="%s band_pack words, device-side length %s" % (U.shape_id(shape), n_dev))


@pytest.mark.parametrize("shape", [(2, 16), (10, 16), (8, 64)], ids=["R2xGL16", "R10xGL16", "R8xGL64"])
def test_mode2_band_above_the_matrix_leaves_its_partner_alone(shape):
    """d = n - 6 with ca = cb = 0: the one square lies above row 0, the task's band is empty and it scores 0 — and the task in
    the other half of its registers, whose band is an ordinary diagonal stretch, scores what it scores alone."""
    rng = np.random.default_rng(6)
    m = min(U.capacity(shape), 150)
    cases = [U.make_case(rng, m, 200) for _ in range(4)]
    prob = U.Problem([(r, h) for r, h, _ in cases])
    words, want = [], []
    for i, (r, h, d0) in enumerate(cases):
        d, ca, cb = (len(h) - 6, 0, 0) if i in (0, 3) else (d0, max(d0 + 1, 0), min(d0 + m, len(h)))
        words.append(U.band_pack(d, ca, cb))
        want.append(U.ranges_score(r, h, *U.squares_band(d, ca, cb, len(r), len(h))))
    assert want[0] == 0 and want[3] == 0 and want[1] > 10 and want[2] > 10
    order = np.arange(4)                                  # the empty band in the low half of one slot and in the high half of the next
    res = U.run_pairs(prob, order, 2, shape, 255, packs=np.array(words, np.uint32))
    check(res, prob, order, want, stage=U.STAGE_DIAG_DP, what="%s empty band beside a diagonal stretch" % U.shape_id(shape))


# ---------------------------------------------------------------- mode 1
@ALL_SHAPES
@pytest.mark.parametrize("with_n_dev", [False, True], ids=["host_length", "device_length"])
def test_mode1_recheck_list(shape, with_n_dev):
    """A random half of the tasks carries the full-matrix score as its provisional score: those get the stage byte
    VTX_STAGE_FULL_CHECK and nothing else.  The others (full - 1, full - 3, or 0) are exactly the recheck list, each with its
    pack; the order is free.  No score changes."""
    prob = shape_problem(shape)
    full = U.full_scores(shape)
    rng = np.random.default_rng(11 + with_n_dev)
    order = rng.permutation(prob.n)[:prob.n - 1]
    n_dev = len(order) - 3 if with_n_dev else None
    keep = rng.random(prob.n) < 0.5
    delta = np.array([1, 3, 0])[rng.integers(0, 3, prob.n)]
    prov = np.where(keep, full, np.where((delta == 0) & (full > 0), 0, full - np.maximum(delta, 1))).astype(np.int32)
    assert ((prov != full) == ~keep).all()
    ref, alt = np.full(prob.n, U.SCORE_POISON, np.int32), np.full(prob.n, U.SCORE_POISON, np.int32)
    odd = (np.arange(prob.n) & 1).astype(bool)
    ref[~odd], alt[odd] = prov[~odd], prov[odd]
    packs = (0xabc00000 + np.arange(prob.n)).astype(np.uint32)
    res = U.run_pairs(prob, order, 1, shape, 255, packs=packs[order], prov=(ref, alt), n_dev=n_dev)
    what = "%s check, %s" % (U.shape_id(shape), "device-side length %d" % n_dev if with_n_dev else "host-side length")
    assert res.rc == 0, "%s: hipError %d" % (what, res.rc)
    assert np.array_equal(res.ref, ref) and np.array_equal(res.alt, alt), "%s: a score changed" % what
    live = order[:len(order) if n_dev is None else n_dev]
    want_pairs = {(int(prob.tasks[i]), int(packs[i])) for i in live if not keep[i]}
    assert res.recheck_count == len(want_pairs), "%s: %d tasks on the recheck list, want %d" % (what, res.recheck_count, len(want_pairs))
    got_pairs = set(zip(res.recheck_list[:res.recheck_count].tolist(), res.recheck_pack[:res.recheck_count].tolist()))
    assert got_pairs == want_pairs, "%s: missing %s, stray %s" % (what, sorted(want_pairs - got_pairs)[:4], sorted(got_pairs - want_pairs)[:4])
    stage_want = np.full(prob.n, U.STAGE_POISON, np.uint8)
    stage_want[[i for i in live if keep[i]]] = U.STAGE_FULL_CHECK
    assert np.array_equal(res.task_stage, stage_want) and (res.decoy_stage == U.STAGE_POISON).all(), "%s: stage bytes" % what


# ---------------------------------------------------------------- all instances, and the hook's own checks
def test_every_instance_is_launched():
    """3 modes x 9 shapes on three tasks each (an odd list), named one by one."""
    launched = []
    for shape in U.SHAPES:
        prob, packs, want2 = diag_reference(shape)
        cases = diag_cases(shape)
        order = np.array([0, 1, 5])
        bands = [U.oracle_band(cases[i][0], cases[i][1]) for i in order]
        want0 = [U.ranges_score(cases[i][0], cases[i][1], *b) for i, b in zip(order, bands)]
        check(U.run_pairs(prob, order, 0, shape, 255, bands=bands), prob, order, want0, what="%s mode 0" % U.shape_id(shape))
        launched.append("sw_banded_kernel<%d, %d, 0>" % shape)
        full = np.array([oracle.sw_full(c[0], c[1]) for c in cases], np.int32)
        ref, alt = np.full(prob.n, U.SCORE_POISON, np.int32), np.full(prob.n, U.SCORE_POISON, np.int32)
        for k, i in enumerate(order):
            (alt if i & 1 else ref)[i] = full[i] - (k == 1)
        res = U.run_pairs(prob, order, 1, shape, 255, packs=packs[order], prov=(ref, alt))
        assert res.rc == 0 and res.recheck_count == 1 and res.recheck_list[0] == prob.tasks[order[1]] and res.recheck_pack[0] == packs[order[1]]
        assert np.array_equal(res.ref, ref) and np.array_equal(res.alt, alt)
        launched.append("sw_banded_kernel<%d, %d, 1>" % shape)
        check(U.run_pairs(prob, order, 2, shape, 255, packs=packs[order]), prob, order, want2[order], stage=U.STAGE_DIAG_DP,
              what="%s mode 2" % U.shape_id(shape))
        launched.append("sw_banded_kernel<%d, %d, 2>" % shape)
    print("\n".join(launched))
    assert len(set(launched)) == 27


def test_hook_refuses_what_would_launch_out_of_bounds():
    """hipErrorInvalidValue before any launch: a shape the launcher does not have, a read longer than R * GL, a haplotype longer
    than max_hap_len or than its band slot, a task that does not exist."""
    shape = (10, 16)
    prob = shape_problem(shape)
    bands = U.family_bands(shape, "full")
    order = np.arange(8)
    b = [bands[i] for i in order]
    longest = max(len(prob.haps[i]) for i in order)
    assert U.run_pairs(prob, order, 0, shape, 255, bands=b).rc == 0
    assert U.run_pairs(prob, order, 0, (3, 16), 255, bands=b).rc == U.HIP_INVALID_VALUE
    assert U.run_pairs(prob, order, 0, (10, 64), 255, bands=b).rc == U.HIP_INVALID_VALUE
    assert U.run_pairs(prob, order[:1], 0, shape, 255, bands=b[:1], tasks=np.array([2 * prob.n], np.uint32)).rc == U.HIP_INVALID_VALUE
    assert U.run_pairs(prob, order, 0, shape, longest - 1, bands=b).rc == U.HIP_INVALID_VALUE
    assert U.run_pairs(prob, order, 3, shape, 255, bands=b).rc == U.HIP_INVALID_VALUE
    long_read = next(i for i in range(prob.n) if len(prob.reads[i]) == 160)
    assert U.run_pairs(prob, [long_read], 0, (8, 16), 255, bands=[bands[long_read]]).rc == U.HIP_INVALID_VALUE
    # a band slot shorter than the haplotype's n + 1 entries: a 255-base haplotype's task with the two-entry slot of a 1-base one
    tiny = next(i for i in range(prob.n) if len(prob.haps[i]) == 1)
    big = next(i for i in range(prob.n) if len(prob.haps[i]) == 255)
    res = U.run_pairs(prob, [tiny], 0, shape, 255, bands=[bands[tiny]], tasks=np.array([prob.tasks[big]], np.uint32))
    assert res.rc == U.HIP_INVALID_VALUE
