"""Keeps tests/test_gpu_masked_dp.py honest, without a GPU: the reference it compares the masked DP with, the model of the band
of a band_pack word, and the conditions under which its comparisons mean something — all computed from the oracle alone."""
import numpy as np
import pytest

import masked_dp_util as U
from oracle import oracle

W = U.W


def test_full_band_is_the_full_matrix():
    """With lo = 0, hi = m + 1 in every column the range-restricted DP is the full-matrix one."""
    for shape in U.SHAPES:
        bands = U.family_bands(shape, "full")
        for (read, hap, _), (lo, hi) in zip(U.shape_cases(shape), bands):
            assert (lo == 0).all() and (hi == len(read) + 1).all()
        assert np.array_equal(U.family_scores(shape, "full"), U.full_scores(shape)), U.shape_id(shape)


def closed_form(d, ca, cb, m, n):
    """The band as the comment at vtxf::band_pack (vtx_fast_core.h) states it: column j is in band for j in [ca - W, cb + W], rows
    [max(0, max(j - W, ca) - d - W), min(m + 1, min(j + W, cb) - d + W + 1))."""
    lo, hi = U.empty_band(n)
    for j in range(max(0, ca - W), min(n, cb + W) + 1):
        lo_, hi_ = max(0, max(j - W, ca) - d - W), min(m + 1, min(j + W, cb) - d + W + 1)
        if lo_ < hi_:
            lo[j], hi[j] = lo_, hi_
    return lo, hi


def test_squares_model_equals_the_documented_closed_form():
    rng = np.random.default_rng(2024)
    for it in range(400):
        m, n = int(rng.integers(6, 257)), int(rng.integers(6, 256))
        d = int(rng.integers(-(m - 6), n - 6 + 1))
        if it % 8 == 0:
            d = -(m - 6) if it % 16 else n - 6                  # (both ends of its range)
        ca = int(rng.integers(0, n + 1))
        cb = int(rng.integers(ca, n + 1))
        if it % 5 == 0:
            cb = ca
        assert U.same_band(U.squares_band(d, ca, cb, m, n), closed_form(d, ca, cb, m, n)), (d, ca, cb, m, n)


def test_squares_model_reproduces_band_create_on_exact_substrings():
    """A read that is an exact substring of its haplotype at offset o has its chain on diagonal o: for some stretch (ca, cb) near
    (o, o + m) the model with d = o IS band_create's band, column for column."""
    rng = np.random.default_rng(31)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    found = 0
    cases = 60
    for _ in range(cases):
        n = int(rng.integers(60, 256))
        m = int(rng.integers(30, n + 1))
        o = int(rng.integers(0, n - m + 1))
        hap = bytes(acgt[rng.integers(0, 4, n)])
        read = hap[o:o + m]
        want = U.oracle_band(read, hap)
        hit = None
        for ca in range(max(o - 2, 0), o + 14):
            for cb in range(o + m - 14, min(o + m + 2, n) + 1):
                if ca <= cb and U.same_band(U.squares_band(o, ca, cb, m, n), want):
                    hit = (ca, cb)
                    break
            if hit:
                break
        found += hit is not None
    assert found == cases, "%d of %d" % (found, cases)


def shares(shape, family):
    got, full = U.family_scores(shape, family), U.full_scores(shape)
    assert (got <= full).all()
    return float((got > 0).mean()), float((got < full).mean()), int((got < full).sum())


@pytest.mark.parametrize("family", ["random", "stripe", "shifted"])
def test_bands_decide_the_scores(family):
    """No vacuous pass: in every (shape, family) cell at least 90 % of the tasks score above 0 and at least half score below the
    full-matrix score, so a kernel that ignored its band, or saw none of it, would be caught.  (shifted, reads above 256 bases: the
    haplotypes end at 255 bases, a shift of a long read's band costs it little; at least one task must differ.)"""
    for shape in U.SHAPES:
        pos, below, n_below = shares(shape, family)
        print("%s %s: above 0 %.3f, below full %.3f" % (U.shape_id(shape), family, pos, below))
        assert pos >= 0.9, (shape, family, pos)
        if family == "shifted" and U.capacity(shape) > 256:
            assert n_below >= 1, (shape, family)
        else:
            assert below >= 0.5, (shape, family, below)


def test_case_set_is_what_the_gpu_test_says_it_is():
    for shape in U.SHAPES:
        cases = U.shape_cases(shape)
        cap, prev = U.capacity(shape), U.prev_capacity(shape)
        ms = {len(r) for r, _, _ in cases}
        ns = {len(h) for _, h, _ in cases}
        assert {cap, cap - 1, prev + 1, 1, 7} <= ms and any(20 <= x <= 40 and x < cap - 1 for x in ms) and max(ms) == cap
        assert {1, 255} <= ns and min(ns) >= 1 and max(ns) <= 255
        blob = b"".join(r + h for r, h, _ in cases)
        assert b"N" in blob and any(c in blob for c in b"acgt")
