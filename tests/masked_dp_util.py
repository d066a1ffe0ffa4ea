"""Shared by tests/test_masked_dp_model.py (CPU) and tests/test_gpu_masked_dp.py (GPU): the tasks, the bands and the driver of the
direct tests of sw_banded_kernel (vartrix_amd/csrc/vtx_kernels.hip) against the oracle's range-restricted DP (oracle.sw_ranges).

  * cases: (read, haplotype) pairs per kernel shape — reads at the shape's capacity, one below it, one above the previous shape's,
    1, 7 and 20 - 40 bases; haplotypes of 1 .. 255 bases; a read is a noisy stretch of the sequence its haplotype is cut from, with
    one indel, so that scores are large; ACGT with a few N and lower-case bytes.
  * bands: per-column row ranges [lo, hi) in the oracle's coordinates (row ii = read index + 1, column jj = haplotype index + 1,
    row / column 0 = boundary), index jj = 0 .. n; an empty column is (EMPTY_LO, 0).  The families of the issue: full, oracle,
    shifted, random, stripe, and the degenerate bands.
  * squares_band: the band of one band_pack word, written as the literal union of the (2 w + 1)-squares around the cells
    (c - d, c), c = ca .. cb — an independent model of what sw_banded_kernel<.., 2> expands in LDS from a closed form.
  * Problem / run_pairs: a batch in host arrays and one launch through libvtx_dev.so's vtxk_dev_sw_pairs.
"""
import ctypes as C
import functools

import numpy as np

from oracle import oracle
from vartrix_amd.abi import LOCUS_DTYPE, RECORD_DTYPE

SHAPES = ((2, 16), (4, 16), (6, 16), (8, 16), (10, 16), (12, 16), (16, 16), (8, 64), (16, 64))   # kShapes of vtx_api.hip
W = 20                                   # band half-width (src/main.rs:34)
EMPTY_LO = 0x7fff
STAGE_FULL_CHECK, STAGE_DIAG_DP = 3, 7   # include/vtx.h
SCORE_POISON, STAGE_POISON = -123456789, 0xa5
HIP_INVALID_VALUE = 1
FAMILIES = ("full", "oracle", "shifted", "random", "stripe")
N_CASES = 128

_ACGT = np.frombuffer(b"ACGT", np.uint8)


def shape_id(shape):
    return "R%dxGL%d" % shape


def capacity(shape):
    return shape[0] * shape[1]


def prev_capacity(shape):
    i = SHAPES.index(shape)
    return capacity(SHAPES[i - 1]) if i else 0


# ---------------------------------------------------------------- cases
def _spoil(rng, s):
    """a few N and lower-case bytes (byte equality: neither matches its upper-case base)"""
    s = s.copy()
    r = rng.random(len(s))
    s[r < 0.01] = ord("N")
    low = (r >= 0.01) & (r < 0.02)
    s[low] |= 0x20
    return s


def make_case(rng, m, n):
    """(read, hap, d): a read of exactly m bases and a haplotype of n, both cut from one random sequence; the read carries ~3 %
    substitutions and (from 12 bases) one indel.  Read index i lies on haplotype index i + d, up to the indel."""
    g = _ACGT[rng.integers(0, 4, max(m, n) + 2 * n + 2)]
    if m <= n:
        a, b = 0, int(rng.integers(0, n - m + 1))
    else:                                # the haplotype anywhere along the read, up to half of it beyond either end of the read
        b = n
        a = b + int(rng.integers(-(n // 2), m - n + n // 2 + 1))
    hap = g[a:a + n]
    if m >= 12:
        p = int(rng.integers(4, m - 4))
        if rng.random() < 0.5:                                   # a deletion in the read
            src = g[b:b + m + 1]
            read = np.concatenate([src[:p], src[p + 1:]])
        else:                                                    # an insertion
            src = g[b:b + m - 1]
            read = np.concatenate([src[:p], _ACGT[rng.integers(0, 4, 1)], src[p:]])
    else:
        read = g[b:b + m].copy()
    assert len(read) == m and len(hap) == n
    sub = rng.random(m) < 0.03
    read = np.where(sub, _ACGT[rng.integers(0, 4, m)], read).astype(np.uint8)
    return bytes(_spoil(rng, read)), bytes(_spoil(rng, hap)), b - a


def read_lengths(shape):
    """The read lengths of a shape's cases, most of them long: name -> (length or (lo, hi) range, number of cases)."""
    cap, prev = capacity(shape), prev_capacity(shape)
    out = {"one": (1, 2), "seven": (7, 3), "short": ((20, min(40, cap - 2)), 12)}
    rest = N_CASES - 17
    if prev + 1 > 1:
        out.update({"cap": (cap, rest // 3 + rest % 3), "cap-1": (cap - 1, rest // 3), "prev+1": (prev + 1, rest // 3)})
    else:                                                        # (the first shape: the previous capacity + 1 is the 1-base read)
        out.update({"cap": (cap, rest - rest // 2), "cap-1": (cap - 1, rest // 2)})
    return out


@functools.lru_cache(maxsize=None)
def shape_cases(shape):
    """N_CASES (read, hap, d) of a shape; haplotypes of 1 .. 255 bases, both ends among them."""
    rng = np.random.default_rng(9000 + 100 * shape[0] + shape[1])
    lens = []
    for name, (v, cnt) in read_lengths(shape).items():
        for _ in range(cnt):
            lens.append(v if isinstance(v, int) else int(rng.integers(v[0], v[1] + 1)))
    assert len(lens) == N_CASES
    haps = [int(x) for x in rng.integers(1, 256, N_CASES)]
    order = rng.permutation(N_CASES)
    lens = [lens[i] for i in order]
    for i, n in enumerate((255, 1, 254, 2, 6, 41)):              # fixed haplotype lengths, whatever read they meet
        haps[7 * i + 3] = n
    return tuple(make_case(rng, m, n) for m, n in zip(lens, haps))


# ---------------------------------------------------------------- bands
def empty_band(n):
    return np.full(n + 1, EMPTY_LO, np.int32), np.zeros(n + 1, np.int32)


def normalise(lo, hi, m):
    """int32 copies with every empty column as (EMPTY_LO, 0); the others must lie in 0 <= lo < hi <= m + 1 (the oracle indexes
    its m + 1 rows with them, the kernel reads them as signed 16-bit values)."""
    lo, hi = np.array(lo, np.int32), np.array(hi, np.int32)
    e = hi <= lo
    lo[e], hi[e] = EMPTY_LO, 0
    assert ((lo[~e] >= 0) & (hi[~e] <= m + 1)).all()
    return lo, hi


def same_band(a, b):
    """two bands hold the same cells (empty columns compare as empty)"""
    (alo, ahi), (blo, bhi) = a, b
    ae, be = ahi <= alo, bhi <= blo
    return len(alo) == len(blo) and np.array_equal(ae, be) and np.array_equal(alo[~ae], blo[~be]) and np.array_equal(ahi[~ae], bhi[~be])


def full_band(m, n):
    return np.zeros(n + 1, np.int32), np.full(n + 1, m + 1, np.int32)


def oracle_band(read, hap):
    lo, hi, _ = oracle.band_create(read, hap)
    return normalise(lo, hi, len(read))


def shifted_band(rng, read, hap):
    """band_create's band moved by +- 1 .. 30 rows and clipped to the matrix"""
    m = len(read)
    lo, hi = oracle_band(read, hap)
    s = int(rng.integers(1, 31)) * (1 if rng.random() < 0.5 else -1)
    e = hi <= lo
    lo2, hi2 = np.clip(lo + s, 0, m + 1), np.clip(hi + s, 0, m + 1)
    lo2[e], hi2[e] = EMPTY_LO, 0
    return normalise(lo2, hi2, m)


def random_band(rng, m, n):
    """independent lo <= hi per column; a fifth of the columns empty, as the kernels write them: lo = 0x7fff, hi = 0"""
    p = np.sort(rng.integers(0, m + 2, (n + 1, 2)), axis=1)
    lo, hi = p[:, 0].astype(np.int32), p[:, 1].astype(np.int32)
    e = rng.random(n + 1) < 0.2
    lo[e], hi[e] = EMPTY_LO, 0
    return lo, hi                                                # (lo == hi stays as it is: an empty column of another spelling)


def stripe_band(rng, m, n, R):
    """the same range in every column, its ends on a lane's first or last row, +- 1: lane l owns rows l R + 1 .. l R + R"""
    lanes = (m + R - 1) // R
    a = int(rng.integers(0, lanes))
    b = int(rng.integers(a, lanes))
    lo = a * R + int(rng.integers(0, 2))
    hi = min(b * R + R + int(rng.integers(0, 2)), m + 1)
    if lo >= hi:
        lo = hi - 1
    return np.full(n + 1, lo, np.int32), np.full(n + 1, hi, np.int32)


def family_band(family, rng, read, hap, shape):
    m, n = len(read), len(hap)
    if family == "full":
        return full_band(m, n)
    if family == "oracle":
        return oracle_band(read, hap)
    if family == "shifted":
        return shifted_band(rng, read, hap)
    if family == "random":
        return random_band(rng, m, n)
    if family == "stripe":
        return stripe_band(rng, m, n, shape[0])
    raise ValueError(family)


@functools.lru_cache(maxsize=None)
def family_bands(shape, family):
    """the band of every case of shape_cases(shape), as a tuple of (lo, hi)"""
    rng = np.random.default_rng(77 + 1000 * FAMILIES.index(family) + 100 * shape[0] + shape[1])
    return tuple(family_band(family, rng, r, h, shape) for r, h, _ in shape_cases(shape))


def ranges_score(read, hap, lo, hi):
    m = len(read)
    lo, hi = np.asarray(lo, np.int32), np.asarray(hi, np.int32)
    assert len(lo) == len(hi) == len(hap) + 1 and lo.min() >= 0 and hi.max() <= m + 1 and hi.min() >= 0
    return int(oracle.sw_ranges(read, hap, lo, hi))


@functools.lru_cache(maxsize=None)
def family_scores(shape, family):
    """oracle.sw_ranges of every case under its family band (computed once, shared by the tests)"""
    return np.array([ranges_score(r, h, lo, hi) for (r, h, _), (lo, hi) in zip(shape_cases(shape), family_bands(shape, family))], np.int32)


@functools.lru_cache(maxsize=None)
def full_scores(shape):
    return np.array([oracle.sw_full(r, h) for r, h, _ in shape_cases(shape)], np.int32)


def degenerate_bands(read, hap):
    """name -> (lo, hi): the bands at the edges of the kernel's mask arithmetic"""
    m, n = len(read), len(hap)
    out = {}
    out["all_empty"] = empty_band(n)
    # one cell: the middle of the matrix, and a cell where the bases match if there is one
    lo, hi = empty_band(n)
    j, i = (n + 1) // 2, (m + 1) // 2
    lo[j], hi[j] = i, i + 1
    out["one_cell"] = (lo, hi)
    hit = [(i, j) for j in range(1, n + 1) for i in range(1, m + 1) if read[i - 1] == hap[j - 1]][:1]
    if hit:                                  # (a cell alone scores 0 even where its bases match: a match counts from an in-band diagonal neighbour)
        (i, j), = hit
        lo, hi = empty_band(n)
        lo[j], hi[j] = i, i + 1
        out["one_matching_cell"] = (lo, hi)
        lo, hi = lo.copy(), hi.copy()
        lo[j - 1], hi[j - 1] = i - 1, i
        out["two_cells_on_a_diagonal"] = (lo, hi)
    out["row0_only"] = (np.zeros(n + 1, np.int32), np.ones(n + 1, np.int32))
    lo, hi = empty_band(n)
    lo[0], hi[0] = 0, m + 1
    out["col0_only"] = (lo, hi)
    # row 0 in band in the even columns, the band from row 1 in the odd ones
    out["row0_alternating"] = ((np.arange(n + 1) & 1).astype(np.int32), np.full(n + 1, m + 1, np.int32))
    out["from_row1_to_m"] = (np.ones(n + 1, np.int32), np.full(n + 1, m + 1, np.int32))       # hi = m + 1 exactly, without row 0
    out["last_row_only"] = (np.full(n + 1, m, np.int32), np.full(n + 1, m + 1, np.int32))
    return out


# ---------------------------------------------------------------- the band of a band_pack word
def band_pack(d, ca, cb):
    assert -256 <= d < 256 and 0 <= ca <= 255 and 0 <= cb <= 255
    return ((d + 256) << 16) | (ca << 8) | cb


def squares_band(d, ca, cb, m, n, w=W):
    """The union of the (2 w + 1)-squares around the cells (row c - d, column c), c = ca .. cb, clipped to rows 0 .. m and columns
    0 .. n, as (lo, hi) per column.  Written as that union: a matrix of flags, one square after the other."""
    inb = np.zeros((m + 1, n + 1), bool)
    for c in range(ca, cb + 1):
        r = c - d
        r0, r1, c0, c1 = max(r - w, 0), min(r + w, m), max(c - w, 0), min(c + w, n)
        if r0 <= r1 and c0 <= c1:
            inb[r0:r1 + 1, c0:c1 + 1] = True
    lo, hi = empty_band(n)
    for j in range(n + 1):
        rows = np.nonzero(inb[:, j])[0]
        if len(rows):
            assert rows[-1] - rows[0] + 1 == len(rows)           # (squares along one diagonal: a column's rows are one interval)
            lo[j], hi[j] = rows[0], rows[-1] + 1
    return lo, hi


# ---------------------------------------------------------------- a batch in host arrays, one launch
class Problem:
    """One record and one locus per case.  The case's haplotype is the locus's REF haplotype for even cases and its ALT haplotype for
    odd ones (task = 2 * record + haplotype); the other slot holds a decoy of another length, whose task is never listed."""

    def __init__(self, cases):
        self.reads = [c[0] for c in cases]
        self.haps = [c[1] for c in cases]
        n = len(cases)
        rb, hb = bytearray(b"\xee" * 5), bytearray(b"\xdd" * 3)
        self.records = np.zeros(n, RECORD_DTYPE)
        self.loci = np.zeros(n, LOCUS_DTYPE)
        for i, (read, hap) in enumerate(zip(self.reads, self.haps)):
            self.records[i] = (len(rb), len(read), i, 0)
            rb += read
            decoy = hap[::-1][:len(hap) // 2 + 3] + b"G"
            first, second = (hap, decoy) if i % 2 == 0 else (decoy, hap)
            self.loci[i] = (i, i, 1, len(hb), len(first), len(hb) + len(first), len(second), 0)
            hb += first + second
        self.rec_locus = np.arange(n, dtype=np.uint32)
        self.read_arena = np.frombuffer(bytes(rb), np.uint8).copy()
        self.hap_arena = np.frombuffer(bytes(hb), np.uint8).copy()
        self.tasks = (2 * np.arange(n) + (np.arange(n) & 1)).astype(np.uint32)
        self.n = n

    def scores_of(self, ref, alt):
        """the score of every case's task out of the two score arrays, and those of the decoy tasks"""
        odd = (np.arange(self.n) & 1).astype(bool)
        return np.where(odd, alt, ref), np.where(odd, ref, alt)


_dev = None


def dev_lib():
    global _dev
    if _dev is None:
        from vartrix_amd import lib
        L = C.CDLL(lib.lib_path("dev"))
        p, u32 = C.c_void_p, C.c_uint32
        L.vtxk_dev_sw_pairs.restype = C.c_int
        L.vtxk_dev_sw_pairs.argtypes = [p, u32, p, p, u32, p, C.c_uint64, p, C.c_uint64, p, u32, C.c_int, C.c_int, C.c_int, u32,
                                        p, u32, p, p, p, C.c_int64, C.c_int32, C.c_uint8, p, p, p, p, p, p]
        _dev = L
    return _dev


class Result:
    pass


def run_pairs(prob, order, mode, shape, max_hap_len, bands=None, packs=None, prov=None, n_dev=None, tasks=None):
    """One launch of sw_banded_kernel<R, GL, mode> over the cases `order` (indices into prob, in list order).
    bands: mode 0, (lo, hi) per list entry.  packs: modes 1 / 2, a word per list entry.  prov: mode 1, (ref, alt) provisional score
    arrays.  n_dev: the device-side list length, None for a null pointer.  tasks: raw task words instead of prob.tasks[order]
    (the argument checks).  Returns rc, and on success the arrays the hook hands back."""
    order = np.asarray(order, np.int64)
    lst = np.ascontiguousarray(prob.tasks[order] if tasks is None else tasks, np.uint32)
    nl, nr = len(lst), prob.n
    band, stride = None, 0
    if mode == 0:
        stride = max(len(lo) for lo, _ in bands)
        band = np.empty((nl, 2, stride), np.uint16)
        band[:, 0, :], band[:, 1, :] = 0, 0x7fff                 # (behind a slot's n + 1 entries: "every row in band" — nothing may read it)
        for s, (lo, hi) in enumerate(bands):
            assert len(lo) == len(hi) and lo.min() >= 0 and lo.max() <= 0x7fff and hi.min() >= 0 and hi.max() <= 0x7fff
            band[s, 0, :len(lo)], band[s, 1, :len(hi)] = lo, hi
    pk = None if packs is None else np.ascontiguousarray(packs, np.uint32)
    pr = pa = None
    if prov is not None:
        pr, pa = np.ascontiguousarray(prov[0], np.int32), np.ascontiguousarray(prov[1], np.int32)
    res = Result()
    res.ref, res.alt = np.zeros(nr, np.int32), np.zeros(nr, np.int32)
    res.stage = np.zeros(2 * nr, np.uint8)
    count = np.zeros(1, np.uint32)
    res.recheck_list, res.recheck_pack = np.zeros(max(nl, 1), np.uint32), np.zeros(max(nl, 1), np.uint32)

    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)
    res.rc = dev_lib().vtxk_dev_sw_pairs(
        ptr(prob.records), nr, ptr(prob.rec_locus), ptr(prob.loci), len(prob.loci), ptr(prob.read_arena), len(prob.read_arena),
        ptr(prob.hap_arena), len(prob.hap_arena), ptr(lst), nl, mode, shape[0], shape[1], max_hap_len, ptr(band), stride, ptr(pk),
        ptr(pr), ptr(pa), -1 if n_dev is None else int(n_dev), SCORE_POISON, STAGE_POISON, ptr(res.ref), ptr(res.alt), ptr(res.stage),
        ptr(count), ptr(res.recheck_list), ptr(res.recheck_pack))
    if res.rc not in (0, HIP_INVALID_VALUE):
        import pytest                                            # (a device error, not the hook's refusal: nothing more is started on this GPU)
        pytest.exit("vtxk_dev_sw_pairs: hipError %d (mode %d, %s, %d list entries)" % (res.rc, mode, shape_id(tuple(shape)), nl), returncode=3)
    res.recheck_count = int(count[0])
    res.score, res.decoy_score = prob.scores_of(res.ref, res.alt)
    res.task_stage = res.stage[prob.tasks]
    res.decoy_stage = res.stage[prob.tasks ^ 1]
    return res
