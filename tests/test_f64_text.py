"""CPU unit tests of vartrix_amd/csrc/vtx_f64_text.h — the per-lane formatter of Rust's `{}` text of an f64 that mtx_len_kernel<true> /
mtx_text_kernel<true> are compiled from (alt_frac's Matrix-Market values, sprs::io::write_matrix_market, src/main.rs:381-389) — built
for the host by tests/f64text/Makefile.  The yardstick is hostlib.format_f64 (vtxh_format_f64: std::to_chars, fixed), which
tests/test_host.py ties to the oracle and to the reference's test_frac.mtx: every comparison below is byte for byte and total over its
inputs.  The device runs the same source in tests/test_gpu_mtx_f64.py."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle
from vartrix_amd import hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
STRIDE = 48
CANARY = 0xCD


@pytest.fixture(scope="module")
def core():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "f64text"), "-s"])
    L = C.CDLL(os.path.join(HERE, "f64text", "libf64text_host.so"))
    L.vtxt_format.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]
    L.vtxt_format.restype = C.c_uint64
    L.vtxt_gen_ratios.argtypes = [C.c_uint32, C.c_void_p]
    L.vtxt_gen_ratios.restype = C.c_uint64
    L.vtxt_gen_frac.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.vtxt_gen_frac.restype = None
    L.vtxt_max_len.restype = C.c_uint32
    return L


def own(L, values):
    """f64_len / f64_put of every value: the texts (b"" = declined).  f64_put wrote exactly f64_len bytes: the canary behind them is whole."""
    v = np.ascontiguousarray(values, np.float64)
    n = len(v)
    ln = np.zeros(n, np.uint32)
    text = np.full((n, STRIDE), CANARY, np.uint8)
    assert L.vtxt_format(v.ctypes.data, n, ln.ctypes.data, text.ctypes.data, STRIDE) == 0, "f64_put did not end f64_len bytes behind its start"
    assert int(ln.max(initial=0)) <= L.vtxt_max_len()
    written = np.arange(STRIDE, dtype=np.uint32)[None, :] < ln[:, None]
    assert np.all(text[~written] == CANARY), "f64_put wrote beyond f64_len bytes"
    raw = text.tobytes()
    return [raw[i * STRIDE:i * STRIDE + int(ln[i])] for i in range(n)]


_buf = C.create_string_buffer(40)


def host_text(v) -> bytes:
    n = hostlib.load().vtxh_format_f64(float(v), _buf)       # (= hostlib.format_f64 without the decode)
    return _buf.raw[:n]


def bits(v) -> int:
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def from_bits(b) -> float:
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def check_equal_to_host(L, values):
    """Byte-identical to hostlib.format_f64 for every value (none skipped); parses back to the same bits; no text was cut by the host's
    31-byte limit: a cut text is exactly 31 bytes long, so every text of that length is also compared with oracle.format_f64, which has
    no limit.  Returns the longest text's length."""
    values = np.ascontiguousarray(values, np.float64)
    got = own(L, values)
    longest = 0
    for v, g in zip(values.tolist(), got):
        w = host_text(v)
        assert g == w, (v.hex() if v == v else v, g, w)
        longest = max(longest, len(g))
        if len(w) >= 31:
            assert w.decode() == oracle.format_f64(v), ("cut by the host's limit", v.hex(), w)
        if v == v:
            assert bits(float(g)) == bits(v), (v.hex(), g)
        else:
            assert g == b"NaN"
    return longest


def test_every_small_ratio(core):
    """Every a / t for 1 <= t <= 2048, 0 <= a <= t: what alt_frac produces from small counts (0, 1, halves, thirds, sevenths, ...)."""
    n = core.vtxt_gen_ratios(2048, None)
    assert n == sum(t + 1 for t in range(1, 2049))
    v = np.zeros(n, np.float64)
    core.vtxt_gen_ratios(2048, v.ctypes.data)
    assert v[0] == 0.0 and v[1] == 1.0 and v[3] == 0.5 and v[6] == 1 / 3
    assert check_equal_to_host(core, v) <= core.vtxt_max_len()


def test_random_counter_triples(core):
    """emit_coo_kernel's (double)a / ((double)r + a + k) for 10^6 random u32 triples: small counts, counts at the u32 limit, mixed; 0 / 0 is NaN."""
    rng = np.random.default_rng(20240)
    n = 1_000_000

    def counts():
        kind = rng.integers(0, 4, n)
        small = rng.integers(0, 8, n, dtype=np.uint64)
        mid = rng.integers(0, 1 << 16, n, dtype=np.uint64)
        big = np.uint64(0xFFFFFFFF) - rng.integers(0, 1 << 12, n, dtype=np.uint64)
        anyv = rng.integers(0, 1 << 32, n, dtype=np.uint64)
        return np.where(kind == 0, small, np.where(kind == 1, mid, np.where(kind == 2, big, anyv))).astype(np.uint32)

    a, r, k = counts(), counts(), counts()
    a[:4] = [0, 1, 1, 0xFFFFFFFF]
    r[:4] = [0, 0xFFFFFFFF, 0, 0xFFFFFFFF]
    k[:4] = [0, 0xFFFFFFFF, 0, 0xFFFFFFFF]
    v = np.zeros(n, np.float64)
    core.vtxt_gen_frac(a.ctypes.data, r.ctypes.data, k.ctypes.data, n, v.ctypes.data)
    assert math.isnan(v[0]) and v[1] == 1.0 / (2.0 * 4294967295.0 + 1.0) and v[2] == 1.0
    assert np.isnan(v).sum() > 10 and (v == 0).sum() > 100 and (v == 1).sum() > 100
    finite = v[np.isfinite(v) & (v > 0)]
    assert finite.min() >= 1.0 / (3.0 * 4294967296.0) and finite.max() <= 1.0
    assert check_equal_to_host(core, v) <= 29          # "0." + 10 zeros + 17 digits


def test_powers_of_two_and_their_neighbours(core):
    """At 2^e the double below is half as far away as the double above (the asymmetric interval): every power of two of the domain, both
    signs, with its two neighbours."""
    lo, hi = core.vtxt_min_exp2(), core.vtxt_max_exp2()
    vals = []
    for e in range(lo, hi + 1):
        p = math.ldexp(1.0, e)
        for x in (p, math.nextafter(p, math.inf)) + ((math.nextafter(p, 0.0),) if e > lo else ()):
            vals += [x, -x]
    vals.append(math.nextafter(math.ldexp(1.0, hi + 1), 0.0))          # the largest value of the domain
    assert len(vals) == (hi - lo + 1) * 6 - 2 + 1
    assert check_equal_to_host(core, vals) <= core.vtxt_max_len()


def test_seeds_zeros_nans_edges_and_random_bit_patterns(core):
    """The seeds of tests/test_host.py::test_mtx_writer_bytes, -0, NaN with payload and sign bits, the domain's edges, exact ties of the
    last digit (m * 2^-2: both one-digit candidates are equally far away), and 10^5 random bit patterns of the domain."""
    seeds = [(1.0, b"1"), (0.0, b"0"), (0.5, b"0.5"), (1 / 3, b"0.3333333333333333"), (float("nan"), b"NaN"), (2 / 3, b"0.6666666666666666"),
             (1 / 30000, b"0.000033333333333333335"), (7.0, b"7"), (-0.0, b"-0")]
    assert own(core, [v for v, _ in seeds]) == [s for _, s in seeds]
    nans = [from_bits(b) for b in (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF,
                                   0xFFFFFFFFFFFFFFFF, 0x7FF4000000000000, 0x7FF8000000BEEF00)]
    assert all(math.isnan(x) for x in nans) and own(core, nans) == [b"NaN"] * len(nans)
    lo, hi = core.vtxt_min_exp2(), core.vtxt_max_exp2()
    edge = [math.ldexp(1.0, lo), math.nextafter(math.ldexp(1.0, hi + 1), 0.0), 1.0 / (3.0 * 4294967296.0), 4294967296.0, 4294967295.5,
            4294967296.5, 0.1, 0.2, 0.3, 0.1 + 0.2, 1e-11, 1e-12 * 2, 123456.789, 9007199254740991.0, 4503599627370495.5]
    ties = [math.ldexp(1.0, 50) + q for q in (0.25, 0.75, 1.25, 1.75, 2.25, 1000.25, 1000.75)]
    rng = np.random.default_rng(7)
    be = rng.integers(1023 + lo, 1023 + hi + 1, 100_000, dtype=np.uint64)
    pat = (rng.integers(0, 2, 100_000, dtype=np.uint64) << np.uint64(63)) | (be << np.uint64(52)) | rng.integers(0, 1 << 52, 100_000, dtype=np.uint64)
    rnd = pat.view(np.float64)
    assert np.all(np.abs(rnd) >= math.ldexp(1.0, lo)) and np.all(np.abs(rnd) < math.ldexp(1.0, hi + 1))
    vals = np.concatenate([np.array(edge + ties), -np.array(edge + ties), rnd])
    assert check_equal_to_host(core, vals) <= core.vtxt_max_len()


def test_longest_text_and_the_lower_edge(core):
    """The bound the slab arithmetic of vtx_write_mtx_f64 uses (MAX_LEN = 31 bytes) is reached and never exceeded in the lowest binades, both
    signs, and the host's 31-byte limit cuts nothing there: in [10^-12, 2^-39) a text is "-0." + 11 zeros + at most 17 digits, in
    [2^-40, 10^-12) it has 12 zeros but 16 digits always suffice (neighbours 2^-92 = 2.02e-28 apart, 16-digit numbers 10^-28).  Two binades
    under the edge the yardstick itself is cut — it differs from the oracle's unbounded text — which is why the domain cannot go there."""
    lo = core.vtxt_min_exp2()
    assert lo == -40 and math.ldexp(1.0, lo) < 1.0 / (3.0 * 4294967296.0)
    rng = np.random.default_rng(11)
    n = 300_000
    be = rng.integers(1023 + lo, 1023 + lo + 3, n, dtype=np.uint64)
    pat = (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63)) | (be << np.uint64(52)) | rng.integers(0, 1 << 52, n, dtype=np.uint64)
    assert check_equal_to_host(core, pat.view(np.float64)) == core.vtxt_max_len() == 31
    below = float.fromhex("-0x1.2e1df8bb4cafcp-42")
    assert oracle.format_f64(below) == "-0.00000000000026833386765333515" and host_text(below) == b"-0.0000000000002683338676533351"
    assert own(core, [below]) == [b""]


def test_outside_the_domain_is_declined(core):
    lo, hi = core.vtxt_min_exp2(), core.vtxt_max_exp2()
    out = [math.inf, -math.inf, 5e-324, -5e-324, 2.2250738585072009e-308, math.ldexp(1.0, hi + 1), -math.ldexp(1.0, hi + 1), 1e300, -1e300,
           math.ldexp(1.0, lo - 1), -math.ldexp(1.0, lo - 1), math.nextafter(math.ldexp(1.0, lo), 0.0), 2.2250738585072014e-308, 1e-100]
    assert own(core, out) == [b""] * len(out)
