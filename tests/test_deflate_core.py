"""CPU unit tests of vartrix_amd/csrc/vtx_deflate_core.h — the lane and wavefront logic mtx_deflate_kernel is compiled from (the
DEFLATE encoder behind vtx_write_mtx_gz: one BGZF member per chunk of at most 65 280 bytes) — built for the host as a stand-alone
program by tests/deflatecore/Makefile, the 64 lanes as a loop.  The judge is Python's zlib: every member's raw stream inflates to its
chunk exactly, gzip reads the concatenation, BSIZE / CRC32 / ISIZE are checked by hand, no member exceeds n + 31 bytes, and the
project's own host inflater (vtxh_test_inflate) reads the members too.  A second build of the same program runs under AddressSanitizer
and UBSan over the same inputs (host code only; nothing is loaded into Python).  The device runs the same source in
tests/test_gpu_mtx_gz.py, which also pins device bytes == host bytes."""
import ctypes as C
import glob
import os
import random

import numpy as np
import pytest

import deflate_util as DU
from vartrix_amd import hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")


def host_inflate(stream, n):
    L = hostlib.load()
    out = C.create_string_buffer(max(n, 1))
    assert L.vtxh_test_inflate(stream, len(stream), out, n) == 1, "the host inflater declined a member"
    return out.raw[:n]


def no_repeat_text(rng, n):
    """Text in which no 4 bytes occur twice: the encoder finds no match, the distance alphabet stays empty."""
    seen, out = set(), bytearray(b"abc")
    while len(out) < n:
        b = rng.randrange(48, 112)
        k = bytes(out[-3:]) + bytes([b])
        if k in seen:
            continue
        seen.add(k)
        out.append(b)
    return bytes(out)


def fibonacci_bytes(rng):
    """40 symbols with Fibonacci frequencies (22 of them: 46 367 bytes) and 18 symbols once: an unlimited Huffman code is 21 deep."""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    syms = list(b"".join(bytes([40 + i]) * f for i, f in enumerate(fib + [1] * 18)))
    rng.shuffle(syms)
    return bytes(syms)


def alt_frac_text(tmp, n_lines):
    """hostlib.write_mtx's text of an alt_frac-like matrix: NaN, 0, 1, thirds, sevenths and other fractions, long row numbers."""
    rng = np.random.default_rng(11)
    row = np.sort(rng.integers(0, 3_000_000, n_lines)).astype(np.uint32)
    col = rng.integers(0, 10_000, n_lines).astype(np.uint32)
    den = rng.integers(1, 8, n_lines)
    val = rng.integers(0, 8, n_lines) % (den + 1) / den
    val[rng.random(n_lines) < 0.02] = np.nan
    val[rng.random(n_lines) < 0.3] = 1.0 / 3.0
    path = os.path.join(tmp, "frac.mtx")
    hostlib.write_mtx(path, 3_000_000, 10_000, row, col, val)
    text = open(path, "rb").read()
    assert text.count(b"\n") == n_lines + 3 and b" NaN\n" in text and b" 0.3333333333333333\n" in text and b"\n2999" in text
    return text


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """name -> bytes, built once; `big` is the 200 000-line text."""
    tmp = str(tmp_path_factory.mktemp("deflate"))
    rng = random.Random(20261018)
    c = {}
    for n in (0, 1, 3, 4, 5, 63, 64, 65, 257, 258, 259, 65279, 65280, 65281, 130561):
        c["text %d" % n] = (b"12 3456 1\n13 3456 2\n907 11 1\n" * (n // 28 + 1))[:n]
        c["run %d" % n] = b"7" * n                                     # distance 1, length-258 runs, a match that ends on the last byte
    for n in (1, 2, 3):
        c["single %d" % n] = b"x" * n
    for period in (32768, 32769):                                       # the distance limit: 32 768 is a legal distance, 32 769 is not
        c["period %d" % period] = (rng.randbytes(period) * 2)[:DU.CHUNK]
    c["all bytes"] = bytes(range(256))
    shuffled = list(range(256))
    rng.shuffle(shuffled)
    c["all bytes shuffled"] = bytes(shuffled)
    c["fibonacci"] = fibonacci_bytes(rng)
    c["no repeat"] = no_repeat_text(rng, 3000)
    c["random 65280"] = rng.randbytes(DU.CHUNK)
    for p in sorted(glob.glob(os.path.join(G, "*.mtx"))):
        c["fixture " + os.path.basename(p)] = open(p, "rb").read()
    assert sum(k.startswith("fixture") for k in c) >= 6
    c["big"] = alt_frac_text(tmp, 200_000)
    pieces = [v for k, v in c.items() if k != "big" and len(v) <= 70000] + [c["big"][:90000]]
    for i in range(300):                                                # seeded mixtures of the above, cut anywhere
        parts = []
        for _ in range(rng.randrange(1, 5)):
            v = rng.choice(pieces)
            a = rng.randrange(0, len(v) + 1)
            parts.append(v[a:a + rng.choice([3, 70, 700, 7000, 70000])])
        c["mix %d" % i] = b"".join(parts)[:rng.choice([5000, 5000, 5000, 66000, 140000])]
    return c


@pytest.fixture(scope="module")
def encoded(corpus, tmp_path_factory):
    names = list(corpus)
    out = DU.encode_many([corpus[k] for k in names], str(tmp_path_factory.mktemp("enc")))
    return dict(zip(names, out))


def test_every_member_inflates_to_its_chunk(corpus, encoded):
    kinds = {}
    for name, data in corpus.items():
        chunks = DU.cut(data)
        kinds[name] = DU.check_bgzf(encoded[name], chunks, inflate=host_inflate)
    assert len(DU.cut(corpus["text 65281"])) == 2 and len(DU.cut(corpus["text 130561"])) == 3
    assert kinds["random 65280"] == [0] and len(encoded["random 65280"]) == DU.CHUNK + 31 + 28       # stored: the guard
    assert kinds["run 65280"] == [2] and kinds["fibonacci"] == [2] and set(kinds["big"]) == {2}
    assert kinds["text 0"] == [1] and len(encoded["text 0"]) == 28 + 28                             # the empty member, fixed form: 2 bytes
    assert set(sum(kinds.values(), [])) == {0, 1, 2}                                              # every form occurs


def test_runs_and_periods_are_found(corpus, encoded):
    """A run of one byte costs a few hundred bytes (distance 1, length 258 all the way).  Random bytes with a period of 32 768 gain only
    through matches at exactly that distance, the largest DEFLATE can write: the member is smaller than its chunk (by how much
    depends on how many buckets still hold the position one period back: one candidate per bucket).  With a period of 32 769 nothing
    can be gained, and the chunk comes out stored."""
    assert len(encoded["run 65280"]) < 400
    n = len(corpus["period 32768"])
    assert len(encoded["period 32768"]) < n and len(encoded["period 32769"]) == n + 31 + 28


def test_text_without_a_repeat_has_no_distance_code_and_still_inflates(corpus, encoded):
    data = corpus["no repeat"]
    assert len({data[i:i + 4] for i in range(len(data) - 3)}) == len(data) - 3
    assert DU.check_bgzf(encoded["no repeat"], [data]) == [2]
    stream = encoded["no repeat"][18:]
    hdist = ((stream[0] | stream[1] << 8) >> 8) & 31
    assert hdist + 1 == 2          # no distance symbol in use: codes 0 and 1, one bit each — a complete code every inflater takes


def test_the_sanitizer_build_gives_the_same_bytes(corpus, encoded, tmp_path):
    names = list(corpus)
    out = DU.encode_many([corpus[k] for k in names], str(tmp_path), san=True)
    for k, z in zip(names, out):
        assert z == encoded[k], k


def test_compressed_size_against_zlib_level_1(corpus, encoded):
    """The DEFLATE streams of the 200 000-line alt_frac text against zlib's raw deflate at level 1 over the same 65 280-byte chunks:
    at most 15 % larger (one candidate per hash bucket against zlib's chains; both use dynamic Huffman codes).  Measured: 0.954."""
    chunks = DU.cut(corpus["big"])
    ours = sum(len(m) - 26 for m in DU.members(encoded["big"]))
    ref = DU.zlib1_stream_bytes(chunks)
    print("deflate bytes: encoder %d, zlib level 1 %d, ratio %.4f, of the text %.4f" % (ours, ref, ours / ref, ours / len(corpus["big"])))
    assert ours <= 1.15 * ref
