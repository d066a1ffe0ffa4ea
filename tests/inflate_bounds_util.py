"""Shared by tests/test_inflate_bounds.py and tests/test_gpu_ingest.py: the hostile DEFLATE corpus (streams cut short, hand-made
blocks whose input or output runs out) and the stand-alone host build of vartrix_amd/csrc/vtx_inflate_core.h that runs it in exactly
sized allocations (tests/inflatecore/harness.cpp).  The reference is zlib.decompressobj(-15)."""
import collections
import functools
import os
import random
import struct
import subprocess
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ST_OK, ST_BAD_DIST, ST_OVERRUN, ST_INPUT = 0, 5, 6, 8
FILLS = (0x00, 0xFF, 0xA5)

# expect: ST_* where the status is known by construction (every proper prefix of a valid stream: ST_INPUT), None: any status but
# ST_OK unless zlib accepts.  whole: the name of the valid stream this one is a prefix of (its trip count bounds this one's).
Case = collections.namedtuple("Case", "name raw out_len expect whole")


def zlib_verdict(raw, n):
    """zlib's bytes when it reads exactly one complete stream of n bytes from raw, else None."""
    try:
        d = zlib.decompressobj(-15)
        z = d.decompress(raw) + d.flush()
    except zlib.error:
        return None
    return z if d.eof and len(z) == n and not d.unused_data else None


# ---------------------------------------------------------------------------------------------------------------------------
# bit-level authoring
# ---------------------------------------------------------------------------------------------------------------------------
def lsb(v, n):
    return [(v >> i) & 1 for i in range(n)]


def msb(v, n):
    return [(v >> (n - 1 - i)) & 1 for i in range(n)]


def to_bytes(bits):
    out = bytearray((len(bits) + 7) // 8)
    for i, b in enumerate(bits):
        out[i >> 3] |= b << (i & 7)
    return bytes(out)


def canonical(lengths):
    """{symbol: length} -> {symbol: bits, first bit of the stream first} (RFC 1951 3.2.2)."""
    code, out = 0, {}
    for ln in range(1, 16):
        for s in sorted(k for k, v in lengths.items() if v == ln):
            out[s] = msb(code, ln)
            code += 1
        code <<= 1
    return out


def fixed_ll(sym):
    if sym < 144:
        return msb(0x30 + sym, 8)
    if sym < 256:
        return msb(0x190 + sym - 144, 9)
    if sym < 280:
        return msb(sym - 256, 7)
    return msb(0xC0 + sym - 280, 8)


def fixed_block(symbols):
    """A final fixed-Huffman block: symbols are literal / length symbols (no extra bits: lengths 3..10 and 258) or ("d", n): distance
    symbol n < 4."""
    bits = [1] + lsb(1, 2)
    for s in symbols:
        bits += msb(s[1], 5) if isinstance(s, tuple) else fixed_ll(s)
    return to_bytes(bits)


HAND_SHIFTS = (0, 1, 2, 3)
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def hand_dynamic(shift=0):
    """A valid final dynamic block written bit by bit, its code lengths sent with all three repeat codes, behind `shift` empty fixed
    blocks of 10 bits each (they move every field against the byte boundaries): (raw, output, fields) with fields = [(class, first
    bit, bit behind it)] for HLIT, HDIST, HCLEN, each 3-bit length, each repeat's extra bits."""
    ll = {s: 4 for s in list(range(65, 73)) + list(range(97, 101))}
    ll[256] = ll[257] = 3
    dl = {0: 1, 1: 1}
    cl = {18: 2, 4: 2, 16: 3, 17: 3, 3: 3, 1: 3}
    clc, llc, dc = canonical(cl), canonical(ll), canonical(dl)
    bits, fields = ([0] + lsb(1, 2) + fixed_ll(256)) * shift + [1] + lsb(2, 2), []

    def field(kind, b):
        fields.append((kind, len(bits), len(bits) + len(b)))
        bits.extend(b)

    field("HLIT", lsb(258 - 257, 5))
    field("HDIST", lsb(2 - 1, 5))
    field("HCLEN", lsb(18 - 4, 4))
    for s in CL_ORDER[:18]:
        field("len3", lsb(cl.get(s, 0), 3))
    # (symbol of the code-length code, extra value): 65 zeros, 65..72 -> 4, 24 zeros, 97..100 -> 4, 155 zeros, 256 257 -> 3, 1 1
    seq = [(18, 54), (4, None), (16, 3), (4, None), (18, 13), (4, None), (16, 0), (18, 127), (17, 7), (17, 4), (3, None), (3, None), (1, None), (1, None)]
    total = 0
    for s, extra in seq:
        bits.extend(clc[s])
        if s >= 16:
            field("rep%d" % s, lsb(extra, {16: 2, 17: 3, 18: 7}[s]))
        total += {16: 3, 17: 3, 18: 11}.get(s, 1) + (extra or 0) if s >= 16 else 1
    assert total == 258 + 2
    for s in (65, 66, 97):
        bits.extend(llc[s])
    bits.extend(llc[257] + dc[0])              # length 3, distance 1
    bits.extend(llc[256])
    return to_bytes(bits), b"ABaaaa", fields


# ---------------------------------------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------------------------------------
def deflate(data, level=9, strat=zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strat)
    if flush_at is None:
        return co.compress(data) + co.flush()
    return co.compress(data[:flush_at]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(data[flush_at:]) + co.flush()


def long_code_streams():
    """The 15-bit-code streams of tests/test_inflate_core.py::test_long_huffman_codes: [(raw, data)]."""
    rng = random.Random(3)
    out = []
    for trial in range(6):
        syms = list(range(256))
        rng.shuffle(syms)
        data = bytearray()
        while len(data) < 60000:
            k = 0
            while k < 40 and rng.random() < 0.62:
                k += 1
            data.append(syms[k * 6 % 256 if k < 40 else rng.randrange(256)])
        data = bytes(data)
        for strat in (zlib.Z_HUFFMAN_ONLY, zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED):
            out.append((deflate(data, 9, strat), data))
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    """The cases, in a fixed order; built once per process."""
    rng = random.Random(20261019)
    skew = bytes(min(int(rng.expovariate(2.5)), 255) for _ in range(2000))
    small = bytes(rng.choice(b"ACGTTTTN") for _ in range(70))
    wholes = [("fixed", deflate(small, 9, zlib.Z_FIXED), small),
              ("dynamic", deflate(skew), skew),
              ("two blocks", deflate(skew[:600], 9, flush_at=200), skew[:600]),
              ("stored", deflate(small[:60], 0), small[:60])]
    assert 30 <= len(wholes[0][1]) <= 60 and 100 <= len(wholes[1][1]) <= 300, [len(w[1]) for w in wholes]
    assert wholes[0][1][0] & 6 == 2 and wholes[1][1][0] & 6 == 4 and wholes[3][1][0] & 6 == 0         # BTYPE fixed, dynamic, stored
    assert b"\x00\x00\xff\xff" in wholes[2][1]                                                     # the stored empty block of Z_FULL_FLUSH
    for shift in HAND_SHIFTS:
        hd_raw, hd_out, _ = hand_dynamic(shift)
        wholes.append(("hand-made dynamic %d" % shift, hd_raw, hd_out))
    cases = []
    for name, raw, data in wholes:
        assert zlib_verdict(raw, len(data)) == data, name
        cases.append(Case(name, raw, len(data), ST_OK, None))
        for k in range(len(raw)):
            cases.append(Case("%s[:%d]" % (name, k), raw[:k], len(data), ST_INPUT, name))
    for i, (raw, data) in enumerate(long_code_streams()):
        name = "long codes %d" % i
        cases.append(Case(name, raw, len(data), ST_OK, None))
        for cut in (len(raw) // 4, len(raw) // 2, len(raw) - 1):
            cases.append(Case("%s[:%d]" % (name, cut), raw[:cut], len(data), ST_INPUT, name))
    # hand-made
    no_eob = bytes.fromhex("fbffffff")             # a final fixed block: 255 255 255 and two more bits, no end-of-block
    cases += [Case("no end-of-block, out_len 1", no_eob, 1, ST_OVERRUN, None), Case("no end-of-block, out_len 2", no_eob, 2, ST_OVERRUN, None),
              Case("no end-of-block, out_len 258", no_eob, 258, ST_INPUT, None), Case("no end-of-block, out_len 65280", no_eob, 65280, ST_INPUT, None)]
    stored5 = b"\x01\x05\x00\xfa\xff" + b"HELLO"
    cases += [Case("stored whole", stored5, 5, ST_OK, None), Case("stored: LEN one past in_len", stored5[:-1], 5, ST_INPUT, "stored whole")]
    m258 = fixed_block([97, 285, ("d", 0), 256])
    cases += [Case("match of 258 ends at out_len - 1", m258, 259, ST_OK, None),
              Case("match of 258 ends at out_len", fixed_block([97, 97, 285, ("d", 0), 256]), 259, ST_OVERRUN, None),
              Case("match of 258, out_len one less", m258, 258, ST_OVERRUN, None),
              Case("distance 1 at op 0", fixed_block([257, ("d", 0), 256]), 3, ST_BAD_DIST, None)]
    for k in range(4):
        cases += [Case("in_len %d of a stored block" % k, stored5[:k], 5, ST_INPUT, "stored whole"),
                  Case("in_len %d of ff bytes" % k, b"\xfb\xff\xff"[:k], 5, ST_INPUT, None)]
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def dynamic_header_cuts():
    """Per field class of the hand-made dynamic headers, the cases ("hand-made dynamic S[:K]") that end at the field's first bit or
    inside it."""
    cuts = collections.defaultdict(set)
    for shift in HAND_SHIFTS:
        raw, _, fields = hand_dynamic(shift)
        for kind, a, b in fields:
            for k in range(len(raw)):
                if a <= 8 * k < b:
                    cuts[kind].add("hand-made dynamic %d[:%d]" % (shift, k))
    return cuts


# ---------------------------------------------------------------------------------------------------------------------------
# the stand-alone program
# ---------------------------------------------------------------------------------------------------------------------------
def harness(san=False):
    name = "inflate_host_san" if san else "inflate_host"
    subprocess.check_call(["make", "-C", os.path.join(HERE, "inflatecore"), "-s", name])
    return os.path.join(HERE, "inflatecore", name)


Result = collections.namedtuple("Result", "status trips pad_ok out")


def run_program(cases, fill, tmp, san=False):
    """Every case in ONE process, the slack behind payload and output filled with `fill`: [Result] (out: bytes when accepted)."""
    src, dst = os.path.join(tmp, "cases_%02x.bin" % fill), os.path.join(tmp, "results_%02x.bin" % fill)
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            f.write(struct.pack("<III", len(c.raw), c.out_len, fill) + c.raw)
    r = subprocess.run([harness(san), src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, "exit %d\n%s" % (r.returncode, r.stderr[-4000:])
    blob, p, res = open(dst, "rb").read(), 0, []
    for _ in cases:
        st, trips, pad_ok, m = struct.unpack_from("<IIII", blob, p)
        res.append(Result(st, trips, pad_ok, blob[p + 16:p + 16 + m] if st == ST_OK else None))
        p += 16 + m
    assert p == len(blob)
    return res
