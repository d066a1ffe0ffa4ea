"""The byte compare and the base codes of vartrix_amd/csrc/vtx_fast_core.h (eq8, kw_code8, kw_code) have two paths: dot products
(v_dot4_u32_u8) in device code, shifts and ors in every host build of the header.  Both are run here on the same 8-byte words — the
device path through libvtx_dev.so's vtxk_dev_byteops, the portable path through tests/fastcore/byteops_host.cpp, compiled here — and
compared with the DEFINITIONS, written in numpy: bit i of eq8 is (byte i of a == byte i of b); a code has (byte >> 1) & 3 of base i at
bits 2 i (eight bases: kw_code8; the low six: kw_code), whatever the byte.  And with each other."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def vectors():
    rng = np.random.default_rng(1507)
    A, B = [], []

    def add(a, b):
        A.append(np.asarray(a, np.uint8).reshape(-1, 8))
        B.append(np.asarray(b, np.uint8).reshape(-1, 8))

    # every byte value against itself, value ^ 0x80, value ^ 0x01 and ~value, at each of the eight positions; the other seven bytes
    # are equal in a and b (random, so a flag that leaks into a neighbour shows)
    v = np.arange(256, dtype=np.uint8)
    for pos in range(8):
        for other in (v, v ^ 0x80, v ^ 0x01, ~v):
            a = rng.integers(0, 256, (256, 8), dtype=np.uint8)
            b = a.copy()
            a[:, pos], b[:, pos] = v, other
            add(a, b)
    # a ^ b = 0xff next to 0x00, in both orders, at every pair of neighbouring positions, over an all-zero, an all-ones and a random a:
    # the non-zero test adds 0x7f to the low seven bits of every byte, and no carry may reach the neighbour
    for pos in range(7):
        for z0, z1 in ((0xff, 0x00), (0x00, 0xff)):
            for a in (np.zeros(8, np.uint8), np.full(8, 0xff, np.uint8), rng.integers(0, 256, 8, dtype=np.uint8)):
                z = np.zeros(8, np.uint8)
                z[pos], z[pos + 1] = z0, z1
                add(a, a ^ z)
    # 0xff / 0x00 alternating over the whole word
    add([0xff, 0, 0xff, 0, 0xff, 0, 0xff, 0], np.zeros(8, np.uint8))
    add([0, 0xff, 0, 0xff, 0, 0xff, 0, 0xff], np.zeros(8, np.uint8))
    # all-equal and all-different words
    a = rng.integers(0, 256, (32, 8), dtype=np.uint8)
    add(a, a)
    add(a, a ^ rng.integers(1, 256, (32, 8), dtype=np.uint8))
    add(np.zeros(8, np.uint8), np.zeros(8, np.uint8))
    add(np.full(8, 0xff, np.uint8), np.full(8, 0xff, np.uint8))
    add(np.zeros(8, np.uint8), np.full(8, 0xff, np.uint8))
    # random pairs over ACGTN and over all 256 values
    acgtn = np.frombuffer(b"ACGTN", np.uint8)
    add(acgtn[rng.integers(0, 5, (400, 8))], acgtn[rng.integers(0, 5, (400, 8))])
    add(rng.integers(0, 256, (400, 8), dtype=np.uint8), rng.integers(0, 256, (400, 8), dtype=np.uint8))
    return np.ascontiguousarray(np.concatenate(A)), np.ascontiguousarray(np.concatenate(B))


def by_definition(a, b):
    """(eq8, kw_code8, kw_code) of the rows of a and b (n x 8 bytes, byte i of a word = column i)."""
    i = np.arange(8, dtype=np.uint32)
    eq = ((a == b).astype(np.uint32) << i).sum(axis=1, dtype=np.uint32)
    two = (a.astype(np.uint32) >> 1) & 3
    code8 = (two << (2 * i)).sum(axis=1, dtype=np.uint32)
    code6 = (two[:, :6] << (2 * i[:6])).sum(axis=1, dtype=np.uint32)
    return eq, code8, code6


def run(fn, a, b):
    n = len(a)
    wa, wb = a.view("<u8").reshape(-1), b.view("<u8").reshape(-1)
    out = np.full(3 * n, 0xdeadbeef, np.uint32)
    rc = fn(wa.ctypes.data_as(C.c_void_p), wb.ctypes.data_as(C.c_void_p), C.c_uint32(n), out.ctypes.data_as(C.c_void_p))
    return rc, (out[:n], out[n:2 * n], out[2 * n:])


def test_device_and_host_byte_ops_match_their_definitions():
    from vartrix_amd import lib
    a, b = vectors()
    assert 4000 <= len(a) <= 10000
    want = by_definition(a, b)

    dev = C.CDLL(lib.lib_path("dev"))
    dev.vtxk_dev_byteops.restype = C.c_int
    dev.vtxk_dev_byteops.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    rc, got_dev = run(dev.vtxk_dev_byteops, a, b)
    assert rc == 0, "vtxk_dev_byteops: hipError %d" % rc

    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libbyteops_host.so")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "fastcore", "byteops_host.cpp")],
                              timeout=300)
        host = C.CDLL(so)
        host.fastcore_byteops.restype = None
        host.fastcore_byteops.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        _, got_host = run(host.fastcore_byteops, a, b)

    for name, w, d, h in zip(("eq8", "kw_code8", "kw_code"), want, got_dev, got_host):
        for path, g in (("device", d), ("host", h)):
            bad = np.nonzero(g != w)[0]
            assert len(bad) == 0, "%s, %s path: %d of %d words differ from the definition; first: a = %s b = %s got %#x want %#x" % (
                name, path, len(bad), len(w), bytes(a[bad[0]]).hex(), bytes(b[bad[0]]).hex(), int(g[bad[0]]), int(w[bad[0]]))
        assert np.array_equal(d, h), "%s: device and host paths differ" % name
