"""What vartrix_amd/csrc/vtx_inflate_core.h — the per-lane DEFLATE decoder of bgzf_inflate_kernel — TOUCHES and what decides its verdict
when the input runs out (CPU).  tests/test_inflate_core.py checks what the decoder answers on streams in over-sized buffers; here
every stream of the hostile corpus (tests/inflate_bounds_util.py: every byte-prefix of valid streams, 15-bit-code streams cut short,
hand-made blocks without an end-of-block, headers cut at each field) runs in a stand-alone program (tests/inflatecore/harness.cpp)
inside allocations of exactly the device's sizes — in_len + IN_PAD and out_len + OUT_PAD — once plain and once under AddressSanitizer
and UBSan, with the slack filled by 00, FF and A5.  Nothing sanitized is loaded into Python.  The reference is
zlib.decompressobj(-15).  The device runs the same corpus through the kernel in tests/test_gpu_ingest.py."""
import ctypes as C
import os
import subprocess

import pytest

import inflate_bounds_util as U

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """{fill: [Result]} of the plain program, one process per fill."""
    tmp = str(tmp_path_factory.mktemp("bounds"))
    return {f: U.run_program(U.corpus(), f, tmp) for f in U.FILLS}


def test_the_corpus_holds_what_it_should():
    cases = U.corpus()
    names = {c.name for c in cases}
    for whole in ("fixed", "dynamic", "two blocks", "stored"):
        n = len(next(c for c in cases if c.name == whole).raw)
        assert all("%s[:%d]" % (whole, k) in names for k in range(n)), whole            # every proper prefix, the empty one too
    cuts = U.dynamic_header_cuts()
    assert set(cuts) == {"HLIT", "HDIST", "HCLEN", "len3", "rep16", "rep17", "rep18"} and all(v <= names for v in cuts.values())
    for c in cases:                              # what the corpus calls valid is valid for zlib, what it calls hostile is not
        z = U.zlib_verdict(c.raw, c.out_len)
        assert (z is not None) == (c.expect == U.ST_OK), c.name


def test_the_sanitized_program_reports_nothing_and_agrees(plain, tmp_path):
    """ASan's red zone starts where the device's allocation of a LAST block would end: a load behind in_len + IN_PAD or
    out_len + OUT_PAD, or a store behind out_len + OUT_PAD, ends the program.  (run_program asserts exit 0 and an empty stderr.)"""
    for f in U.FILLS:
        assert U.run_program(U.corpus(), f, str(tmp_path), san=True) == plain[f], "fill %02x" % f


def test_status_trips_and_output_do_not_depend_on_the_slack(plain):
    cases = U.corpus()
    a, b, c = (plain[f] for f in U.FILLS)
    for case, x, y, z in zip(cases, a, b, c):
        assert x == y == z, (case.name, x[:3], y[:3], z[:3])
        assert x.pad_ok == 1, case.name                      # nothing written behind out_len


def test_every_proper_prefix_is_input_ran_out_and_no_later_than_the_whole(plain):
    cases = U.corpus()
    for f in U.FILLS:
        by_name = {c.name: r for c, r in zip(cases, plain[f])}
        n = 0
        for c, r in zip(cases, plain[f]):
            if c.whole is None:
                continue
            assert r.status == U.ST_INPUT, (c.name, f, r.status)
            assert r.trips <= by_name[c.whole].trips, (c.name, f, r.trips, by_name[c.whole].trips)
            n += 1
        assert n > 400


def test_verdicts_against_zlib_and_by_construction(plain):
    for c, r in zip(U.corpus(), plain[0xFF]):
        z = U.zlib_verdict(c.raw, c.out_len)
        if r.status == U.ST_OK:
            assert z is not None and r.out == z, c.name          # nothing zlib rejects is accepted; accepted bytes are zlib's
        if c.expect is not None:
            assert r.status == c.expect, (c.name, r.status)      # valid streams stay accepted; the hand-made ones fail the way they were made to


def test_the_shared_object_agrees_and_leaves_64_guard_bytes(plain):
    """The build the rest of the CPU suite (and the GPU test, as its expected statuses) uses — libinflate_host.so, the input in a
    buffer with 16 bytes of A5 behind it — gives the same status and trips, and the 64 bytes behind the output stay as they were."""
    subprocess.check_call(["make", "-C", os.path.join(HERE, "inflatecore"), "-s"])
    L = C.CDLL(os.path.join(HERE, "inflatecore", "libinflate_host.so"))
    L.vtxt_inflate.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
    L.vtxt_inflate.restype = C.c_uint32
    for i, (c, r) in enumerate(zip(U.corpus(), plain[0x00])):
        n = c.out_len
        out = (C.c_uint8 * (n + 64))()
        C.memset(C.addressof(out), 0xCD, n + 64)
        trips = C.c_uint32(0)
        st = L.vtxt_inflate(c.raw, len(c.raw), C.addressof(out), n, 1 + i % 3 * 31, C.addressof(trips))
        assert (st, trips.value) == (r.status, r.trips), c.name
        assert bytes(out[n:n + 64]) == b"\xcd" * 64, c.name
        if st == U.ST_OK:
            assert bytes(out[:n]) == r.out, c.name
