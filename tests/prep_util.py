"""ctypes access to tests/prepcore/ (the host build of vartrix_amd/csrc/vtx_prep_core.h) for tests/test_prep_core.py and
tests/test_gpu_prep_cases.py: the CPU harness runs the whole raw-batch preparation from the functions the kernels are compiled from."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from vartrix_amd.abi import RECORD_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "prepcore")
MAX_READ_LEN = 30000                     # kMaxReadLen of vtx_api.hip
MUTANTS = tuple(range(1, 11))
NO_CELL = 0xFFFFFFFF


def load(mutant=0):
    name = "libprep_host_mut%d.so" % mutant if mutant else "libprep_host.so"
    subprocess.check_call(["make", "-C", DIR, "-s", name])
    L = C.CDLL(os.path.join(DIR, name))
    L.vtxt_prep_mutant.restype = C.c_int
    assert L.vtxt_prep_mutant() == mutant
    L.vtxt_hash_bytes.restype = C.c_uint64
    L.vtxt_hash_bytes.argtypes = [C.c_char_p, C.c_uint32, C.c_uint64]
    L.vtxt_bytes_equal.restype = C.c_int
    L.vtxt_bytes_equal.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32]
    L.vtxt_next_seed.restype = C.c_uint64
    L.vtxt_next_seed.argtypes = [C.c_uint64]
    L.vtxt_key_widths.restype = None
    L.vtxt_key_widths.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
    L.vtxt_table.restype = C.c_uint32
    L.vtxt_table.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.vtxt_table_probe.restype = C.c_uint32
    L.vtxt_table_probe.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint32]
    L.vtxt_prep_run.restype = C.c_int
    L.vtxt_prep_run.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int,
                                C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vtxt_prep_check.restype = C.c_uint64
    L.vtxt_prep_check.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_int]
    return L


def barcode_arrays(barcodes):
    off = np.zeros(len(barcodes) + 1, np.uint64)
    if barcodes:
        np.cumsum([len(b) for b in barcodes], out=off[1:])
    data = np.frombuffer(b"".join(barcodes) + b"\x00", np.uint8).copy()     # (one spare byte: an empty list still has an address)
    return off, data


def table_slots(L, barcodes):
    off, data = barcode_arrays(barcodes)
    slots = np.zeros(L.vtxt_table(None, off.ctypes.data, len(barcodes), None), np.uint32)
    L.vtxt_table(data.ctypes.data, off.ctypes.data, len(barcodes), slots.ctypes.data)
    return [int(s) for s in slots]


def prepare(L, raw, barcodes, use_umi, weak_rounds=0, nibbles=False):
    """-> (status, stats dict, records, rec_begin, rec_count) of the CPU harness"""
    off, data = barcode_arrays(barcodes)
    recs = np.zeros(max(raw.n_records, 1), RECORD_DTYPE)
    begin, count = np.zeros(max(raw.n_loci, 1), np.uint32), np.zeros(max(raw.n_loci, 1), np.uint32)
    stats = np.zeros(8, np.uint64)
    tags = raw.tag_arena if raw.tag_arena.size else np.zeros(1, np.uint8)
    rc = L.vtxt_prep_run(raw.loci.ctypes.data, raw.n_loci, raw.records.ctypes.data, raw.n_records, tags.ctypes.data, int(raw.tag_arena.size),
                         int(raw.read_arena.size), MAX_READ_LEN, int(nibbles), data.ctypes.data, off.ctypes.data, len(barcodes), int(use_umi),
                         weak_rounds, recs.ctypes.data, begin.ctypes.data, count.ctypes.data, stats.ctypes.data)
    st = dict(zip(("num_not_cell_bc", "num_non_umi", "kept", "hash_rounds", "cell_bits", "end_bit", "table_slots"), (int(x) for x in stats)))
    return rc, st, recs[:st["kept"]] if rc == 0 else recs[:0], begin[:raw.n_loci], count[:raw.n_loci]


def check_word(L, batch, n_barcodes, use_umi, nibbles=False):
    """prep_check_kernel's verdict on a packed batch from the core: None, or (record, code)"""
    w = L.vtxt_prep_check(batch.loci.ctypes.data, batch.n_loci, batch.records.ctypes.data, batch.n_records, int(batch.read_arena.size) * (2 if nibbles else 1),
                          MAX_READ_LEN, int(nibbles), n_barcodes, int(use_umi))
    return None if w == (1 << 64) - 1 else (w >> 3, w & 7)


def program_input(items):
    """items: [(raw, barcodes, use_umi, weak_rounds)] -> the bytes tests/prepcore/main.cpp reads"""
    out = [struct.pack("<I", len(items))]
    for raw, barcodes, use_umi, weak in items:
        off, _ = barcode_arrays(barcodes)
        bc = b"".join(barcodes)
        out.append(struct.pack("<10I", raw.n_loci, raw.n_records, raw.tag_arena.size, raw.read_arena.size, MAX_READ_LEN, 0, len(barcodes), len(bc),
                               int(use_umi), weak))
        out += [raw.loci.tobytes(), raw.records.tobytes(), raw.tag_arena.tobytes(), off.tobytes(), bc]
    return b"".join(out)


def program_output(data, items):
    """-> [(status, stats dict, records, rec_begin, rec_count)]"""
    res, p = [], 0
    for raw, _, _, _ in items:
        status, kept, rounds, _, not_bc, non_umi = struct.unpack_from("<iIIIQQ", data, p)
        p += 32
        st = {"num_not_cell_bc": not_bc, "num_non_umi": non_umi, "kept": kept, "hash_rounds": rounds}
        recs, begin, count = np.zeros(0, RECORD_DTYPE), np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        if status == 0:
            recs = np.frombuffer(data, RECORD_DTYPE, kept, p)
            p += 16 * kept
            begin = np.frombuffer(data, np.uint32, raw.n_loci, p)
            p += 4 * raw.n_loci
            count = np.frombuffer(data, np.uint32, raw.n_loci, p)
            p += 4 * raw.n_loci
        res.append((status, st, recs, begin, count))
    assert p == len(data)
    return res


def run_program(items, tmp, san):
    name = "prep_host_san" if san else "prep_host"
    subprocess.check_call(["make", "-C", DIR, "-s", name])
    src, dst = os.path.join(tmp, name + ".in"), os.path.join(tmp, name + ".out")
    with open(src, "wb") as f:
        f.write(program_input(items))
    r = subprocess.run([os.path.join(DIR, name), src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, "exit %d\n%s" % (r.returncode, r.stderr[-4000:])
    with open(dst, "rb") as f:
        return program_output(f.read(), items)
