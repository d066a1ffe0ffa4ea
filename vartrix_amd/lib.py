"""ctypes binding of libvtx.so — the host side of the C-ABI in ``include/vtx.h``.

There is no fallback: if the shared library is missing or no gfx950 device is
present, the calls raise.  The method names follow the C entry points, which in
turn name the reference seam they replace (``evaluate_chunk`` +
the merge loop, reference ``src/main.rs:596-607`` / ``:320-348``).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# Build variants of the SAME sources (vartrix_amd/csrc/Makefile), never loaded in production:
#   dev    -DVTX_DEVTOOLS: the experiment / test hooks (stage switches, ablations, buffer caps, the socket transport standing in for
#          RCCL) exist only there; the production libvtx.so reads VTX_DEBUG and nothing else
#   lazy0, lazy40, anchor5, noseed0   one recollected detail of the crate's band switched (tests/test_gpu_variants.py)
#   (the compile-time A/B builds nw3 and not3 are gone, last in commit 5c0dd06: mask words and t3[] are picked at run time)
# VTX_LIB_VARIANT=<name> makes a variant the process default; load(variant) / Context(cfg, variant=...) pick one explicitly.
DEFAULT_VARIANT = os.environ.get("VTX_LIB_VARIANT", "")


def lib_path(variant=None) -> str:
    v = DEFAULT_VARIANT if variant is None else variant
    return os.path.join(_HERE, "libvtx%s.so" % ("_" + v if v else ""))


LIB_PATH = lib_path()

SYMBOLS = (
    "vtx_config_default", "vtx_create", "vtx_destroy", "vtx_submit", "vtx_run", "vtx_fetch_scores",
    "vtx_fetch_coo", "vtx_device_scores", "vtx_device_coo", "vtx_last_timing", "vtx_last_cells", "vtx_strerror",
    "vtx_status_name", "vtx_abi_sizes", "vtx_set_barcodes", "vtx_submit_raw", "vtx_fetch_records",
    "vtx_comm_id", "vtx_comm_init", "vtx_gather_coo", "vtx_fetch_gathered", "vtx_gather_abort", "vtx_gather_plan",
    "vtx_set_debug", "vtx_fetch_stage", "vtx_debug_bands", "vtx_debug_tables", "vtx_set_read_format",
    "vtx_submit_bam", "vtx_submit_bam_segments", "vtx_debug_ingest", "vtx_debug_inflate", "vtx_comm_ranks", "vtx_write_mtx", "vtx_prefetch_file",
    "vtx_last_crc_ms", "vtx_write_mtx_gz", "vtx_mtx_part", "vtx_mtx_part_free", "vtx_mtx_join",
    "vtx_device_csr", "vtx_csr_transpose", "vtx_last_csr_ms",
    "vtx_csr_row_stats", "vtx_csr_select_plan", "vtx_csr_select", "vtx_sizeof_csr_stats",
    "vtx_csr_group_window", "vtx_csr_group_max", "vtx_csr_group_plan", "vtx_csr_group_sum",
    "vtx_csr_geno_max", "vtx_sizeof_geno_tally", "vtx_csr_geno_tally",
    "vtx_csr_geno_pair_max", "vtx_sizeof_geno_pair_tally", "vtx_csr_geno_pair_tally",
    "vtx_csr_dense_max", "vtx_csr_dense_sum",
)
# (entry points with a digit in their name: tests/test_abi.py finds the header's declarations with [a-z_]+ and compares them with SYMBOLS,
# so these are listed — and checked against the header and every build of the library, tests/test_abi_f64.py — on their own)
SYMBOLS_ALNUM = ("vtx_write_mtx_f64", "vtx_debug_crc32")


class VtxError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__("%s: %s" % (status_name(status), message))
        self.status = status


_libs = {}


def load(variant=None):
    """dlopen libvtx.so (built in-tree by ``__graft_entry__.build()``); raises if absent."""
    path = lib_path(variant)
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise ImportError("%s not built — run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(make -C vartrix_amd/csrc). There is no CPU fallback." % path)
    L = C.CDLL(path)
    ctxp = C.c_void_p
    L.vtx_config_default.restype = None
    L.vtx_config_default.argtypes = [C.POINTER(abi.VtxConfig)]
    L.vtx_create.restype = C.c_int
    L.vtx_create.argtypes = [C.POINTER(abi.VtxConfig), C.POINTER(ctxp)]
    L.vtx_destroy.restype = None
    L.vtx_destroy.argtypes = [ctxp]
    L.vtx_submit.restype = C.c_int
    L.vtx_submit.argtypes = [ctxp, C.POINTER(abi.VtxBatch)]
    L.vtx_run.restype = C.c_int
    L.vtx_run.argtypes = [ctxp]
    L.vtx_set_barcodes.restype = C.c_int
    L.vtx_set_barcodes.argtypes = [ctxp, C.c_void_p, C.c_void_p, C.c_uint32]
    L.vtx_submit_raw.restype = C.c_int
    L.vtx_submit_raw.argtypes = [ctxp, C.POINTER(abi.VtxRawBatch), C.POINTER(abi.VtxRawStats)]
    L.vtx_fetch_records.restype = C.c_int
    L.vtx_fetch_records.argtypes = [ctxp, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vtx_fetch_scores.restype = C.c_int
    L.vtx_fetch_scores.argtypes = [ctxp, C.c_void_p, C.c_void_p]
    L.vtx_fetch_coo.restype = C.c_int
    L.vtx_fetch_coo.argtypes = [ctxp, C.POINTER(abi.VtxCoo)]
    L.vtx_device_scores.restype = C.c_int
    L.vtx_device_scores.argtypes = [ctxp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.vtx_device_coo.restype = C.c_int
    L.vtx_device_coo.argtypes = [ctxp, C.POINTER(abi.VtxCoo)]
    L.vtx_device_csr.restype = C.c_int
    L.vtx_device_csr.argtypes = [ctxp, C.c_uint32, C.c_uint32, C.POINTER(abi.VtxCsr)]
    L.vtx_csr_transpose.restype = C.c_int
    L.vtx_csr_transpose.argtypes = [ctxp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_uint32]
    csr_in = [ctxp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]       # ctx, n_major, n_minor, nnz, d_indptr, d_indices
    L.vtx_csr_row_stats.restype = C.c_int
    L.vtx_csr_row_stats.argtypes = csr_in + [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(abi.VtxCsrStats)]
    L.vtx_csr_select_plan.restype = C.c_int
    L.vtx_csr_select_plan.argtypes = csr_in + [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.vtx_csr_select.restype = C.c_int
    L.vtx_csr_select.argtypes = csr_in + [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_uint32]
    L.vtx_csr_group_window.restype = C.c_uint32
    L.vtx_csr_group_window.argtypes = []
    L.vtx_csr_group_max.restype = C.c_uint32
    L.vtx_csr_group_max.argtypes = []
    L.vtx_csr_group_plan.restype = C.c_int
    L.vtx_csr_group_plan.argtypes = csr_in + [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
    L.vtx_csr_group_sum.restype = C.c_int
    L.vtx_csr_group_sum.argtypes = csr_in + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p,
                                             C.POINTER(abi.VtxCsrStats)]
    L.vtx_csr_geno_max.restype = C.c_uint32
    L.vtx_csr_geno_max.argtypes = []
    L.vtx_sizeof_geno_tally.restype = C.c_uint32
    L.vtx_sizeof_geno_tally.argtypes = []
    L.vtx_csr_geno_tally.restype = C.c_int
    L.vtx_csr_geno_tally.argtypes = csr_in + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(abi.VtxGenoTally)]
    L.vtx_csr_geno_pair_max.restype = C.c_uint32
    L.vtx_csr_geno_pair_max.argtypes = []
    L.vtx_sizeof_geno_pair_tally.restype = C.c_uint32
    L.vtx_sizeof_geno_pair_tally.argtypes = []
    L.vtx_csr_geno_pair_tally.restype = C.c_int
    L.vtx_csr_geno_pair_tally.argtypes = csr_in + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(abi.VtxGenoPairTally)]
    L.vtx_csr_dense_max.restype = C.c_uint32
    L.vtx_csr_dense_max.argtypes = []
    L.vtx_csr_dense_sum.restype = C.c_int
    L.vtx_csr_dense_sum.argtypes = csr_in + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.vtx_sizeof_csr_stats.restype = C.c_uint32
    L.vtx_sizeof_csr_stats.argtypes = []
    L.vtx_last_csr_ms.restype = C.c_int
    L.vtx_last_csr_ms.argtypes = [ctxp, C.POINTER(C.c_float), C.c_uint32]
    L.vtx_last_timing.restype = C.c_int
    L.vtx_last_timing.argtypes = [ctxp, C.POINTER(abi.VtxTiming)]
    L.vtx_last_cells.restype = C.c_int
    L.vtx_last_cells.argtypes = [ctxp, C.POINTER(C.c_uint64)]
    L.vtx_strerror.restype = C.c_char_p
    L.vtx_strerror.argtypes = [ctxp]
    L.vtx_status_name.restype = C.c_char_p
    L.vtx_status_name.argtypes = [C.c_int]
    L.vtx_abi_sizes.restype = C.c_int
    L.vtx_abi_sizes.argtypes = [C.POINTER(C.c_uint32), C.c_uint32]
    L.vtx_comm_id.restype = C.c_int
    L.vtx_comm_id.argtypes = [C.c_void_p]
    L.vtx_comm_init.restype = C.c_int
    L.vtx_comm_init.argtypes = [ctxp, C.c_void_p, C.c_int, C.c_int]
    L.vtx_gather_coo.restype = C.c_int
    L.vtx_gather_coo.argtypes = [ctxp, C.c_int, C.POINTER(abi.VtxCoo)]
    L.vtx_fetch_gathered.restype = C.c_int
    L.vtx_fetch_gathered.argtypes = [ctxp, C.POINTER(abi.VtxCoo)]
    L.vtx_gather_abort.restype = C.c_int
    L.vtx_gather_abort.argtypes = [ctxp]
    L.vtx_gather_plan.restype = C.c_int
    L.vtx_gather_plan.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.vtx_set_debug.restype = C.c_int
    L.vtx_set_debug.argtypes = [ctxp, C.c_int, C.c_int64]
    L.vtx_fetch_stage.restype = C.c_int
    L.vtx_fetch_stage.argtypes = [ctxp, C.c_void_p]
    L.vtx_set_read_format.restype = C.c_int
    L.vtx_set_read_format.argtypes = [ctxp, C.c_int]
    L.vtx_debug_tables.restype = C.c_int
    L.vtx_debug_tables.argtypes = [ctxp, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.vtx_debug_bands.restype = C.c_int
    L.vtx_debug_bands.argtypes = [ctxp, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vtx_submit_bam.restype = C.c_int
    L.vtx_submit_bam.argtypes = [ctxp, C.POINTER(abi.VtxBamIngest), C.POINTER(abi.VtxIngestStats)]
    L.vtx_submit_bam_segments.restype = C.c_int
    L.vtx_submit_bam_segments.argtypes = [ctxp, C.POINTER(abi.VtxBamSegments), C.POINTER(abi.VtxIngestStats)]
    L.vtx_prefetch_file.restype = C.c_int
    L.vtx_prefetch_file.argtypes = [ctxp, C.c_char_p, C.c_uint64, C.c_uint64]
    L.vtx_write_mtx.restype = C.c_int
    L.vtx_write_mtx.argtypes = [ctxp, C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_double)]
    L.vtx_write_mtx_f64.restype = C.c_int
    L.vtx_write_mtx_f64.argtypes = [ctxp, C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_double)]
    L.vtx_write_mtx_gz.restype = C.c_int
    L.vtx_write_mtx_gz.argtypes = [ctxp, C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.vtx_mtx_part.restype = C.c_int
    L.vtx_mtx_part.argtypes = [ctxp, C.c_int, C.c_int, C.c_int, C.POINTER(abi.VtxMtxPart)]
    L.vtx_mtx_part_free.restype = None
    L.vtx_mtx_part_free.argtypes = [C.POINTER(abi.VtxMtxPart)]
    L.vtx_mtx_join.restype = C.c_int
    L.vtx_mtx_join.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(abi.VtxMtxPart), C.c_uint32, C.POINTER(C.c_uint64)]
    L.vtx_comm_ranks.restype = C.c_int
    L.vtx_comm_ranks.argtypes = [ctxp, C.POINTER(C.c_int)]
    L.vtx_debug_inflate.restype = C.c_int
    L.vtx_debug_inflate.argtypes = [ctxp, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    L.vtx_debug_ingest.restype = C.c_int
    L.vtx_debug_ingest.argtypes = [ctxp, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.vtx_debug_crc32.restype = C.c_int
    L.vtx_debug_crc32.argtypes = [ctxp, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]
    L.vtx_last_crc_ms.restype = C.c_int
    L.vtx_last_crc_ms.argtypes = [ctxp, C.POINTER(C.c_float)]
    _libs[path] = L
    return L


def status_name(status: int) -> str:
    return load().vtx_status_name(status).decode()


COMM_ID_BYTES = 128


def gather_plan(counts):
    """(status, offsets, total) of vtx_gather_plan: where every rank's triplets land in the gathered arrays (pure; no GPU)."""
    L = load()
    n = len(counts)
    c = (C.c_uint64 * n)(*[int(v) for v in counts])
    off = (C.c_uint64 * n)()
    tot = C.c_uint64(0)
    rc = L.vtx_gather_plan(n, c, off, C.byref(tot))
    return rc, list(off), int(tot.value)


def comm_id() -> bytes:
    """RCCL unique id (rank 0 creates it; the host hands the 128 bytes to the other ranks)."""
    L = load()
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = L.vtx_comm_id(buf)
    if rc != abi.VTX_OK:
        raise VtxError(rc, L.vtx_strerror(None).decode())
    return buf.raw


def mtx_join(path: str, n_rows: int, n_cols: int, parts, gz: bool = False, variant=None) -> int:
    """vtx_mtx_join: ``path`` = the three Matrix-Market header lines (nnz = the parts' total), then the parts (``abi.MtxPart``, from
    ``Context.mtx_part`` or ``hostlib.mtx_part``) in order; with ``gz`` a BGZF file (the header a member of its own, the empty member at
    the end).  Needs no GPU.  Returns the uncompressed size of the file."""
    L = load(variant)
    arr = (abi.VtxMtxPart * max(len(parts), 1))()
    keep = []
    for i, p in enumerate(parts):
        buf = C.create_string_buffer(p.bytes, len(p.bytes)) if p.bytes else None
        keep.append(buf)
        arr[i] = abi.VtxMtxPart(C.cast(buf, C.c_void_p) if buf is not None else None, len(p.bytes), p.text_bytes, p.nnz, p.sum, int(p.gz), 0)
    t = C.c_uint64(0)
    rc = L.vtx_mtx_join(path.encode(), n_rows, n_cols, int(bool(gz)), arr if parts else None, len(parts), C.byref(t))
    if rc != abi.VTX_OK:
        raise VtxError(rc, L.vtx_strerror(None).decode())
    return int(t.value)


def _out_struct(cls, out: dict, names, who: str, what: str):
    """A struct of output pointers from a dict name -> device address; a name that is missing or 0 stays NULL, a name the struct does
    not have is a ValueError."""
    unknown = set(out) - set(names)
    if unknown:
        raise ValueError("%s: unknown %s %s" % (who, what, sorted(unknown)))
    st = cls()
    for k, typ in st._fields_:
        setattr(st, k, C.cast(C.c_void_p(int(out.get(k) or 0) or None), typ))
    return st


def _payload_arrays(payloads):
    """(address in, address out, element bytes) per array that moves with the entries -> the three C arrays and their length."""
    n = len(payloads)
    p_in = (C.c_void_p * max(n, 1))(*[int(p[0]) or None for p in payloads])
    p_out = (C.c_void_p * max(n, 1))(*[int(p[1]) or None for p in payloads])
    p_sz = (C.c_uint32 * max(n, 1))(*[int(p[2]) for p in payloads])
    return p_in, p_out, p_sz, n


class Context:
    """One vtx_ctx: bound to one GPU, holds one resident batch."""

    def __init__(self, cfg: abi.VtxConfig, variant=None):
        self._L = load(variant)
        self._h = C.c_void_p()
        self.cfg = cfg
        rc = self._L.vtx_create(C.byref(cfg), C.byref(self._h))
        if rc != abi.VTX_OK:
            raise VtxError(rc, self._L.vtx_strerror(None).decode())
        self.n_records = 0

    def _check(self, rc: int):
        if rc != abi.VTX_OK:
            raise VtxError(rc, self._L.vtx_strerror(self._h).decode())

    def close(self):
        if self._h:
            self._L.vtx_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_read_format(self, fmt: int):
        self._check(self._L.vtx_set_read_format(self._h, int(fmt)))

    def submit(self, batch: abi.PackedBatch):
        self.set_read_format(getattr(batch, "read_format", 0))
        st = batch.as_struct()
        self._check(self._L.vtx_submit(self._h, C.byref(st)))
        self.n_records = batch.n_records
        self._n_loci = batch.n_loci

    def set_barcodes(self, barcodes):
        """Barcode list (bytes objects, index = matrix column) for ``submit_raw``; load_barcodes, src/main.rs:697-718."""
        blobs = [b if isinstance(b, bytes) else b.encode() for b in barcodes]
        offsets = np.zeros(len(blobs) + 1, np.uint64)
        np.cumsum([len(b) for b in blobs], out=offsets[1:])
        data = np.frombuffer(b"".join(blobs), np.uint8) if blobs else np.zeros(0, np.uint8)
        data = np.ascontiguousarray(data)
        self._check(self._L.vtx_set_barcodes(self._h, data.ctypes.data if data.size else None, offsets.ctypes.data, len(blobs)))

    def submit_raw(self, raw: abi.RawBatch) -> abi.VtxRawStats:
        self.set_read_format(getattr(raw, "read_format", 0))
        st = raw.as_struct()
        stats = abi.VtxRawStats()
        self._check(self._L.vtx_submit_raw(self._h, C.byref(st), C.byref(stats)))
        self.n_records = int(stats.kept)
        self._n_loci = raw.n_loci
        return stats

    def prefetch_file(self, path: str, file_off: int = 0, n: int = 0):
        """Start uploading bytes [file_off, file_off + n) of the file (n = 0: to its end) for a later submit_bam."""
        self._check(self._L.vtx_prefetch_file(self._h, path.encode(), file_off, n))

    def submit_bam(self, ingest: abi.VtxBamIngest, n_loci: int) -> abi.VtxIngestStats:
        """Device-side ingest of a BAM range (vtx_submit_bam): ``ingest`` comes from ``hostlib.plan_ingest`` (or is built by hand in the
        tests); the barcode list must be set.  Afterwards the context is in the state ``submit_raw`` leaves."""
        stats = abi.VtxIngestStats()
        self._check(self._L.vtx_submit_bam(self._h, C.byref(ingest), C.byref(stats)))
        self.n_records = int(stats.raw.kept)
        self._n_loci = n_loci
        return stats

    def submit_bam_segments(self, plan: abi.VtxBamSegments, n_loci: int) -> abi.VtxIngestStats:
        """Device-side ingest of a SEGMENTED plan (vtx_submit_bam_segments; sparse loci: ``hostlib.plan_ingest(..).segments``): only the
        segments' bytes travel, record chains end where their segment ends.  The same state afterwards as ``submit_bam``."""
        stats = abi.VtxIngestStats()
        self._check(self._L.vtx_submit_bam_segments(self._h, C.byref(plan), C.byref(stats)))
        self.n_records = int(stats.raw.kept)
        self._n_loci = n_loci
        return stats

    def debug_inflate(self, data: bytes, blocks):
        """bgzf_inflate_kernel on raw-DEFLATE payloads: blocks = [(offset, clen, isize)] into ``data``.  -> (status array, [bytes per block])"""
        blk = np.array(blocks, dtype=abi.BGZF_BLOCK_DTYPE) if len(blocks) else np.zeros(0, abi.BGZF_BLOCK_DTYPE)
        total = int(blk["isize"].sum())
        out = np.zeros(total + 64, np.uint8)
        status = np.zeros(max(len(blk), 1), np.uint32)
        self._check(self._L.vtx_debug_inflate(self._h, data, len(data), blk.ctypes.data if len(blk) else None, len(blk),
                                              out.ctypes.data, total, status.ctypes.data))
        offs = np.concatenate([[0], np.cumsum(blk["isize"])]).astype(np.int64)
        return status[:len(blk)], [bytes(out[offs[i]:offs[i + 1]]) for i in range(len(blk))]

    def debug_crc32(self, data: bytes, offsets) -> np.ndarray:
        """bgzf_crc32_kernel on byte ranges of ``data``: range i = data[offsets[i]:offsets[i + 1]] (ascending, each at most 64 KiB).
        -> uint32 array of their CRC-32s (zlib.crc32's values)."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(off) - 1
        buf = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
        out = np.zeros(max(n, 1), np.uint32)
        self._check(self._L.vtx_debug_crc32(self._h, buf.ctypes.data, len(data), off.ctypes.data, n, out.ctypes.data))
        return out[:n]

    def crc_ms(self) -> float:
        """Device time of the last CRC32 check (submit_bam / submit_bam_segments / debug_crc32), milliseconds."""
        ms = C.c_float(0)
        self._check(self._L.vtx_last_crc_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def debug_ingest(self, what: int, dtype=np.uint8) -> np.ndarray:
        """An intermediate array of the last submit_bam (abi.INGEST_*)."""
        n = C.c_uint64(0)
        self._check(self._L.vtx_debug_ingest(self._h, what, None, 0, C.byref(n)))
        out = np.zeros(int(n.value), np.uint8)
        if n.value:
            self._check(self._L.vtx_debug_ingest(self._h, what, out.ctypes.data, n.value, C.byref(n)))
        return out.view(dtype)

    def fetch_records(self):
        """Resolved, sorted records of the resident batch + per-locus (rec_begin, rec_count)."""
        recs = np.zeros(self.n_records, abi.RECORD_DTYPE)
        nl = getattr(self, "_n_loci", 0)
        begin = np.zeros(nl, np.uint32)
        count = np.zeros(nl, np.uint32)
        self._check(self._L.vtx_fetch_records(self._h, recs.ctypes.data, begin.ctypes.data, count.ctypes.data))
        return recs, begin, count

    def run(self):
        self._check(self._L.vtx_run(self._h))

    def fetch_scores(self):
        ref = np.zeros(self.n_records, np.int32)
        alt = np.zeros(self.n_records, np.int32)
        self._check(self._L.vtx_fetch_scores(self._h, ref.ctypes.data, alt.ctypes.data))
        return ref, alt

    def fetch_coo(self) -> dict:
        coo = abi.VtxCoo()
        self._check(self._L.vtx_fetch_coo(self._h, C.byref(coo)))
        n = int(coo.nnz)
        out = {}
        for k, dt in (("row", np.uint32), ("col", np.uint32), ("alt", np.uint32), ("ref", np.uint32),
                      ("unk", np.uint32), ("value", np.float64), ("ref_value", np.float64)):
            out[k] = np.ctypeslib.as_array(getattr(coo, k), shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dt)
        return out

    def device_scores(self):
        r, a = C.c_void_p(), C.c_void_p()
        self._check(self._L.vtx_device_scores(self._h, C.byref(r), C.byref(a)))
        return r.value, a.value

    def device_coo(self) -> dict:
        """Raw device addresses of the triplet arrays + nnz (for torch/RCCL interop)."""
        coo = abi.VtxCoo()
        self._check(self._L.vtx_device_coo(self._h, C.byref(coo)))
        out = {"nnz": int(coo.nnz)}
        for k in ("row", "col", "alt", "ref", "unk", "value", "ref_value"):
            out[k] = C.cast(getattr(coo, k), C.c_void_p).value or 0
        return out

    def device_csr(self, row_begin: int, row_end: int) -> dict:
        """Raw device addresses of the last run's variant-major CSR over the rows [row_begin, row_end) (vtx_device_csr): ``indptr``
        (row_end - row_begin + 1 uint64), ``indices`` (the address ``device_coo()["col"]`` reports), the five data arrays, plus nnz,
        row_begin, row_end, n_cols.  VTX_E_INVAL when a triplet's row lies outside the window."""
        st = abi.VtxCsr()
        self._check(self._L.vtx_device_csr(self._h, int(row_begin), int(row_end), C.byref(st)))
        out = {"nnz": int(st.nnz), "row_begin": int(st.row_begin), "row_end": int(st.row_end), "n_cols": int(st.n_cols)}
        for k in ("indptr", "indices", "alt", "ref", "unk", "value", "ref_value"):
            out[k] = C.cast(getattr(st, k), C.c_void_p).value or 0
        return out

    def csr_transpose(self, n_major: int, n_minor: int, nnz: int, indptr: int, indices: int, indptr_t: int, indices_t: int, perm: int = 0,
                      payloads=()):
        """Stable transpose of a CSR in device memory (vtx_csr_transpose); every array is a raw device ADDRESS.  ``payloads``: a list
        of (address in, address out, element bytes 4 | 8) that move with the entries.  ``perm`` = 0: not wanted."""
        p_in, p_out, p_sz, n = _payload_arrays(payloads)
        self._check(self._L.vtx_csr_transpose(self._h, int(n_major), int(n_minor), int(nnz), indptr or None, indices or None, indptr_t or None,
                                              indices_t or None, perm or None, p_in, p_out, p_sz, n))

    def csr_ms(self) -> dict:
        """Device time of the last CSR call by phase, milliseconds (vtx_last_csr_ms: events on the context's stream).  ``sort`` is the
        scans of a selection, ``place`` the reduction of ``csr_row_stats``."""
        ms = (C.c_float * 4)()
        self._check(self._L.vtx_last_csr_ms(self._h, ms, 4))
        return dict(zip(("check", "sort", "offsets", "place"), (float(v) for v in ms)))

    def csr_row_stats(self, n_major: int, n_minor: int, nnz: int, indptr: int, indices: int, alt: int, ref: int, unk: int, out: dict):
        """The statistics of every row of a CSR in device memory (vtx_csr_row_stats); every array is a raw device ADDRESS.  ``out``:
        name (``abi.CSR_STAT_NAMES``) -> address of n_major uint32 (the four counts) / uint64 (the three sums); a name that is missing
        or 0 is not computed into memory."""
        st = _out_struct(abi.VtxCsrStats, out, abi.CSR_STAT_NAMES, "csr_row_stats", "statistics")
        self._check(self._L.vtx_csr_row_stats(self._h, int(n_major), int(n_minor), int(nnz), indptr or None, indices or None, alt or None,
                                              ref or None, unk or None, C.byref(st)))

    def csr_select_plan(self, n_major: int, n_minor: int, nnz: int, indptr: int, indices: int, keep_major: int = 0, keep_minor: int = 0):
        """The sizes (n_major_out, n_minor_out, nnz_out) of the selection of a CSR in device memory by byte masks (vtx_csr_select_plan);
        a mask address of 0 keeps everything."""
        a, b, n = C.c_uint32(), C.c_uint32(), C.c_uint64()
        self._check(self._L.vtx_csr_select_plan(self._h, int(n_major), int(n_minor), int(nnz), indptr or None, indices or None, keep_major or None,
                                                keep_minor or None, C.byref(a), C.byref(b), C.byref(n)))
        return int(a.value), int(b.value), int(n.value)

    def csr_select(self, n_major: int, n_minor: int, nnz: int, indptr: int, indices: int, keep_major: int, keep_minor: int, sizes, indptr_out: int,
                   indices_out: int, major_ids: int = 0, minor_ids: int = 0, payloads=()):
        """Stable selection of rows and columns of a CSR in device memory (vtx_csr_select).  ``sizes``: what ``csr_select_plan`` returned
        for the same inputs, the sizes the outputs were allocated for — any other selection is refused with nothing written.
        ``payloads``: (address in, address out, element bytes 4 | 8) per array that moves with the entries."""
        p_in, p_out, p_sz, n = _payload_arrays(payloads)
        self._check(self._L.vtx_csr_select(self._h, int(n_major), int(n_minor), int(nnz), indptr or None, indices or None, keep_major or None,
                                           keep_minor or None, int(sizes[0]), int(sizes[1]), int(sizes[2]), indptr_out or None, indices_out or None,
                                           major_ids or None, minor_ids or None, p_in, p_out, p_sz, n))

    def csr_group_plan(self, n_major: int, n_minor: int, nnz: int, indptr: int, indices: int, group: int, n_groups: int) -> int:
        """nnz_out of the CSR in device memory summed per group of columns (vtx_csr_group_plan): the number of (row, group) pairs with at
        least one entry.  ``group``: the address of n_minor uint32 labels, each below ``n_groups`` or ``abi.VTX_GROUP_NONE``."""
        n = C.c_uint64()
        self._check(self._L.vtx_csr_group_plan(self._h, int(n_major), int(n_minor), int(nnz), indptr or None, indices or None, group or None,
                                               int(n_groups), C.byref(n)))
        return int(n.value)

    def csr_group_sum(self, n_major: int, n_minor: int, nnz: int, indptr: int, indices: int, alt: int, ref: int, unk: int, group: int,
                      n_groups: int, nnz_out: int, indptr_out: int, indices_out: int, out: dict):
        """The CSR in device memory summed per group of columns (vtx_csr_group_sum) into a CSR of n_major x n_groups.  ``nnz_out``: what
        ``csr_group_plan`` returned for the same inputs, the size the outputs were allocated for — any other fold is refused with
        nothing written.  ``out``: name (``abi.CSR_STAT_NAMES``) -> address of nnz_out uint32 (the four counts) / uint64 (the three
        sums); a name that is missing or 0 is not written."""
        st = _out_struct(abi.VtxCsrStats, out, abi.CSR_STAT_NAMES, "csr_group_sum", "statistics")
        self._check(self._L.vtx_csr_group_sum(self._h, int(n_major), int(n_minor), int(nnz), indptr or None, indices or None, alt or None,
                                              ref or None, unk or None, group or None, int(n_groups), int(nnz_out), indptr_out or None,
                                              indices_out or None, C.byref(st)))

    def csr_geno_tally(self, n_major: int, n_minor: int, nnz: int, indptr: int, indices: int, alt: int, ref: int, geno: int, n_donors: int,
                       out: dict):
        """Every row of a CSR in device memory (rows = cells, indices = variants) tallied against the genotypes of ``n_donors`` donors
        (vtx_csr_geno_tally).  ``geno``: the address of n_minor * n_donors bytes, variant-major, each 0, 1, 2 or ``abi.VTX_GENO_NONE``.
        ``out``: name (``abi.GENO_TALLY_NAMES``) -> address of n_major * n_donors * 4 uint64 (``sum_alt``, ``sum_ref``) / uint32
        (``n_obs``); a name that is missing or 0 is not written."""
        st = _out_struct(abi.VtxGenoTally, out, abi.GENO_TALLY_NAMES, "csr_geno_tally", "outputs")
        self._check(self._L.vtx_csr_geno_tally(self._h, int(n_major), int(n_minor), int(nnz), indptr or None, indices or None, alt or None,
                                               ref or None, geno or None, int(n_donors), C.byref(st)))

    def csr_geno_pair_tally(self, n_major: int, n_minor: int, nnz: int, indptr: int, indices: int, alt: int, ref: int, geno: int, n_donors: int,
                            pairs: int, n_pairs: int, out: dict):
        """Every row of a CSR in device memory (rows = cells, indices = variants) tallied against ``n_pairs`` pairs of donors
        (vtx_csr_geno_pair_tally).  ``geno``: as for ``csr_geno_tally``.  ``pairs``: the address of 2 * n_pairs uint32 in device memory,
        the donors (a, b) of pair p at [2 p], [2 p + 1], both below ``n_donors``.  ``out``: name (``abi.GENO_TALLY_NAMES``) -> address of
        n_major * n_pairs * 6 uint64 (``sum_alt``, ``sum_ref``) / uint32 (``n_obs``), by the dosage g_a + g_b (5: either donor without a
        call); a name that is missing or 0 is not written."""
        st = _out_struct(abi.VtxGenoPairTally, out, abi.GENO_TALLY_NAMES, "csr_geno_pair_tally", "outputs")
        self._check(self._L.vtx_csr_geno_pair_tally(self._h, int(n_major), int(n_minor), int(nnz), indptr or None, indices or None, alt or None,
                                                    ref or None, geno or None, int(n_donors), pairs or None, int(n_pairs), C.byref(st)))

    def csr_dense_sum(self, n_major: int, n_minor: int, nnz: int, indptr: int, indices: int, alt: int, ref: int, w_alt: int, w_ref: int,
                      n_cols: int, out: int):
        """Every row of a CSR in device memory times one or two tables of int32 weights (vtx_csr_dense_sum): ``out[r * n_cols + h]`` =
        the sum over the row's entries of ``alt * w_alt[index * n_cols + h] + ref * w_ref[index * n_cols + h]``, modulo 2^64.  ``w_alt``,
        ``w_ref``: the addresses of n_minor * n_cols int32, minor-major; 0 leaves the term out (not both, unless n_minor is 0).  ``out``:
        the address of n_major * n_cols int64, each written once.  At most ``abi.CSR_DENSE_MAX`` columns."""
        self._check(self._L.vtx_csr_dense_sum(self._h, int(n_major), int(n_minor), int(nnz), indptr or None, indices or None, alt or None,
                                              ref or None, w_alt or None, w_ref or None, int(n_cols), out or None))

    def comm_init(self, ident: bytes, rank: int, world: int):
        """Join the RCCL communicator of the sharded run (collective; vtx_comm_init)."""
        assert len(ident) == COMM_ID_BYTES
        self._check(self._L.vtx_comm_init(self._h, C.c_char_p(ident), rank, world))

    def write_mtx(self, path: str, n_rows: int, n_cols: int, which: int = 0, real: bool = False) -> float:
        """The last run's triplets as Matrix-Market text, formatted on the device and streamed into ``path``; returns the sum of the
        values.  Raises VTX_E_UNSUPPORTED for non-integral values (alt_frac) unless ``real``: vtx_write_mtx_f64 formats those too
        (shortest round-trip digits, NaN; the sum is NaN when a value is)."""
        s = C.c_double(0.0)
        fn = self._L.vtx_write_mtx_f64 if real else self._L.vtx_write_mtx
        self._check(fn(self._h, path.encode(), n_rows, n_cols, which, C.byref(s)))
        return float(s.value)

    def write_mtx_gz(self, path: str, n_rows: int, n_cols: int, which: int = 0, real: bool = False):
        """``write_mtx`` gzip-compressed on the device (vtx_write_mtx_gz): ``path``, used as given, becomes a BGZF file whose
        decompressed bytes are ``write_mtx``'s; only the compressed bytes leave the card.  Returns (sum, text_bytes): the sum of the
        values and the uncompressed size."""
        s, t = C.c_double(0.0), C.c_uint64(0)
        self._check(self._L.vtx_write_mtx_gz(self._h, path.encode(), n_rows, n_cols, which, int(bool(real)), C.byref(s), C.byref(t)))
        return float(s.value), int(t.value)

    def mtx_part(self, which: int = 0, real: bool = False, gz: bool = False) -> abi.MtxPart:
        """The last run's triplets as a finished PART of a Matrix-Market file (vtx_mtx_part): the lines alone, formatted on the device
        (``gz``: deflated there into BGZF members) — for a matrix that several runs make; ``lib.mtx_join`` writes the parts behind a
        header.  ``which`` / ``real`` and the decline rule (VTX_E_UNSUPPORTED) as for ``write_mtx``."""
        st = abi.VtxMtxPart()
        self._check(self._L.vtx_mtx_part(self._h, which, int(bool(real)), int(bool(gz)), C.byref(st)))
        try:
            return abi.MtxPart.from_struct(st)
        finally:
            self._L.vtx_mtx_part_free(C.byref(st))

    def comm_ranks(self) -> int:
        n = C.c_int(0)
        self._check(self._L.vtx_comm_ranks(self._h, C.byref(n)))
        return int(n.value)

    def gather_coo(self, dst: int = 0) -> dict:
        """Collective: every rank's triplets to rank ``dst`` over RCCL (vtx_gather_coo).  Returns the device addresses of
        the gathered arrays + nnz on ``dst`` (nnz = 0 elsewhere), same form as ``device_coo``."""
        coo = abi.VtxCoo()
        self._check(self._L.vtx_gather_coo(self._h, dst, C.byref(coo)))
        out = {"nnz": int(coo.nnz)}
        for k in ("row", "col", "alt", "ref", "unk", "value", "ref_value"):
            out[k] = C.cast(getattr(coo, k), C.c_void_p).value or 0
        return out

    def gather_abort(self):
        """Collective: takes part in the status round of ``gather_coo`` with an error flag, so that the other ranks leave
        their ``gather_coo`` with VTX_E_PEER (vtx_gather_abort)."""
        self._check(self._L.vtx_gather_abort(self._h))

    def fetch_gathered(self) -> dict:
        coo = abi.VtxCoo()
        self._check(self._L.vtx_fetch_gathered(self._h, C.byref(coo)))
        n = int(coo.nnz)
        out = {}
        for k, dt in (("row", np.uint32), ("col", np.uint32), ("alt", np.uint32), ("ref", np.uint32),
                      ("unk", np.uint32), ("value", np.float64), ("ref_value", np.float64)):
            out[k] = np.ctypeslib.as_array(getattr(coo, k), shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dt)
        return out

    # ---- audit / test hooks (include/vtx.h: vtx_set_debug) ----
    def set_stage_trace(self, on: bool = True):
        self._check(self._L.vtx_set_debug(self._h, abi.DEBUG_STAGE_TRACE, int(bool(on))))

    def set_poison(self, value=None):
        """Every later run first fills the score arrays with ``value`` (None: off)."""
        if value is not None:
            self._check(self._L.vtx_set_debug(self._h, abi.DEBUG_POISON_VALUE, int(value)))
        self._check(self._L.vtx_set_debug(self._h, abi.DEBUG_POISON_SCORES, 0 if value is None else 1))

    def fetch_stage(self) -> np.ndarray:
        """One byte per task (2 * record + haplotype): the stage that decided its score (abi.STAGE_*)."""
        st = np.zeros(2 * self.n_records, np.uint8)
        self._check(self._L.vtx_fetch_stage(self._h, st.ctypes.data))
        return st

    def debug_bands(self, tasks, stride: int):
        """(lo, hi, status) of band_sweep_kernel for the given tasks of the resident batch (vtx_debug_bands)."""
        t = np.ascontiguousarray(tasks, np.uint32)
        lo = np.zeros((len(t), stride), np.uint16)
        hi = np.zeros((len(t), stride), np.uint16)
        status = np.zeros(len(t), np.uint8)
        self._check(self._L.vtx_debug_bands(self._h, t.ctypes.data, len(t), stride, lo.ctypes.data, hi.ctypes.data, status.ctypes.data))
        return lo, hi, status

    def debug_tables(self) -> np.ndarray:
        """The haplotype k-mer tables the last banded run left in global memory, as bytes (vtx_debug_tables); empty: tables in LDS."""
        n = C.c_uint64(0)
        self._check(self._L.vtx_debug_tables(self._h, None, 0, C.byref(n)))
        out = np.zeros(int(n.value), np.uint8)
        if n.value:
            self._check(self._L.vtx_debug_tables(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def timing(self) -> abi.VtxTiming:
        t = abi.VtxTiming()
        self._check(self._L.vtx_last_timing(self._h, C.byref(t)))
        return t

    def cells(self) -> int:
        n = C.c_uint64(0)
        self._check(self._L.vtx_last_cells(self._h, C.byref(n)))
        return int(n.value)
