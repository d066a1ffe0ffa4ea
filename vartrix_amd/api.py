"""The public Python entry point: the four input files in, the matrices out as scipy or torch CSR.

``run()`` is what the command line does (ingest -> ``vtx_run`` per range of loci) without the Matrix-Market text at the end: after every
run the variant-major CSR of its triplets is taken ON THE DEVICE (``vtx_device_csr``: only the row offsets are new, the other arrays
are the run's own), the parts of several runs are stacked (``stack_parts``), and the cell-major orientation — the ``X`` of an AnnData —
is one stable transpose of the stacked whole (``vtx_csr_transpose``).  Every array of the run comes back: the scoring mode's values
(the reference's ``matrix`` / ``ref_matrix``, src/main.rs:323-346) and the alt / ref / unknown counts behind them
(CellCounts, src/main.rs:1032-1039), which no file of the command line holds outside the coverage mode.

``run(stats=True)`` adds the seven statistics of every variant and of every cell (``vtx_csr_row_stats`` on the CSR and on its transpose),
``run(min_alt_cells=, min_ref_cells=)`` drops the variants too few cells inform before anything is transposed or copied (the locus
filter of the demultiplexers: ``vtx_csr_row_stats`` + ``vtx_csr_select`` on the stacked CSR), and ``select()`` cuts a finished result
down by boolean masks.

``pseudobulk()`` folds a result into variants x groups by a label per cell (cluster, donor, clone, sample): per (variant, group) the alt /
ref / unknown counts summed over the cells of the group and the number of its cells that support each allele (``vtx_csr_group_plan`` +
``vtx_csr_group_sum`` on the device for a torch result, scipy on the host for a scipy one); ``run(groups=)`` does it on the stacked CSR
of the run, and ``read_groups()`` reads the labels from a two-column file such as cellranger's ``clusters.csv``.

``donor_tally()`` produces what the donor label is made from when samples are pooled: per (cell, donor) pair the cell's alt and ref reads
by the class of the donor's known genotype at each variant (``vtx_csr_geno_tally`` on the device for a torch result, scipy on the host
for a scipy one; ``read_genotypes()`` reads the table from a VCF), and ``assign_donors()`` is the plain likelihood on top, in numpy.
``doublet_tally()`` is the same for droplets of two donors: per (cell, pair of donors) the reads by the dosage of the pair's genotypes
(``vtx_csr_geno_pair_tally``), and ``assign_doublets()`` scores the two-donor hypotheses next to the one-donor ones (50 : 50 mixtures).

``weighted_sum()`` is the integer part of the models that know no genotype classes: the CSR times one or two tables of int32 weights per
(variant, hypothesis), exact in int64 (``vtx_csr_dense_sum`` on the device for a torch result, scipy on the host for a scipy one), and
``cluster_donors()`` is genotype-free clustering on top of it: a soft EM whose two halves are that sum in the two orientations, with
the floating point between them in torch on the device (numpy for a scipy result).

There is no CPU path: the scores, the calls, the offsets and the transpose are computed on the GPU; torch carries the device arrays
(``__cuda_array_interface__``) and, for ``to="scipy"``, copies the finished arrays to the host.
"""
from __future__ import annotations

import gzip
import os
from dataclasses import dataclass

import numpy as np

from . import abi, hostlib, lib

DATA_FIELDS = ("value", "ref_value", "alt", "ref", "unk")          # the five data arrays of a part, vtx_coo's names
_ELEM_BYTES = {"value": 8, "ref_value": 8, "alt": 4, "ref": 4, "unk": 4}


@dataclass
class Result:
    matrix: object            # the scoring mode's values (consensus 1 / 2 / 3, alt_frac's fractions and NaN, coverage's alt counts)
    ref_matrix: object        # coverage mode: the ref counts (the reference's --ref-matrix); None otherwise
    alt_counts: object        # integer, same sparsity as ``matrix``
    ref_counts: object
    unknown_counts: object
    variants: list            # "{chrom}_{pos0}" per VCF record, what --out-variants writes
    barcodes: list
    metrics: dict             # the nine counters of hostlib.METRIC_NAMES (of the whole run, whatever is filtered afterwards)
    shape: tuple
    variant_stats: dict = None    # run(stats=True): abi.CSR_STAT_NAMES -> one array per (kept) variant
    cell_stats: dict = None       # ... per cell, of the matrix as returned
    variant_index: object = None  # the source row of every kept variant (int64); None when nothing was filtered
    orient: str = None            # "variants" or "cells": what the rows of the matrices are
    groups: object = None         # run(groups=): the GroupResult of the matrix as returned (after the filter)


@dataclass
class GroupResult:
    """A result folded by a label per cell: variants x groups (``orient="variants"``) or groups x variants (``"cells"``).  Every matrix
    is int64 and has an entry where at least one cell of the group has an entry for the variant (a scipy result folded on the host:
    where the number itself is not zero)."""
    alt_counts: object        # the alt / ref / unknown counts summed over the cells of the group
    ref_counts: object
    unknown_counts: object
    n_cells: object           # cells of the group with an entry for the variant
    n_alt_cells: object       # ... with alt support (alt > 0), with ref support, with both (what consensus writes as 3)
    n_ref_cells: object
    n_both_cells: object
    variants: list
    groups: list              # the distinct labels at least one cell of the run has, sorted: as numbers if every one parses as an int
    group_sizes: object       # cells per group, from the labels (numpy int64)
    shape: tuple
    orient: str
    n_unmatched: int = 0      # keys of a dict of labels that are no barcode of the run


# GroupResult field -> the statistic of vtx_csr_stats it is
_GROUP_FIELDS = {"alt_counts": "sum_alt", "ref_counts": "sum_ref", "unknown_counts": "sum_unk", "n_cells": "n_entries",
                 "n_alt_cells": "n_alt", "n_ref_cells": "n_ref", "n_both_cells": "n_both"}


def _is_torch(a) -> bool:
    return type(a).__module__.split(".")[0] == "torch"


def stack_parts(parts):
    """Stack CSR parts over consecutive row ranges into one CSR (what ``scipy.sparse.vstack`` does), on numpy arrays or torch tensors.

    A part is a dict with ``indptr`` (rows + 1 offsets starting at 0), ``indices`` and any number of further arrays of one element per
    entry (the same keys in every part).  Rows ascend from part to part, so stacking is concatenation: the entry arrays back to back,
    and each part's offsets (without its leading 0) shifted by the entries in front of it.  Pure: the parts are not changed.  No
    parts: the CSR of a matrix without rows (numpy)."""
    parts = list(parts)
    if not parts:
        return {"indptr": np.zeros(1, np.int64), "indices": np.zeros(0, np.int64)}
    keys = [k for k in parts[0] if k != "indptr"]
    if _is_torch(parts[0]["indptr"]):
        import torch
        cat = torch.cat
    else:
        cat = np.concatenate
    ptrs, base = [parts[0]["indptr"][:1] * 0], 0
    for p in parts:
        ptrs.append(p["indptr"][1:] + base)
        base += int(p["indptr"][-1])
    out = {"indptr": cat(ptrs)}
    for k in keys:
        out[k] = cat([p[k] for p in parts])
    return out


class _DevArray:
    """A raw device pointer as an object ``torch.as_tensor`` takes without a copy (``shard._DevArray``)."""

    def __init__(self, ptr: int, n: int, typestr: str):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _device_part(ctx, torch, dev, row_begin, row_end):
    """The last run's variant-major CSR over [row_begin, row_end) as CLONED torch tensors.  The library has finished writing the
    arrays when ``device_csr`` returns (it synchronises its own stream); the clones are copies torch queues on ITS current stream, so
    that stream is synchronised before this returns: only then may the next submit / run, on the library's stream, overwrite the
    source arrays.  After that the clones outlive the next run and the context."""
    d = ctx.device_csr(row_begin, row_end)
    n = d["nnz"]

    def take(key, count, typestr, dtype):
        if not count:
            return torch.zeros(0, dtype=dtype, device=dev)
        return torch.as_tensor(_DevArray(d[key], count, typestr), device=dev).clone()
    part = {"indptr": take("indptr", row_end - row_begin + 1, "<i8", torch.int64), "indices": take("indices", n, "<i4", torch.int32)}
    for k in DATA_FIELDS:
        part[k] = take(k, n, "<f8", torch.float64) if _ELEM_BYTES[k] == 8 else take(k, n, "<i4", torch.int32)
    torch.cuda.current_stream(dev).synchronize()     # the copies out of the context's arrays are complete (shard.gather_coo_async does the same)
    return part


def _empty_part(torch, dev, n_rows):
    part = {"indptr": torch.zeros(n_rows + 1, dtype=torch.int64, device=dev), "indices": torch.zeros(0, dtype=torch.int32, device=dev)}
    for k in DATA_FIELDS:
        part[k] = torch.zeros(0, dtype=torch.float64 if _ELEM_BYTES[k] == 8 else torch.int32, device=dev)
    return part


def _transpose(ctx, torch, dev, csr, n_major, n_minor, fields=DATA_FIELDS):
    """One stable transpose of the stacked CSR on the device; ``perm`` is computed once and moves every data array of ``fields``."""
    nnz = int(csr["indices"].shape[0])
    out = {"indptr": torch.empty(n_minor + 1, dtype=torch.int64, device=dev), "indices": torch.empty(nnz, dtype=torch.int32, device=dev)}
    for k in fields:
        out[k] = torch.empty_like(csr[k])
    src = {k: csr[k].contiguous() for k in ("indptr", "indices") + tuple(fields)}
    torch.cuda.synchronize(dev)              # the library works on its own stream: torch's writes to these arrays have to be done
    ctx.csr_transpose(n_major, n_minor, nnz, src["indptr"].data_ptr(), src["indices"].data_ptr(), out["indptr"].data_ptr(),
                      out["indices"].data_ptr(), 0, [(src[k].data_ptr(), out[k].data_ptr(), src[k].element_size()) for k in fields])
    return out


def _row_stats(ctx, torch, dev, csr, n_major, n_minor, names=abi.CSR_STAT_NAMES):
    """``names`` of the seven statistics of every row of a CSR with ``alt`` / ``ref`` / ``unk`` arrays, on the device: int64 tensors
    (the counts are exact; a sum is the library's uint64, exact below 2^63)."""
    nnz = int(csr["indices"].shape[0])
    raw = {k: torch.empty(n_major, dtype=torch.int32 if k in abi.CSR_STAT_COUNTS else torch.int64, device=dev) for k in names}
    src = {k: csr[k].contiguous() for k in ("indptr", "indices", "alt", "ref", "unk")}
    torch.cuda.synchronize(dev)
    ctx.csr_row_stats(n_major, n_minor, nnz, src["indptr"].data_ptr(), src["indices"].data_ptr(), src["alt"].data_ptr(), src["ref"].data_ptr(),
                      src["unk"].data_ptr(), {k: v.data_ptr() for k, v in raw.items()})
    return {k: (v.to(torch.int64) & 0xFFFFFFFF) if k in abi.CSR_STAT_COUNTS else v for k, v in raw.items()}


def _select(ctx, torch, dev, csr, n_major, n_minor, keep_major=None, keep_minor=None):
    """Rows and columns of a CSR (a dict of device tensors: ``indptr``, ``indices`` and any data arrays of 4- or 8-byte elements) by
    boolean device tensors, on the device: one plan, one select that moves every data array.  -> (the selected CSR, the source row of
    every kept row, the source column of every kept column; int32)."""
    nnz = int(csr["indices"].shape[0])
    fields = [k for k in csr if k not in ("indptr", "indices")]
    src = {k: v.contiguous() for k, v in csr.items()}
    masks = [None if m is None else m.to(device=dev, dtype=torch.bool).contiguous() for m in (keep_major, keep_minor)]
    ptrs = [0 if m is None else m.data_ptr() for m in masks]
    torch.cuda.synchronize(dev)
    head = (n_major, n_minor, nnz, src["indptr"].data_ptr(), src["indices"].data_ptr())
    sizes = ctx.csr_select_plan(*head, *ptrs)
    out = {"indptr": torch.empty(sizes[0] + 1, dtype=torch.int64, device=dev), "indices": torch.empty(sizes[2], dtype=torch.int32, device=dev)}
    for k in fields:
        out[k] = torch.empty(sizes[2], dtype=src[k].dtype, device=dev)
    major_ids, minor_ids = (torch.empty(n, dtype=torch.int32, device=dev) for n in sizes[:2])
    ctx.csr_select(*head, *ptrs, sizes, out["indptr"].data_ptr(), out["indices"].data_ptr(), major_ids.data_ptr(), minor_ids.data_ptr(),
                   [(src[k].data_ptr(), out[k].data_ptr(), src[k].element_size()) for k in fields])
    return out, major_ids, minor_ids


def read_groups(path) -> dict:
    """barcode -> label from a file of two columns, barcode then label: comma-separated for ``.csv`` / ``.csv.gz``, tab-separated
    otherwise; ``.gz`` is read through gzip.  A first line whose first field is ``Barcode`` or ``barcode`` is a header (cellranger's
    ``clusters.csv``).  Labels stay strings; empty lines are skipped."""
    path = os.fspath(path)
    name = path[:-3] if path.endswith(".gz") else path
    sep = "," if name.endswith(".csv") else "\t"
    out = {}
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path, "rt")) as f:
        for n, line in enumerate(f):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            fields = line.split(sep)
            if len(fields) < 2:
                raise ValueError("%s line %d: two columns, barcode and label, separated by %r" % (path, n + 1, sep))
            if n == 0 and fields[0] in ("Barcode", "barcode"):
                continue
            out[fields[0]] = fields[1]
    return out


def _labels(groups, barcodes):
    """The labels of the cells as numbers.  -> (uint32 per barcode: the position of its label in ``names``, abi.VTX_GROUP_NONE for a
    cell that is left out; names: the sorted distinct labels; cells per group (int64); keys of a dict that are no barcode)."""
    if isinstance(groups, (str, os.PathLike)):
        groups = read_groups(groups)
    n_unmatched = 0
    if isinstance(groups, dict):
        by_name = {(k.decode() if isinstance(k, bytes) else k): v for k, v in groups.items()}
        n_unmatched = len(set(by_name) - set(barcodes))
        per_cell = [by_name.get(b) for b in barcodes]
    else:
        per_cell = groups.cpu().tolist() if _is_torch(groups) else list(groups)      # (a tensor: cluster_donors' labels of a torch result)
        if len(per_cell) != len(barcodes):
            raise ValueError("pseudobulk: %d labels for %d barcodes: one label per cell (None leaves the cell out)" % (len(per_cell), len(barcodes)))
    names = list({g for g in per_cell if g is not None})
    try:
        names.sort(key=lambda g: (int(str(g)), str(g)))      # numbers, if every label is one
    except ValueError:
        names.sort(key=str)
    number = {g: i for i, g in enumerate(names)}
    labels = np.array([abi.VTX_GROUP_NONE if g is None else number[g] for g in per_cell], np.uint32).reshape(len(barcodes))
    sizes = np.bincount(labels[labels != abi.VTX_GROUP_NONE].astype(np.int64), minlength=len(names)).astype(np.int64)
    return labels, names, sizes, n_unmatched


def _group_sum(ctx, torch, dev, csr, n_major, n_minor, labels, n_groups):
    """A CSR with ``alt`` / ``ref`` / ``unk`` arrays summed per group of columns on the device: one plan, one sum.  -> the n_major x
    n_groups CSR (``indptr``, ``indices`` and the seven arrays of ``abi.CSR_STAT_NAMES``, int64)."""
    nnz = int(csr["indices"].shape[0])
    src = {k: csr[k].contiguous() for k in ("indptr", "indices", "alt", "ref", "unk")}
    group = torch.from_numpy(np.ascontiguousarray(labels, np.uint32).view(np.int32).copy()).to(dev)
    torch.cuda.synchronize(dev)
    head = (n_major, n_minor, nnz, src["indptr"].data_ptr(), src["indices"].data_ptr())
    n_out = ctx.csr_group_plan(*head, group.data_ptr(), n_groups)
    out = {"indptr": torch.empty(n_major + 1, dtype=torch.int64, device=dev), "indices": torch.empty(n_out, dtype=torch.int32, device=dev)}
    raw = {k: torch.empty(n_out, dtype=torch.int32 if k in abi.CSR_STAT_COUNTS else torch.int64, device=dev) for k in abi.CSR_STAT_NAMES}
    torch.cuda.synchronize(dev)
    ctx.csr_group_sum(*head, src["alt"].data_ptr(), src["ref"].data_ptr(), src["unk"].data_ptr(), group.data_ptr(), n_groups, n_out,
                      out["indptr"].data_ptr(), out["indices"].data_ptr(), {k: v.data_ptr() for k, v in raw.items()})
    for k, v in raw.items():
        out[k] = (v.to(torch.int64) & 0xFFFFFFFF) if k in abi.CSR_STAT_COUNTS else v
    return out


def _pseudobulk_device(ctx, torch, dev, csr, variants, barcodes, groups, orient, to):
    """The fold of a VARIANT-major device CSR (``indptr``, ``indices``, ``alt``, ``ref``, ``unk``) as a GroupResult; ``orient="cells"``:
    one more transpose, of the small result."""
    labels, names, sizes, n_unmatched = _labels(groups, barcodes)
    n_var, n_cell, n_groups = len(variants), len(barcodes), len(names)
    shape = (n_var, n_groups) if orient == "variants" else (n_groups, n_var)
    if not n_groups:                             # no cell has a label: nothing to sum, and the library takes no fold into 0 groups
        out = {"indptr": torch.zeros(shape[0] + 1, dtype=torch.int64, device=dev), "indices": torch.zeros(0, dtype=torch.int32, device=dev)}
        out.update({k: torch.zeros(0, dtype=torch.int64, device=dev) for k in abi.CSR_STAT_NAMES})
    else:
        out = _group_sum(ctx, torch, dev, csr, n_var, n_cell, labels, n_groups)
        if orient == "cells":
            out = _transpose(ctx, torch, dev, out, n_var, n_groups, abi.CSR_STAT_NAMES)
    if to == "torch":
        cols = out["indices"].to(torch.int64)
        mats = {f: torch.sparse_csr_tensor(out["indptr"], cols, out[k], size=shape) for f, k in _GROUP_FIELDS.items()}
    else:
        import scipy.sparse as sp
        indptr, cols = out["indptr"].cpu().numpy(), out["indices"].cpu().numpy()
        mats = {f: sp.csr_matrix((out[k].cpu().numpy(), cols, indptr), shape=shape) for f, k in _GROUP_FIELDS.items()}
    return GroupResult(**mats, variants=list(variants), groups=names, group_sizes=sizes, shape=shape, orient=orient, n_unmatched=n_unmatched)


def _pseudobulk_host(result, groups, orient):
    """The fold of a scipy result on the host: ``A @ one-hot`` for the sums, the same of ``A > 0`` for the support counts."""
    import scipy.sparse as sp
    labels, names, sizes, n_unmatched = _labels(groups, result.barcodes)
    n_var, n_cell, n_groups = len(result.variants), len(result.barcodes), len(names)
    cells = np.flatnonzero(labels != abi.VTX_GROUP_NONE)
    onehot = sp.csr_matrix((np.ones(len(cells), np.int64), (cells, labels[cells].astype(np.int64))), shape=(n_cell, n_groups))

    def fold(m):
        m = sp.csr_matrix(m).astype(np.int64)
        return sp.csr_matrix(m @ onehot if orient == "variants" else onehot.T @ m)
    alt, ref, unk = (sp.csr_matrix(m) for m in (result.alt_counts, result.ref_counts, result.unknown_counts))
    entries = sp.csr_matrix((np.ones(len(alt.data), np.int64), alt.indices, alt.indptr), shape=alt.shape)      # every stored entry, explicit zeros too
    has_alt, has_ref = alt > 0, ref > 0
    mats = dict(alt_counts=fold(alt), ref_counts=fold(ref), unknown_counts=fold(unk), n_cells=fold(entries), n_alt_cells=fold(has_alt),
                n_ref_cells=fold(has_ref), n_both_cells=fold(has_alt.multiply(has_ref)))
    shape = (n_var, n_groups) if orient == "variants" else (n_groups, n_var)
    return GroupResult(**mats, variants=list(result.variants), groups=names, group_sizes=sizes, shape=shape, orient=orient, n_unmatched=n_unmatched)


def _stats_out(st, to):
    """The statistics as the caller gets them: device tensors (int64) for torch, numpy for scipy (uint32 counts, uint64 sums)."""
    if to == "torch":
        return dict(st)
    return {k: v.cpu().numpy().astype(np.uint32) if k in abi.CSR_STAT_COUNTS else v.cpu().numpy().view(np.uint64) for k, v in st.items()}


def _finish(csr, field, shape, to, torch):
    if to == "torch":
        return torch.sparse_csr_tensor(csr["indptr"], csr["indices"].to(torch.int64), csr[field], size=shape)
    import scipy.sparse as sp
    data = csr[field].cpu().numpy()
    if data.dtype == np.int32:
        data = data.view(np.uint32)
    # (data, indices, indptr) as given: explicit zeros and NaN stay, nothing is summed or sorted
    return sp.csr_matrix((data, csr["indices"].cpu().numpy(), csr["indptr"].cpu().numpy()), shape=shape)


def run(vcf, bam, fasta, cell_barcodes, *, scoring_method="consensus", padding=100, mapq=0, primary_alignments=False,
        no_duplicates=False, umi=False, bam_tag="CB", valid_chars="ATGCatgc", aligner="banded", ingest="auto", stream_loci=None,
        threads=1, device=0, orient="variants", to="scipy", stats=False, min_alt_cells=0, min_ref_cells=0, groups=None) -> Result:
    """Genotype the cells of ``bam`` at the variants of ``vcf`` and return every matrix of the run as CSR.

    The arguments up to ``valid_chars`` are the command line's (the reference's, src/main.rs:54-160).  ``ingest``: "host" packs the
    reads on the CPU (``hostlib.pack_files``, every batch of a pack), "device" hands the BAM's bytes to the card
    (``hostlib.plan_ingest`` + ``submit_bam`` / ``submit_bam_segments``) and fails with the plan's or the device's reason, "auto" takes
    the plan where there is one and the host packer for a range the device declines (VTX_E_UNSUPPORTED), as the command line does.
    ``stream_loci=N``: the VCF in ranges of N records, one context reused.  ``orient``: "variants" (variants x cells, the files'
    orientation) or "cells" (cells x variants: AnnData's X).  ``to``: "scipy" (``scipy.sparse.csr_matrix`` on the host) or "torch"
    (``torch.sparse_csr_tensor`` on ``device``; the values never pass through the host).  Explicit zeros and NaN are kept.  The
    result does not depend on ``ingest``, ``stream_loci`` or ``to``.

    ``min_alt_cells=a, min_ref_cells=r`` (either > 0) keep the variants with alt support in at least ``a`` cells and ref support in at
    least ``r`` (``n_alt >= a and n_ref >= r``).  The filter runs on the stacked variant-major CSR on the device, before the transpose
    and before anything reaches the host: ``variants``, ``shape`` and every matrix follow the kept set, ``variant_index`` holds its
    source rows, ``metrics`` stay those of the whole run.  ``stats=True`` fills ``variant_stats`` and ``cell_stats``: per variant and
    per cell of the matrix as returned (after the filter) the number of entries, of entries with alt > 0, with ref > 0, with both, and
    the sums of the alt / ref / unknown counts — device tensors for ``to="torch"``, numpy for ``to="scipy"``.

    ``groups`` (a label per cell, a dict from barcode to label, or the path of a file ``read_groups`` takes: see ``pseudobulk``) fills
    ``Result.groups`` with the ``GroupResult`` of the run: the fold runs on the stacked variant-major CSR on the device, after the
    filter and before the transpose."""
    import torch
    if scoring_method not in abi.MODES:
        raise ValueError("scoring_method %r: one of %s" % (scoring_method, sorted(abi.MODES)))
    if aligner not in abi.ALIGNERS:
        raise ValueError("aligner %r: one of %s" % (aligner, sorted(abi.ALIGNERS)))
    if ingest not in ("auto", "host", "device"):
        raise ValueError("ingest %r: auto, host or device" % (ingest,))
    if orient not in ("variants", "cells"):
        raise ValueError("orient %r: variants or cells" % (orient,))
    if to not in ("scipy", "torch"):
        raise ValueError("to %r: scipy or torch" % (to,))
    if int(min_alt_cells) < 0 or int(min_ref_cells) < 0:
        raise ValueError("min_alt_cells %r / min_ref_cells %r: numbers of cells, 0 or more" % (min_alt_cells, min_ref_cells))
    if stream_loci is not None and int(stream_loci) < 1:
        raise ValueError("stream_loci %r: a positive number of VCF records, or None" % (stream_loci,))
    if isinstance(groups, (str, os.PathLike)):
        groups = read_groups(groups)         # a file that cannot be read fails before the run, not after it
    dev = torch.device("cuda", int(device))
    files = dict(vcf=str(vcf), bam=str(bam), fasta=str(fasta), cell_barcodes=str(cell_barcodes))
    filt = dict(padding=int(padding), mapq=int(mapq), primary_only=bool(primary_alignments), no_duplicates=bool(no_duplicates),
                use_umi=bool(umi), bam_tag=bam_tag, valid_chars=valid_chars, threads=int(threads))
    metrics = dict.fromkeys(hostlib.METRIC_NAMES, 0)
    state = {"ctx": None, "barcodes": None, "variants": None, "n_variants": None, "bc_set": False}
    parts = []

    def add(m):
        for k, v in m.items():
            metrics[k] += int(v)

    def context(n_variants, barcodes, variants):
        if state["ctx"] is None:
            cfg = abi.default_config(aligner=aligner, scoring_mode=scoring_method, use_umi=int(bool(umi)), n_barcodes=len(barcodes),
                                     device=int(device))
            state.update(ctx=lib.Context(cfg), barcodes=barcodes, variants=variants, n_variants=n_variants)
        return state["ctx"]

    def take(ctx, lo, hi):
        ctx.run()
        parts.append(_device_part(ctx, torch, dev, lo, hi))

    def window(lo, hi):
        nv = int(state["n_variants"])
        return min(lo, nv), (nv if hi is None else min(hi, nv))

    def host_range(rows, lo, hi):
        batches, m, nv, barcodes, variants = hostlib.pack_files(**files, **filt, all_batches=True, rows=rows)
        ctx = context(nv, barcodes, variants)
        lo, hi = window(lo, hi)
        add(m)
        batches = [b for b in batches if b.n_loci]
        if not batches:
            parts.append(_empty_part(torch, dev, hi - lo))
        for i, b in enumerate(batches):      # consecutive loci: a batch's rows end where the next batch's begin
            cut = int(batches[i + 1].loci["row"][0]) if i + 1 < len(batches) else hi
            ctx.submit(b)
            take(ctx, lo, cut)
            lo = cut

    def device_range(rows, lo, hi):
        """True: done on the device.  False: declined and ``ingest`` is auto (the host packs this range)."""
        with hostlib.plan_ingest(**files, **filt, rows=rows) as plan:
            ctx = context(plan.n_variants, plan.barcodes, plan.variants)
            lo, hi = window(lo, hi)
            if plan.reason is not None:
                if ingest == "device":
                    raise hostlib.HostError("no device ingest for rows [%d, %d): %s" % (lo, hi, plan.reason))
                return False
            if not plan.n_loci:              # nothing to look at in this range (skipped records only): its rows are empty
                add(plan.metrics)
                parts.append(_empty_part(torch, dev, hi - lo))
                return True
            if not state["bc_set"]:
                ctx.set_barcodes(plan.barcodes)
                state["bc_set"] = True
            try:
                st = ctx.submit_bam_segments(plan.segments, plan.n_loci) if plan.kind == "segmented" else ctx.submit_bam(plan.ingest, plan.n_loci)
            except lib.VtxError as e:
                if e.status == abi.VTX_E_UNSUPPORTED and ingest == "auto":
                    return False
                raise
            add(plan.metrics)
            add(dict(num_reads=st.num_reads, num_low_mapq=st.num_low_mapq, num_non_primary=st.num_non_primary,
                     num_duplicates=st.num_duplicates, num_not_useful=st.num_not_useful,
                     num_not_cell_bc=st.num_no_barcode_tag + st.raw.num_not_cell_bc, num_non_umi=st.raw.num_non_umi))
        take(ctx, lo, hi)
        return True

    try:
        lo = 0
        while True:                          # the number of VCF records is known once the first range is packed or planned
            hi = None if stream_loci is None else lo + int(stream_loci)
            rows = None if stream_loci is None else (lo, hi)
            if ingest == "host" or not device_range(rows, lo, hi):
                host_range(rows, lo, hi)
            lo = window(lo, hi)[1]
            if lo >= state["n_variants"]:
                break
        ctx = state["ctx"]
        n_rows, n_cols = int(state["n_variants"]), len(state["barcodes"])
        csr = stack_parts(parts)
        variants, variant_index = list(state["variants"]), None
        if int(min_alt_cells) > 0 or int(min_ref_cells) > 0:      # on the variant-major whole, before the transpose and any copy
            st = _row_stats(ctx, torch, dev, csr, n_rows, n_cols, ("n_alt", "n_ref"))
            keep = (st["n_alt"] >= int(min_alt_cells)) & (st["n_ref"] >= int(min_ref_cells))
            csr, kept, _ = _select(ctx, torch, dev, csr, n_rows, n_cols, keep, None)
            variant_index = kept.cpu().numpy().astype(np.int64)
            variants = [variants[i] for i in variant_index]
            n_rows = len(variants)
        variant_stats = cell_stats = None
        if stats:
            variant_stats = _stats_out(_row_stats(ctx, torch, dev, csr, n_rows, n_cols), to)
        barcodes = [b.decode() if isinstance(b, bytes) else b for b in state["barcodes"]]
        group_result = None
        if groups is not None:                   # on the variant-major whole as well: the transpose of orient="cells" is of the small result
            group_result = _pseudobulk_device(ctx, torch, dev, csr, variants, barcodes, groups, orient, to)
        shape = (n_rows, n_cols)
        if orient == "cells":
            csr = _transpose(ctx, torch, dev, csr, n_rows, n_cols)
            shape = (n_cols, n_rows)
        if stats:                                # the other axis: the same call on the transpose (the one orient="cells" needs anyway)
            by_cell = csr if orient == "cells" else _transpose(ctx, torch, dev, csr, n_rows, n_cols, ("alt", "ref", "unk"))
            cell_stats = _stats_out(_row_stats(ctx, torch, dev, by_cell, n_cols, n_rows), to)
        coverage = abi.MODES[scoring_method] == abi.MODE_COVERAGE
        return Result(matrix=_finish(csr, "value", shape, to, torch),
                      ref_matrix=_finish(csr, "ref_value", shape, to, torch) if coverage else None,
                      alt_counts=_finish(csr, "alt", shape, to, torch), ref_counts=_finish(csr, "ref", shape, to, torch),
                      unknown_counts=_finish(csr, "unk", shape, to, torch), variants=variants,
                      barcodes=barcodes, metrics=metrics, shape=shape,
                      variant_stats=variant_stats, cell_stats=cell_stats, variant_index=variant_index, orient=orient, groups=group_result)
    finally:
        if state["ctx"] is not None:
            state["ctx"].close()


_MATRIX_FIELDS = ("matrix", "ref_matrix", "alt_counts", "ref_counts", "unknown_counts")


def _mask(mask, n, what):
    """A boolean mask over ``n`` names as a numpy array (None: everything)."""
    if mask is None:
        return np.ones(n, bool)
    m = np.asarray(mask.cpu() if _is_torch(mask) else mask)
    if m.ndim != 1 or m.shape[0] != n:
        raise ValueError("select: the mask over the %s has shape %s, the result has %d %s" % (what, m.shape, n, what))
    if m.dtype != bool:
        raise ValueError("select: the mask over the %s has dtype %s: a boolean mask, one value per name" % (what, m.dtype))
    return m


def select(result: Result, variants=None, cells=None) -> Result:
    """The variants and cells of a ``Result`` that boolean masks keep (None: all), as a new ``Result`` of the same container type with
    the names trimmed; ``variant_index`` follows, ``metrics`` stay those of the run.  A torch result is cut on its device — one
    ``vtx_csr_select_plan`` and one ``vtx_csr_select`` move the data arrays of all its matrices, on a bare context for that device —
    a scipy result by scipy's own indexing on the host.  Statistics describe the matrix they were counted on and are not carried
    over.  ``ValueError`` for a mask of the wrong length."""
    n_var, n_cell = len(result.variants), len(result.barcodes)
    vm, cm = _mask(variants, n_var, "variants"), _mask(cells, n_cell, "cells")
    orient = result.orient or ("cells" if tuple(result.shape) == (n_cell, n_var) != (n_var, n_cell) else "variants")
    rows, cols = (vm, cm) if orient == "variants" else (cm, vm)
    mats = {f: getattr(result, f) for f in _MATRIX_FIELDS if getattr(result, f) is not None}
    shape = (int(rows.sum()), int(cols.sum()))
    if _is_torch(result.matrix):
        import torch
        first = result.matrix
        dev = first.device
        csr = {"indptr": first.crow_indices(), "indices": first.col_indices().to(torch.int32)}
        for f, m in mats.items():
            if m.values().shape[0] != csr["indices"].shape[0]:
                raise ValueError("select: %s does not have the sparsity of matrix" % f)
            csr[f] = m.values()
        index = torch.cuda.current_device() if dev.index is None else dev.index
        with lib.Context(abi.default_config(n_barcodes=max(n_cell, 1), device=index)) as ctx:    # no batch, no run: device, stream, work space
            out, _, _ = _select(ctx, torch, dev, csr, int(first.shape[0]), int(first.shape[1]), torch.as_tensor(rows, device=dev),
                                torch.as_tensor(cols, device=dev))
        cut = {f: torch.sparse_csr_tensor(out["indptr"], out["indices"].to(torch.int64), out[f], size=shape) for f in mats}
    else:
        cut = {f: m[rows][:, cols] for f, m in mats.items()}
    index = np.arange(n_var, dtype=np.int64) if result.variant_index is None else np.asarray(result.variant_index, np.int64)
    return Result(**{f: cut.get(f) for f in _MATRIX_FIELDS}, variants=[v for v, k in zip(result.variants, vm) if k],
                  barcodes=[b for b, k in zip(result.barcodes, cm) if k], metrics=dict(result.metrics), shape=shape,
                  variant_index=None if variants is None and result.variant_index is None else index[vm], orient=result.orient)


def pseudobulk(result: Result, groups, *, to=None) -> GroupResult:
    """Fold a ``Result`` by a label per cell into variants x groups (groups x variants for a result with ``orient="cells"``): per
    variant and group the alt / ref / unknown counts summed over the cells of the group, and the number of its cells with an entry,
    with alt support, with ref support and with both.

    ``groups``: a sequence of ``len(result.barcodes)`` labels, ``None`` leaving a cell out; or a dict from barcode to label — barcodes
    of the run that the dict lacks are left out, keys that are no barcode of the run are ignored and counted in ``n_unmatched``; or the
    path of a file ``read_groups`` takes.  ``GroupResult.groups`` is the sorted list of the distinct labels at least one cell has: by
    number if every label parses as an int, by ``str`` otherwise.  A filtered result folds its kept variants.

    A torch result is folded on its device — one ``vtx_csr_group_plan`` and one ``vtx_csr_group_sum`` on a bare context for that device
    (at most ``vtx_csr_group_max()`` groups) — into ``torch.sparse_csr_tensor``s, or into scipy matrices on the host with
    ``to="scipy"``; a scipy result is folded on the host with scipy."""
    n_var, n_cell = len(result.variants), len(result.barcodes)
    orient = result.orient or ("cells" if tuple(result.shape) == (n_cell, n_var) != (n_var, n_cell) else "variants")
    if to not in (None, "scipy", "torch"):
        raise ValueError("to %r: scipy, torch, or None for the container of the result" % (to,))
    if not _is_torch(result.alt_counts):
        if to == "torch":
            raise ValueError("pseudobulk: a scipy result is folded on the host; to=\"torch\" needs a torch result (run(to=\"torch\"))")
        return _pseudobulk_host(result, groups, orient)
    import torch
    first = result.alt_counts
    dev = first.device
    csr = {"indptr": first.crow_indices(), "indices": first.col_indices().to(torch.int32)}
    for k, m in (("alt", first), ("ref", result.ref_counts), ("unk", result.unknown_counts)):
        if m.values().shape[0] != csr["indices"].shape[0]:
            raise ValueError("pseudobulk: the count matrices do not have one sparsity")
        csr[k] = m.values().to(torch.int32)
    index = torch.cuda.current_device() if dev.index is None else dev.index
    with lib.Context(abi.default_config(n_barcodes=max(n_cell, 1), device=index)) as ctx:    # no batch, no run: device, stream, work space
        if orient == "cells":                    # back to variant-major: the fold sums over the columns
            csr = _transpose(ctx, torch, dev, csr, n_cell, n_var, ("alt", "ref", "unk"))
        return _pseudobulk_device(ctx, torch, dev, csr, result.variants, result.barcodes, groups, orient, to or "torch")


@dataclass
class DonorTally:
    """Every cell's reads by the genotype class of every donor: arrays of cells x donors x 4, int64 (numpy, or torch tensors on the
    result's device).  The last axis is the class of the donor's genotype at the variant of an entry: 0 hom-ref, 1 het, 2 hom-alt,
    3 missing."""
    alt: object               # alt reads of the cell at the variants where the donor has that class
    ref: object               # ref reads
    n_obs: object             # entries of the cell with alt + ref > 0 at those variants
    donors: list
    barcodes: list


@dataclass
class DonorAssignment:
    best: object              # int64 per cell: the donor (an index into ``donors``) with the highest likelihood; -1 for a cell without a read at a genotyped variant
    margin: object            # float64 per cell: the best log-likelihood minus the second best; +inf with one donor
    log_lik: object           # float64, cells x donors
    donors: list
    barcodes: list


_GT_CLASS = {("0", "0"): 0, ("0", "1"): 1, ("1", "0"): 1, ("1", "1"): 2}


def read_genotypes(path, variants):
    """The genotypes of the donors of a text VCF (plain or ``.gz``) at the variants of a run.  -> (uint8 array, len(variants) x
    donors: 0 hom-ref, 1 het, 2 hom-alt, ``abi.VTX_GENO_NONE`` missing; the donor names of the ``#CHROM`` line).

    A record belongs to the variant named ``"{chrom}_{pos0}"`` (``pos0`` = POS - 1: what ``Result.variants`` holds).  Its ``GT`` is
    split at ``/`` or ``|``: ``0/0`` is 0, ``0/1`` and ``1/0`` are 1, ``1/1`` is 2; everything else is missing — a ``.``, a haploid
    call, an allele index above 1, a record without ``GT``.  A name that occurs more than once, in the file or in ``variants``, is
    ambiguous and missing for every donor; so is a variant the file lacks."""
    path = os.fspath(path)
    times = {}
    for v in variants:
        times[v] = times.get(v, 0) + 1
    donors, seen, calls = [], {}, {}
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path, "rt")) as f:
        for line in f:
            line = line.rstrip("\r\n")
            if line.startswith("##") or not line.strip():
                continue
            fields = line.split("\t")
            if line.startswith("#"):
                donors = fields[9:]
                continue
            if len(fields) < 2:
                continue
            try:
                name = "%s_%d" % (fields[0], int(fields[1]) - 1)
            except ValueError:
                continue
            seen[name] = seen.get(name, 0) + 1
            if name not in times or seen[name] > 1:
                continue
            row = np.full(len(donors), abi.VTX_GENO_NONE, np.uint8)
            keys = fields[8].split(":") if len(fields) > 8 else []
            if "GT" in keys:
                at = keys.index("GT")
                for d, sample in enumerate(fields[9:9 + len(donors)]):
                    parts = sample.split(":")
                    gt = parts[at] if at < len(parts) else "."
                    row[d] = _GT_CLASS.get(tuple(gt.replace("|", "/").split("/")), abi.VTX_GENO_NONE)
            calls[name] = row
    geno = np.full((len(variants), len(donors)), abi.VTX_GENO_NONE, np.uint8)
    for i, v in enumerate(variants):
        if times[v] == 1 and seen.get(v, 0) == 1:
            geno[i] = calls[v]
    return geno, list(donors)


def _genotypes(genotypes, donors, variants):
    """The table as (uint8 array of len(variants) x donors, donor names), from an array or from a path for ``read_genotypes``."""
    if isinstance(genotypes, (str, os.PathLike)):
        geno, names = read_genotypes(genotypes, variants)
    else:
        raw = np.asarray(genotypes.cpu() if _is_torch(genotypes) else genotypes)
        if raw.ndim != 2 or raw.shape[0] != len(variants):
            raise ValueError("donor_tally: genotypes of shape %s: one row per variant of the result (%d), one column per donor" % (raw.shape, len(variants)))
        wide = raw.astype(np.int64)
        bad = np.argwhere(~np.isin(wide, (0, 1, 2, abi.VTX_GENO_NONE)))
        if len(bad):
            raise ValueError("donor_tally: the genotype of variant %d, donor %d is %d: 0, 1, 2 or VTX_GENO_NONE" % (bad[0][0], bad[0][1], wide[tuple(bad[0])]))
        geno, names = np.ascontiguousarray(wide.astype(np.uint8)), list(range(raw.shape[1]))
    if donors is not None:
        names = list(donors)
        if len(names) != geno.shape[1]:
            raise ValueError("donor_tally: %d donor names for %d columns of genotypes" % (len(names), geno.shape[1]))
    return geno, names


def _class_tally(call, torch, dev, csr, n_major, n_minor, geno, n_donors, n_hyp, n_classes, pairs=None):
    """A CELL-major CSR with ``alt`` / ``ref`` arrays against the table, and the ``pairs`` if any, on the device: ``call`` is
    ``ctx.csr_geno_tally`` or ``ctx.csr_geno_pair_tally`` -> the three arrays of ``abi.GENO_TALLY_NAMES`` as int64 tensors of
    n_major x n_hyp x n_classes."""
    nnz = int(csr["indices"].shape[0])
    src = {k: csr[k].contiguous() for k in ("indptr", "indices", "alt", "ref")}
    table = torch.from_numpy(np.ascontiguousarray(geno, np.uint8).reshape(-1).copy()).to(dev)
    hyp = ()
    if pairs is not None:
        plist = torch.from_numpy(pairs.astype(np.int32).reshape(-1).copy()).to(dev)     # < n_donors <= vtx_csr_geno_max(): the bits of the uint32
        hyp = (plist.data_ptr(), n_hyp)
    n = n_major * n_hyp * n_classes
    raw = {"sum_alt": torch.empty(n, dtype=torch.int64, device=dev), "sum_ref": torch.empty(n, dtype=torch.int64, device=dev),
           "n_obs": torch.empty(n, dtype=torch.int32, device=dev)}
    torch.cuda.synchronize(dev)
    call(n_major, n_minor, nnz, src["indptr"].data_ptr(), src["indices"].data_ptr(), src["alt"].data_ptr(), src["ref"].data_ptr(),
         table.data_ptr(), n_donors, *hyp, {k: v.data_ptr() for k, v in raw.items()})
    raw["n_obs"] = raw["n_obs"].to(torch.int64) & 0xFFFFFFFF
    return {k: v.reshape(n_major, n_hyp, n_classes) for k, v in raw.items()}


def _geno_tally(ctx, torch, dev, csr, n_major, n_minor, geno, n_donors):
    """``vtx_csr_geno_tally`` -> int64 tensors of n_major x n_donors x 4."""
    return _class_tally(ctx.csr_geno_tally, torch, dev, csr, n_major, n_minor, geno, n_donors, n_donors, 4)


def _class_tally_host(result, cls, n_classes, orient):
    """The tally of a scipy result on the host from ``cls``, the class of every (variant, hypothesis): per class ``A^T @ (cls == c)``
    for a variant-major ``A``, ``A @ (cls == c)`` for a cell-major one; ``A`` the alt counts, the ref counts, and the indicator of
    alt + ref > 0.  -> the three arrays of ``abi.GENO_TALLY_NAMES``, int64, cells x hypotheses x n_classes."""
    import scipy.sparse as sp
    alt, ref = (sp.csr_matrix(m).astype(np.int64) for m in (result.alt_counts, result.ref_counts))
    obs = sp.csr_matrix((alt + ref) > 0).astype(np.int64)
    n_cell, n_hyp = len(result.barcodes), cls.shape[1]
    out = {k: np.zeros((n_cell, n_hyp, n_classes), np.int64) for k in abi.GENO_TALLY_NAMES}
    for c in range(n_classes):
        has = (cls == c).astype(np.int64)
        for k, m in (("sum_alt", alt), ("sum_ref", ref), ("n_obs", obs)):
            out[k][:, :, c] = np.asarray((m.T if orient == "variants" else m) @ has).reshape(n_cell, n_hyp)
    return out


def _donor_tally_host(result, geno, orient):
    """The class of (variant, donor) is the donor's genotype, 3 where it has no call."""
    wide = geno.astype(np.int64)
    return _class_tally_host(result, np.where(wide == abi.VTX_GENO_NONE, 3, wide), 4, orient)


def _tally_head(result, genotypes, donors, to):
    """What ``donor_tally`` and ``doublet_tally`` begin with -> (orient, n_var, n_cell, the table, the donor names)."""
    n_var, n_cell = len(result.variants), len(result.barcodes)
    orient = result.orient or ("cells" if tuple(result.shape) == (n_cell, n_var) != (n_var, n_cell) else "variants")
    if to not in (None, "scipy", "torch"):
        raise ValueError("to %r: scipy, torch, or None for the container of the result" % (to,))
    geno, names = _genotypes(genotypes, donors, result.variants)
    return orient, n_var, n_cell, geno, names


def _tally_csr(who, result, torch):
    """The alt and ref counts of a torch result as the CSR arrays the tallies take -> (csr, device)."""
    first = result.alt_counts
    if first.values().shape[0] != result.ref_counts.values().shape[0]:
        raise ValueError("%s: the count matrices do not have one sparsity" % who)
    return {"indptr": first.crow_indices(), "indices": first.col_indices().to(torch.int32), "alt": first.values().to(torch.int32),
            "ref": result.ref_counts.values().to(torch.int32)}, first.device


def donor_tally(result: Result, genotypes, donors=None, *, to=None) -> DonorTally:
    """Every cell's reads tallied against the known genotypes of pooled donors: per (cell, donor) pair the alt reads, the ref reads and
    the informative entries of the cell, by the class of the donor's genotype at the entry's variant (0 hom-ref, 1 het, 2 hom-alt,
    3 missing) — the integer part of scoring cells against donors, and what ``assign_donors`` takes.

    ``genotypes``: an array of ``len(result.variants)`` x donors holding 0, 1, 2 or ``abi.VTX_GENO_NONE``, or the path of a VCF for
    ``read_genotypes``; a result cut by ``select`` takes the table cut by the same mask.  ``donors``: their names (default: the VCF's
    sample names, or 0, 1, ... for an array).

    A torch result is tallied on its device — one ``vtx_csr_geno_tally`` on a bare context for that device (at most
    ``vtx_csr_geno_max()`` donors), after one transpose of the alt and ref counts if the result is variant-major — into int64
    tensors, or into numpy arrays with ``to="scipy"``; a scipy result is tallied on the host with scipy into numpy arrays."""
    orient, n_var, n_cell, geno, names = _tally_head(result, genotypes, donors, to)
    n_donors = geno.shape[1]
    if not _is_torch(result.alt_counts):
        if to == "torch":
            raise ValueError("donor_tally: a scipy result is tallied on the host; to=\"torch\" needs a torch result (run(to=\"torch\"))")
        out = _donor_tally_host(result, geno, orient)
        return DonorTally(alt=out["sum_alt"], ref=out["sum_ref"], n_obs=out["n_obs"], donors=names, barcodes=list(result.barcodes))
    import torch
    csr, dev = _tally_csr("donor_tally", result, torch)
    if not n_donors:                             # nothing to tally against, and the library takes no table without donors
        out = {k: torch.zeros((n_cell, 0, 4), dtype=torch.int64, device=dev) for k in abi.GENO_TALLY_NAMES}
    else:
        index = torch.cuda.current_device() if dev.index is None else dev.index
        with lib.Context(abi.default_config(n_barcodes=max(n_cell, 1), device=index)) as ctx:    # no batch, no run: device, stream, work space
            if orient == "variants":             # to cell-major: a wavefront tallies the row of a cell
                csr = _transpose(ctx, torch, dev, csr, n_var, n_cell, ("alt", "ref"))
            out = _geno_tally(ctx, torch, dev, csr, n_cell, n_var, geno, n_donors)
    if to == "scipy":
        out = {k: v.cpu().numpy() for k, v in out.items()}
    return DonorTally(alt=out["sum_alt"], ref=out["sum_ref"], n_obs=out["n_obs"], donors=names, barcodes=list(result.barcodes))


def assign_donors(tally_or_result, genotypes=None, *, error=0.01) -> DonorAssignment:
    """The most likely donor of every cell under the plain genotype model: a read of a cell shows the alt allele with probability
    ``p = (error, 0.5, 1 - error)`` where its donor is hom-ref, het, hom-alt.  Takes a ``DonorTally``, or a ``Result`` with the
    ``genotypes`` ``donor_tally`` takes.  In numpy float64, from the integer tallies, in exactly this order:

        ll = alt[..., 0] * log(p[0]) + ref[..., 0] * log1p(-p[0]) + alt[..., 1] * log(p[1]) + ref[..., 1] * log1p(-p[1])
             + alt[..., 2] * log(p[2]) + ref[..., 2] * log1p(-p[2])

    so that the same tallies give the same bits wherever they were counted.  Missing genotypes contribute nothing.  ``best`` is the
    donor with the highest ``ll``, the lowest index on a tie, and -1 for a cell whose ``n_obs`` over the classes 0 - 2 is zero for every
    donor; ``margin`` is the best minus the second best, ``+inf`` with one donor.  ``error`` must lie in (0, 0.5).

    Droplets of two donors are ``doublet_tally``'s and ``assign_doublets``'; pools without genotypes (souporcell's and vireo's other
    modes) are ``cluster_donors``'.  Out of scope: ambient RNA (a matter of other tables for ``weighted_sum``)."""
    if not 0.0 < float(error) < 0.5:
        raise ValueError("assign_donors: error %r: a probability in (0, 0.5)" % (error,))
    tally = tally_or_result
    if isinstance(tally, Result):
        if genotypes is None:
            raise ValueError("assign_donors: a Result needs the genotypes of the donors")
        tally = donor_tally(tally, genotypes, to="scipy" if _is_torch(tally.alt_counts) else None)
    alt, ref, n_obs = (np.asarray(a.cpu() if _is_torch(a) else a).astype(np.float64) for a in (tally.alt, tally.ref, tally.n_obs))
    p = (float(error), 0.5, 1.0 - float(error))
    ll = (alt[..., 0] * np.log(p[0]) + ref[..., 0] * np.log1p(-p[0]) + alt[..., 1] * np.log(p[1]) + ref[..., 1] * np.log1p(-p[1])
          + alt[..., 2] * np.log(p[2]) + ref[..., 2] * np.log1p(-p[2]))
    n_cell, n_donors = ll.shape
    if n_donors:
        best = np.argmax(ll, axis=1).astype(np.int64)
        best[n_obs[..., :3].sum(axis=(1, 2)) == 0] = -1
    else:
        best = np.full(n_cell, -1, np.int64)
    if n_donors >= 2:
        top = np.sort(ll, axis=1)
        margin = top[:, -1] - top[:, -2]
    else:
        margin = np.full(n_cell, np.inf)
    return DonorAssignment(best=best, margin=margin, log_lik=ll, donors=list(tally.donors), barcodes=list(tally.barcodes))


@dataclass
class DoubletTally:
    """Every cell's reads by the dosage class of pairs of donors: arrays of cells x pairs x 6, int64 (numpy, or torch tensors on the
    result's device).  The last axis is the class of the pair (a, b) at the variant of an entry: the dosage ``g_a + g_b`` in 0 .. 4,
    and 5 where either donor has no call."""
    alt: object               # alt reads of the cell at the variants where the pair has that class
    ref: object               # ref reads
    n_obs: object             # entries of the cell with alt + ref > 0 at those variants
    pairs: object             # int64, n_pairs x 2 (numpy): indices into ``donors``
    donors: list
    barcodes: list


@dataclass
class DoubletAssignment:
    kind: object              # int8 per cell: 1 doublet, 0 singlet, -1 for a cell without a read at a genotyped variant
    best: object              # int64 per cell: the singlet donor, ``assign_donors``' ``best``
    best_pair: object         # int64 per cell: the pair (an index into ``pairs``) with the highest likelihood; -1 without pairs
    log_odds: object          # float64 per cell: the best doublet hypothesis against the best singlet one, priors included
    log_lik_pairs: object     # float64, cells x pairs
    pairs: object
    donors: list
    barcodes: list


def _pairs(pairs, n_donors):
    """The list of pairs as an int64 array of n_pairs x 2: the caller's, or every a < b in ``np.triu_indices(n_donors, 1)`` order."""
    raw = None if pairs is None else np.asarray(pairs.cpu() if _is_torch(pairs) else pairs)
    if (raw is None and n_donors < 2) or (raw is not None and raw.size == 0):
        return np.zeros((0, 2), np.int64)                     # no list: no library call either
    most = int(lib.load().vtx_csr_geno_pair_max())
    if raw is None:
        if n_donors * (n_donors - 1) // 2 > most:
            raise ValueError("doublet_tally: %d donors have %d pairs, more than the %d of one call: pass `pairs` (the candidates, such as the "
                             "pairs of every cell's best few donors)" % (n_donors, n_donors * (n_donors - 1) // 2, most))
        a, b = np.triu_indices(n_donors, 1)
        return np.stack([a, b], axis=1).astype(np.int64)
    if raw.ndim != 2 or raw.shape[1] != 2 or raw.dtype.kind not in "iu":
        raise ValueError("doublet_tally: pairs of shape %s, dtype %s: integers, one row (a, b) per pair" % (raw.shape, raw.dtype))
    out = np.ascontiguousarray(raw.astype(np.int64))
    bad = np.flatnonzero(((out < 0) | (out >= n_donors)).any(axis=1))
    if len(bad):
        raise ValueError("doublet_tally: pair %d is (%d, %d): donors are 0 .. %d" % (bad[0], out[bad[0], 0], out[bad[0], 1], n_donors - 1))
    if len(out) > most:
        raise ValueError("doublet_tally: %d pairs: at most %d in one call" % (len(out), most))
    return out


def _geno_pair_tally(ctx, torch, dev, csr, n_major, n_minor, geno, n_donors, pairs):
    """``vtx_csr_geno_pair_tally`` -> int64 tensors of n_major x n_pairs x 6."""
    return _class_tally(ctx.csr_geno_pair_tally, torch, dev, csr, n_major, n_minor, geno, n_donors, len(pairs), abi.GENO_PAIR_CLASSES, pairs)


def _doublet_tally_host(result, geno, pairs, orient):
    """The class of (variant, pair) is the dosage of the two donors, 5 where either has no call."""
    ga, gb = geno[:, pairs[:, 0]].astype(np.int64), geno[:, pairs[:, 1]].astype(np.int64)
    cls = np.where((ga == abi.VTX_GENO_NONE) | (gb == abi.VTX_GENO_NONE), abi.GENO_PAIR_CLASSES - 1, ga + gb)
    return _class_tally_host(result, cls, abi.GENO_PAIR_CLASSES, orient)


def doublet_tally(result: Result, genotypes, pairs=None, donors=None, *, to=None) -> DoubletTally:
    """Every cell's reads tallied against PAIRS of pooled donors: per (cell, pair) the alt reads, the ref reads and the informative
    entries of the cell, by the dosage ``g_a + g_b`` (0 .. 4) of the pair's known genotypes at the entry's variant, and in class 5 where
    either donor has no call — the integer part of scoring the two-donor hypotheses, and what ``assign_doublets`` takes beside a
    ``DonorTally``.  The six classes assume the two cells of a droplet contribute reads in equal parts (50 : 50); other proportions
    are out of scope, as is ambient RNA (both are a matter of other tables for ``weighted_sum``); clustering without genotypes is
    ``cluster_donors``'.

    ``genotypes``, ``donors``: as for ``donor_tally``.  ``pairs``: integers of n_pairs x 2, indices into the donors; any list is
    allowed — duplicates, both orders, ``(a, a)``, which carries donor a's one-donor tally on the classes 0, 2, 4.  ``None`` means every
    ``a < b`` in ``np.triu_indices(n_donors, 1)`` order; beyond ``vtx_csr_geno_pair_max()`` = 4 096 pairs (91 donors and more) that is a
    ``ValueError``: pass the candidate pairs.

    A torch result is tallied on its device — one ``vtx_csr_geno_pair_tally`` on a bare context for that device (one GPU, fewer than
    2^32 entries), after one transpose of the alt and ref counts if the result is variant-major — into int64 tensors, or into numpy
    arrays with ``to="scipy"``; a scipy result is tallied on the host with scipy into numpy arrays.  Zero donors or zero pairs give
    empty arrays without a library call."""
    orient, n_var, n_cell, geno, names = _tally_head(result, genotypes, donors, to)
    n_donors = geno.shape[1]
    plist = _pairs(pairs, n_donors)
    n_pairs = len(plist)
    on_device = _is_torch(result.alt_counts)
    if not on_device and to == "torch":
        raise ValueError("doublet_tally: a scipy result is tallied on the host; to=\"torch\" needs a torch result (run(to=\"torch\"))")
    if not on_device:
        if n_pairs:
            out = _doublet_tally_host(result, geno, plist, orient)
        else:
            out = {k: np.zeros((n_cell, 0, abi.GENO_PAIR_CLASSES), np.int64) for k in abi.GENO_TALLY_NAMES}
    else:
        import torch
        csr, dev = _tally_csr("doublet_tally", result, torch)
        if not n_pairs:                          # nothing to tally against, and the library takes no empty list
            out = {k: torch.zeros((n_cell, 0, abi.GENO_PAIR_CLASSES), dtype=torch.int64, device=dev) for k in abi.GENO_TALLY_NAMES}
        else:
            index = torch.cuda.current_device() if dev.index is None else dev.index
            with lib.Context(abi.default_config(n_barcodes=max(n_cell, 1), device=index)) as ctx:    # no batch, no run: device, stream, work space
                if orient == "variants":         # to cell-major: a wavefront tallies the row of a cell
                    csr = _transpose(ctx, torch, dev, csr, n_var, n_cell, ("alt", "ref"))
                out = _geno_pair_tally(ctx, torch, dev, csr, n_cell, n_var, geno, n_donors, plist)
        if to == "scipy":
            out = {k: v.cpu().numpy() for k, v in out.items()}
    return DoubletTally(alt=out["sum_alt"], ref=out["sum_ref"], n_obs=out["n_obs"], pairs=plist, donors=names, barcodes=list(result.barcodes))


def assign_doublets(singlets: DonorTally, doublets: DoubletTally, *, error=0.01, doublet_prior=0.5) -> DoubletAssignment:
    """Singlet or doublet, per cell, under the plain genotype model with the two cells of a doublet mixed 50 : 50: a read of a droplet
    of the donors (a, b) shows the alt allele with probability ``q = (error, 0.25, 0.5, 0.75, 1 - error)`` at the dosage ``g_a + g_b``
    = 0 .. 4.  Takes ``donor_tally``'s and ``doublet_tally``'s outputs for the same cells.  In numpy float64, from the integer tallies,
    in exactly this order:

        ll2 = alt[..., 0] * log(q[0]) + ref[..., 0] * log1p(-q[0]) + alt[..., 1] * log(q[1]) + ref[..., 1] * log1p(-q[1])
              + alt[..., 2] * log(q[2]) + ref[..., 2] * log1p(-q[2]) + alt[..., 3] * log(q[3]) + ref[..., 3] * log1p(-q[3])
              + alt[..., 4] * log(q[4]) + ref[..., 4] * log1p(-q[4])
        ll1 = assign_donors(singlets, error=error).log_lik
        log_odds = (max(ll2) + log(doublet_prior) - log(n_pairs)) - (max(ll1) + log1p(-doublet_prior) - log(n_donors))

    so that the same tallies give the same bits wherever they were counted.  Class 5 (a donor without a call) contributes nothing.
    ``kind`` is 1 (doublet) where ``log_odds > 0``, 0 (singlet) otherwise, and -1 where ``assign_donors`` gives -1; ``best`` is
    ``assign_donors``' donor; ``best_pair`` the pair with the highest ``ll2``, the lowest index on a tie.  Without pairs ``best_pair``
    is -1 and ``log_odds`` is -inf: no doublet hypothesis was scored.  ``error`` must lie in (0, 0.5), ``doublet_prior`` in (0, 1).

    Out of scope: mixtures other than 50 : 50 and ambient RNA (both a matter of other tables for ``weighted_sum``).  Clustering without
    genotypes is ``cluster_donors``'."""
    if not 0.0 < float(error) < 0.5:
        raise ValueError("assign_doublets: error %r: a probability in (0, 0.5)" % (error,))
    if not 0.0 < float(doublet_prior) < 1.0:
        raise ValueError("assign_doublets: doublet_prior %r: a probability in (0, 1)" % (doublet_prior,))
    if list(singlets.barcodes) != list(doublets.barcodes):
        raise ValueError("assign_doublets: the two tallies are not of the same cells")
    one = assign_donors(singlets, error=error)
    alt, ref = (np.asarray(a.cpu() if _is_torch(a) else a).astype(np.float64) for a in (doublets.alt, doublets.ref))
    q = (float(error), 0.25, 0.5, 0.75, 1.0 - float(error))
    ll2 = (alt[..., 0] * np.log(q[0]) + ref[..., 0] * np.log1p(-q[0]) + alt[..., 1] * np.log(q[1]) + ref[..., 1] * np.log1p(-q[1])
           + alt[..., 2] * np.log(q[2]) + ref[..., 2] * np.log1p(-q[2]) + alt[..., 3] * np.log(q[3]) + ref[..., 3] * np.log1p(-q[3])
           + alt[..., 4] * np.log(q[4]) + ref[..., 4] * np.log1p(-q[4]))
    n_cell, n_pairs = ll2.shape
    n_donors = one.log_lik.shape[1]
    if n_pairs and n_donors:
        best_pair = np.argmax(ll2, axis=1).astype(np.int64)
        log_odds = ((np.max(ll2, axis=1) + np.log(float(doublet_prior)) - np.log(float(n_pairs)))
                    - (np.max(one.log_lik, axis=1) + np.log1p(-float(doublet_prior)) - np.log(float(n_donors))))
    else:
        best_pair = np.argmax(ll2, axis=1).astype(np.int64) if n_pairs else np.full(n_cell, -1, np.int64)
        log_odds = np.full(n_cell, np.inf if n_pairs else -np.inf)
    kind = (log_odds > 0).astype(np.int8)
    kind[one.best < 0] = -1
    return DoubletAssignment(kind=kind, best=one.best, best_pair=best_pair, log_odds=log_odds, log_lik_pairs=ll2,
                             pairs=np.asarray(doublets.pairs), donors=list(doublets.donors), barcodes=list(doublets.barcodes))


SCORE_SCALE = 2 ** 20          # S: a log-probability as an int32 weight is rint(S * log p)
RESP_SCALE = 2 ** 15           # Q: a responsibility as an int32 weight is rint(Q * r), r in [0, 1]
CLUSTER_MAX = 64               # the dense theta table of cluster_donors is the limit, not the kernel (abi.CSR_DENSE_MAX columns)


@dataclass
class DonorClusters:
    """Cells clustered by donor without genotypes (``cluster_donors``): numpy arrays, or torch tensors on the result's device."""
    labels: object            # int64 per cell: the cluster with the highest score, the lowest index on a tie; -1 for a cell without a read
    resp: object              # float64, cells x k: the responsibilities rq / RESP_SCALE; rows of cells without a read are 0
    score: object             # int64, cells x k: the last round's fixed-point log-likelihoods, weighted_sum(w_alt, w_ref)
    theta: object             # float64, variants x k: the alt probability of every variant in every cluster
    w_alt: object             # int32, variants x k: rint(SCORE_SCALE * log(theta)), the table ``score`` was summed with
    w_ref: object             # int32, variants x k: rint(SCORE_SCALE * log1p(-theta))
    log_lik: float            # the sum over the cells with a read of logsumexp(score / SCORE_SCALE)
    n_iter: int               # rounds of the winning restart
    converged: bool           # ... which ended below ``tol``
    restart: int              # the winning restart
    barcodes: list
    variants: list


def _orient(result):
    n_var, n_cell = len(result.variants), len(result.barcodes)
    return result.orient or ("cells" if tuple(result.shape) == (n_cell, n_var) != (n_var, n_cell) else "variants")


def _dense_table(w, n_rows, what, torch=None, dev=None):
    """A table of weights as a C-contiguous int32 array of ``n_rows`` x columns: numpy, or a tensor on ``dev`` when ``torch`` is given."""
    if w is None:
        return None
    if _is_torch(w):
        if str(w.dtype) != "torch.int32":
            raise ValueError("weighted_sum: %s is %s: the tables are int32" % (what, w.dtype))
        w = w.to(dev).contiguous() if torch is not None else np.ascontiguousarray(w.cpu().numpy())
    else:
        w = np.asarray(w)
        if w.dtype != np.int32:
            raise ValueError("weighted_sum: %s is %s: the tables are int32" % (what, w.dtype))
        w = torch.from_numpy(np.ascontiguousarray(w)).to(dev) if torch is not None else np.ascontiguousarray(w)
    if w.ndim != 2 or w.shape[0] != n_rows:
        raise ValueError("weighted_sum: %s of shape %s: %d rows (one per variant for over=\"cells\", per cell for over=\"variants\"), one column per hypothesis"
                         % (what, tuple(w.shape), n_rows))
    return w


def _dense_guard(w_alt, w_ref, max_row):
    """The guard against a wrapped sum: no |sum| can reach 2^63 when max|w| * (the largest row's alt + ref reads) stays below it."""
    most = 0
    for w in (w_alt, w_ref):
        if w is not None and w.shape[0] and w.shape[1]:
            most = max(most, -int(w.min()), int(w.max()))
    if most * max_row >= 1 << 63:
        raise ValueError("weighted_sum: max|w| = %d times the %d reads of the largest row reaches 2^63: the 64-bit sum could wrap" % (most, max_row))


def _dense_operand_host(result, over):
    """The alt and ref counts of a scipy result as int64 matrices whose rows are what ``over`` names, and the largest row's reads."""
    import scipy.sparse as sp
    alt, ref = (sp.csr_matrix(m).astype(np.int64) for m in (result.alt_counts, result.ref_counts))
    if _orient(result) != over:
        alt, ref = sp.csr_matrix(alt.T), sp.csr_matrix(ref.T)
    rows = np.asarray(alt.sum(axis=1)).reshape(-1) + np.asarray(ref.sum(axis=1)).reshape(-1)
    return (alt, ref), rows


def _dense_sum_host(op, w_alt, w_ref, n_cols):
    """scipy's sparse x dense product in int64: exact wherever the guard held."""
    out = np.zeros((op[0].shape[0], n_cols), np.int64)
    for m, w in zip(op, (w_alt, w_ref)):
        if w is not None:
            out += np.asarray(m @ w.astype(np.int64)).reshape(out.shape)
    return out


def _dense_operands_device(ctx, torch, dev, result, overs):
    """The alt and ref counts of a torch result as the CSR arrays vtx_csr_dense_sum takes, in each orientation of ``overs`` (one
    ``vtx_csr_transpose`` for the orientation the result does not have) -> {over: (csr, n_major, n_minor, reads per row (int64))}."""
    csr, _ = _tally_csr("weighted_sum", result, torch)
    csr = {k: v.contiguous() for k, v in csr.items()}
    n_var, n_cell = len(result.variants), len(result.barcodes)
    have = _orient(result)
    size = {"variants": (n_var, n_cell), "cells": (n_cell, n_var)}
    out = {}
    for over in overs:
        c = csr if over == have else _transpose(ctx, torch, dev, csr, *size[have], ("alt", "ref"))
        reads = (c["alt"].to(torch.int64) & 0xFFFFFFFF) + (c["ref"].to(torch.int64) & 0xFFFFFFFF)
        upto = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(reads, 0)])
        out[over] = (c, size[over][0], size[over][1], upto[c["indptr"][1:]] - upto[c["indptr"][:-1]])
    return out


def _dense_sum_device(ctx, torch, dev, op, w_alt, w_ref, n_cols):
    """One ``vtx_csr_dense_sum`` -> an int64 tensor of n_major x n_cols.  The tables are int32 tensors on ``dev``, C-contiguous."""
    csr, n_major, n_minor, _ = op
    out = torch.empty((n_major, n_cols), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)              # the library works on its own stream: torch's writes to the tables have to be done
    ctx.csr_dense_sum(n_major, n_minor, int(csr["indices"].shape[0]), csr["indptr"].data_ptr(), csr["indices"].data_ptr(), csr["alt"].data_ptr(),
                      csr["ref"].data_ptr(), 0 if w_alt is None else w_alt.data_ptr(), 0 if w_ref is None else w_ref.data_ptr(), n_cols, out.data_ptr())
    return out


def _bare_context(torch, dev, n_cell):
    index = torch.cuda.current_device() if dev.index is None else dev.index
    return lib.Context(abi.default_config(n_barcodes=max(n_cell, 1), device=index))      # no batch, no run: device, stream, work space


def weighted_sum(result: Result, w_alt=None, w_ref=None, *, over="cells", to=None):
    """The integer part of every likelihood that depends on the variant through more than a genotype class — a free alt probability
    per (variant, cluster), an ambient profile, an unequal mixture: with ``over="cells"``, per cell c and column h,

        out[c, h] = sum over the cell's entries (c, v) of  alt[c, v] * w_alt[v, h] + ref[c, v] * w_ref[v, h]

    from tables of ``len(result.variants)`` x n_cols; with ``over="variants"`` the same per variant, from tables of
    ``len(result.barcodes)`` x n_cols.  The tables are int32 (fixed-point: ``rint(SCORE_SCALE * log p)``, say), numpy or torch; one
    of them may be ``None`` and its term is then absent.  -> int64, cells (variants) x n_cols.

    A torch result is summed on its device — one ``vtx_csr_dense_sum`` on a bare context for that device (at most
    ``abi.CSR_DENSE_MAX`` columns, fewer than 2^32 entries), after one ``vtx_csr_transpose`` of the alt and ref counts when the result's
    rows are not what ``over`` names — into a tensor, or into a numpy array with ``to="scipy"``; a scipy result is summed on the host
    in int64.  Zero columns give an empty array without a library call.  The library's sum wraps modulo 2^64; this raises
    ``ValueError`` when ``max|w|`` times the alt + ref reads of the largest row reaches 2^63, so what it returns never wrapped.

    ``cluster_donors`` is built from this; ambient RNA and unequal mixtures are a matter of other tables and are not built here."""
    if over not in ("cells", "variants"):
        raise ValueError("weighted_sum: over %r: cells or variants" % (over,))
    if to not in (None, "scipy", "torch"):
        raise ValueError("to %r: scipy, torch, or None for the container of the result" % (to,))
    if w_alt is None and w_ref is None:
        raise ValueError("weighted_sum: w_alt, w_ref or both")
    n_var, n_cell = len(result.variants), len(result.barcodes)
    n_rows, n_table = (n_cell, n_var) if over == "cells" else (n_var, n_cell)
    on_device = _is_torch(result.alt_counts)
    if not on_device and to == "torch":
        raise ValueError("weighted_sum: a scipy result is summed on the host; to=\"torch\" needs a torch result (run(to=\"torch\"))")
    torch = dev = None
    if on_device:
        import torch
        dev = result.alt_counts.device
    w_alt, w_ref = _dense_table(w_alt, n_table, "w_alt", torch, dev), _dense_table(w_ref, n_table, "w_ref", torch, dev)
    n_cols = int((w_alt if w_alt is not None else w_ref).shape[1])
    if w_alt is not None and w_ref is not None and tuple(w_alt.shape) != tuple(w_ref.shape):
        raise ValueError("weighted_sum: w_alt of shape %s and w_ref of shape %s" % (tuple(w_alt.shape), tuple(w_ref.shape)))
    if not on_device:
        if not n_cols:
            return np.zeros((n_rows, 0), np.int64)
        op, rows = _dense_operand_host(result, over)
        _dense_guard(w_alt, w_ref, int(rows.max()) if len(rows) else 0)
        return _dense_sum_host(op, w_alt, w_ref, n_cols)
    if not n_cols:                               # nothing to sum, and the library takes no table without columns
        out = torch.zeros((n_rows, 0), dtype=torch.int64, device=dev)
    else:
        if n_cols > abi.CSR_DENSE_MAX:
            raise ValueError("weighted_sum: %d columns: at most %d" % (n_cols, abi.CSR_DENSE_MAX))
        with _bare_context(torch, dev, n_cell) as ctx:
            op = _dense_operands_device(ctx, torch, dev, result, (over,))[over]
            _dense_guard(w_alt, w_ref, int(op[3].max()) if n_rows else 0)
            out = _dense_sum_device(ctx, torch, dev, op, w_alt, w_ref, n_cols)
    return out.cpu().numpy() if to == "scipy" else out


def _m_step_tables(A, R, prior):
    """The M-step's floating point, float64 in numpy or in torch (on the tensors' device), from the exact weighted reads A and R (int64,
    variants x k): theta = (A / Q + prior[0]) / ((A + R) / Q + prior[0] + prior[1]), and the int32 tables rint(S log theta), rint(S
    log1p(-theta)).  -> (theta, w_alt, w_ref)"""
    q, s = float(RESP_SCALE), float(SCORE_SCALE)
    if _is_torch(A):
        import torch
        theta = (A.to(torch.float64) / q + prior[0]) / ((A + R).to(torch.float64) / q + (prior[0] + prior[1]))
        return theta, torch.round(s * torch.log(theta)).to(torch.int32), torch.round(s * torch.log1p(-theta)).to(torch.int32)
    theta = (A.astype(np.float64) / q + prior[0]) / ((A + R).astype(np.float64) / q + (prior[0] + prior[1]))
    return theta, np.rint(s * np.log(theta)).astype(np.int32), np.rint(s * np.log1p(-theta)).astype(np.int32)


def _e_step_resp(score, live):
    """The E-step's floating point: rq' = rint(Q softmax(score / S)) per live cell (the row maximum subtracted first), 0 for the
    others, and the log-likelihood sum over the live cells of logsumexp(score / S).  -> (rq' int32, log_lik float)"""
    q, s = float(RESP_SCALE), float(SCORE_SCALE)
    if _is_torch(score):
        import torch
        x = score.to(torch.float64) / s
        top = x.max(dim=1, keepdim=True).values
        e = torch.exp(x - top)
        total = e.sum(dim=1, keepdim=True)
        rq = torch.round(q * (e / total)).to(torch.int32) * live.to(torch.int32)[:, None]
        return rq, float(((top + torch.log(total))[:, 0] * live.to(torch.float64)).sum())
    x = score.astype(np.float64) / s
    top = x.max(axis=1, keepdims=True)
    e = np.exp(x - top)
    total = e.sum(axis=1, keepdims=True)
    rq = np.rint(q * (e / total)).astype(np.int32) * live.astype(np.int32)[:, None]
    return rq, float(((top + np.log(total))[:, 0] * live.astype(np.float64)).sum())


def cluster_donors(result: Result, k, *, n_init=8, max_iter=100, tol=2 ** -10, prior=(1.0, 1.0), seed=0, to=None) -> DonorClusters:
    """Cluster the cells of a pool by donor WITHOUT genotypes (souporcell's and vireo's default mode): a soft EM over a free alt
    probability ``theta`` per (variant, cluster), whose integer parts are two ``weighted_sum``s.  With ``S = SCORE_SCALE`` and ``Q =
    RESP_SCALE``:

    A cell is live when it has an entry with ``alt + ref > 0``; the others keep responsibilities 0 and the label -1.  Restart ``t`` of
    ``n_init`` draws ``lab = np.random.default_rng([seed, t]).integers(0, k, n_cells)`` for all cells in barcode order and sets ``rq[c,
    lab[c]] = Q`` for the live ones (``rq``: int32, cells x k).  A round is

        A = weighted_sum(w_alt=rq, over="variants");  R = weighted_sum(w_ref=rq, over="variants")              exact int64
        theta = (A / Q + prior[0]) / ((A + R) / Q + prior[0] + prior[1])                                      float64
        w_alt = rint(S * log(theta));  w_ref = rint(S * log1p(-theta))                                        int32
        score = weighted_sum(w_alt, w_ref, over="cells")                                                      exact int64
        rq' = rint(Q * softmax(score / S)) per live cell, the row maximum subtracted first                    int32

    and the restart stops when ``max |rq' - rq| <= tol * Q``, or after ``max_iter`` rounds.  ``log_lik`` is the sum over the live
    cells of ``logsumexp(score / S)``; the restart with the highest wins, the lowest ``t`` on a tie.  ``labels`` is the argmax of the
    winner's ``score``, the lowest cluster on a tie, and is accepted as ``groups`` by ``pseudobulk`` (the cells without a read form
    the group -1).

    On a torch result the sums are ``vtx_csr_dense_sum`` calls on one bare context, after one ``vtx_csr_transpose``, and the floating
    point between them is torch float64 on the device: the CSR, the tables and the scores never leave it between rounds (one number,
    the convergence test, does).  On a scipy result everything is numpy.  The integer sums are exact either way; the float64 steps of
    the two may differ in the last bit, and with them a table entry by one unit.  -> ``DonorClusters`` of tensors, or of numpy arrays
    for a scipy result and with ``to="scipy"``.

    ``k`` must lie in 1 .. 64.  Out of scope: ambient RNA and unequal mixtures (other tables for ``weighted_sum``), more than 64
    clusters, several GPUs."""
    if int(k) != k or k < 1:
        raise ValueError("cluster_donors: k %r: at least one cluster" % (k,))
    if k > CLUSTER_MAX:
        raise ValueError("cluster_donors: %d clusters: at most %d (theta is a dense variants x k table)" % (k, CLUSTER_MAX))
    k = int(k)
    if n_init < 1 or max_iter < 1:
        raise ValueError("cluster_donors: n_init %r, max_iter %r: at least one restart and one round" % (n_init, max_iter))
    prior = (float(prior[0]), float(prior[1]))
    if not (prior[0] > 0.0 and prior[1] > 0.0):
        raise ValueError("cluster_donors: prior %r: two positive pseudo-counts" % (prior,))
    if to not in (None, "scipy", "torch"):
        raise ValueError("to %r: scipy, torch, or None for the container of the result" % (to,))
    on_device = _is_torch(result.alt_counts)
    if not on_device and to == "torch":
        raise ValueError("cluster_donors: a scipy result is clustered on the host; to=\"torch\" needs a torch result (run(to=\"torch\"))")
    n_var, n_cell = len(result.variants), len(result.barcodes)

    def em(sum_over, as_table, live):
        """Every restart: sum_over(over, w_alt, w_ref) is the guarded sum, as_table(numpy int32) an array where the sums run, ``live``
        the live cells there.  -> the winner's state"""
        live_host = np.asarray(live.cpu() if _is_torch(live) else live)
        best = None
        for t in range(int(n_init)):
            lab = np.random.default_rng([seed, t]).integers(0, k, n_cell)
            first = np.zeros((n_cell, k), np.int32)
            first[np.arange(n_cell), lab] = RESP_SCALE
            rq = as_table(first * live_host.astype(np.int32)[:, None])
            converged = False
            for n_iter in range(1, int(max_iter) + 1):
                A, R = sum_over("variants", rq, None), sum_over("variants", None, rq)
                theta, w_alt, w_ref = _m_step_tables(A, R, prior)
                score = sum_over("cells", w_alt, w_ref)
                new, log_lik = _e_step_resp(score, live)
                delta = int(abs(new - rq).max()) if n_cell else 0
                rq = new
                if delta <= tol * RESP_SCALE:
                    converged = True
                    break
            if best is None or log_lik > best["log_lik"]:
                best = dict(rq=rq, score=score, theta=theta, w_alt=w_alt, w_ref=w_ref, log_lik=log_lik, n_iter=n_iter, converged=converged, restart=t)
        return best

    if on_device:
        import torch
        dev = result.alt_counts.device
        with _bare_context(torch, dev, n_cell) as ctx:
            ops = _dense_operands_device(ctx, torch, dev, result, ("cells", "variants"))
            most = {over: int(op[3].max()) if op[1] else 0 for over, op in ops.items()}
            live = ops["cells"][3] > 0

            def sum_over(over, w_alt, w_ref):
                _dense_guard(w_alt, w_ref, most[over])
                w_alt, w_ref = (None if w is None else w.contiguous() for w in (w_alt, w_ref))
                return _dense_sum_device(ctx, torch, dev, ops[over], w_alt, w_ref, k)
            best = em(sum_over, lambda a: torch.from_numpy(a).to(dev), live)
        score = best["score"]
        ranks = torch.arange(k, dtype=torch.int64, device=dev)[None, :].expand(n_cell, k)
        labels = torch.where(score == score.max(dim=1, keepdim=True).values, ranks, k).min(dim=1).values      # the lowest index on a tie
        labels = torch.where(live, labels, -1)
        resp = best["rq"].to(torch.float64) / float(RESP_SCALE)
        fields = dict(labels=labels, resp=resp, score=score, theta=best["theta"], w_alt=best["w_alt"], w_ref=best["w_ref"])
        if to == "scipy":
            fields = {f: v.cpu().numpy() for f, v in fields.items()}
    else:
        ops = {over: _dense_operand_host(result, over) for over in ("cells", "variants")}
        most = {over: int(rows.max()) if len(rows) else 0 for over, (_, rows) in ops.items()}
        live = ops["cells"][1] > 0

        def sum_over(over, w_alt, w_ref):
            _dense_guard(w_alt, w_ref, most[over])
            return _dense_sum_host(ops[over][0], w_alt, w_ref, k)
        best = em(sum_over, lambda a: a, live)
        labels = np.where(live, np.argmax(best["score"], axis=1), -1).astype(np.int64)
        fields = dict(labels=labels, resp=best["rq"].astype(np.float64) / float(RESP_SCALE), score=best["score"], theta=best["theta"],
                      w_alt=best["w_alt"], w_ref=best["w_ref"])
    return DonorClusters(**fields, log_lik=best["log_lik"], n_iter=best["n_iter"], converged=best["converged"], restart=best["restart"],
                         barcodes=list(result.barcodes), variants=list(result.variants))
