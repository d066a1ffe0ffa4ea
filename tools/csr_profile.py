"""What it costs to get the matrices of a run OUT as CSR, on the synthetic config-3 batch bench.py uses (vartrix_amd.synth: 100 000
loci x 10 000 barcodes x 256 reads per locus, consensus): the two device calls of this library against what a user does today, all in
ONE process, each entry the median of --runs repetitions after one warm-up.
  device_csr            vtx_device_csr alone (the row offsets; the other arrays are the run's own)           device events by phase + host wall
  csr_transpose         vtx_csr_transpose of that CSR with the five payload arrays, into torch buffers        device events by phase + host wall
  fetch_coo_to_csr      today, without a file: fetch_coo + scipy.sparse.coo_matrix(...).tocsr()               host wall
  fetch_coo_to_csr_T    ... and .T.tocsr() for the cells x variants orientation (one data array, not five)    host wall
  write_mtx_mmread      today, through the file: vtx_write_mtx, then scipy.io.mmread(...).tocsr()             host wall
The device times are the library's own (vtx_last_csr_ms: events on the context's stream around the check of the inputs, the sort, the
offsets and the placement); the host wall time is what a caller waits, the readback of the check's flag word included.  The results of
the device calls are compared with scipy's before anything is timed.
GPU box:   python tools/csr_profile.py --json profiles/r12_csr.json

--ops measures the summaries and selections of that CSR instead (vtx_csr_row_stats variant-major and cell-major, vtx_csr_select_plan and
vtx_csr_select keeping the variants with n_alt >= 10 and n_ref >= 10, all five payloads), each compared with numpy / scipy before it is
timed, against what a user does today: on the device in torch (CSR -> COO rows, index_add_, boolean masking, offsets from a bincount —
each reported only if this torch build can do it, with the error otherwise), and on the host (fetch + numpy / scipy).  It also records
which operations this torch build offers on a sparse CSR tensor.
--sweep times the statistics kernel at every group size G (the developer library's VTX_CSR_STATS_G, so VTX_LIB_VARIANT=dev) on synthetic
CSRs of three shapes — config 3 variant-major and cell-major, and four reads per locus — next to the G the rule picks; no batch is run.
GPU box:   python tools/csr_profile.py --ops --json profiles/r13_csr_ops.json
           VTX_LIB_VARIANT=dev python tools/csr_profile.py --sweep --json profiles/r13_csr_ops.json     (joins the record above)

--group measures the pseudobulk fold (vtx_csr_group_plan + vtx_csr_group_sum) on synthetic CSRs of config 3's shape in both orientations
(Poisson row lengths, uniform random columns and labels; no batch is run) at n_groups = 8, 64, W and 4 W, each result compared with a
numpy model before it is timed, next to (a) vtx_csr_row_stats on the same CSR — the floor: the same bytes without the gather —, (b) torch
on the device (rows by repeat_interleave, key = row * n_groups + label, seven index_add_ into a dense buffer) and (c) the host (the
arrays copied out, scipy A @ one-hot).
GPU box:   python tools/csr_profile.py --group --json profiles/r14_csr_group.json

--geno measures the donor tally (vtx_csr_geno_tally) on the synthetic CSR of config 3's cell-major shape (the generator --group uses) with
a random genotype table of 8 and of 64 donors, each result compared with a numpy model before it is timed, next to (a) vtx_csr_row_stats
on the same CSR — the same bytes without the gather — and (b) torch on the device (rows by repeat_interleave, a gather of the genotype
rows, three index_add_ into a dense buffer).
GPU box:   python tools/csr_profile.py --geno --json profiles/r22_csr_geno.json

--pairs measures the doublet tally (vtx_csr_geno_pair_tally) on --geno's CSR and table at 8 donors (all 28 pairs), 16 donors (all 120) and
64 donors (a list of 64 pairs), each result compared with a numpy model before it is timed, next to (a) vtx_csr_geno_tally on the same CSR
and table — the cost of a (entry, donor) slot against that of a (entry, pair) slot — and (b) torch on the device (rows by
repeat_interleave, per pair two gathered genotype columns, the dosage, three index_add_ into a dense buffer of the output's size).
GPU box:   python tools/csr_profile.py --pairs --json profiles/r25_csr_geno_pair.json

--dense measures the CSR x integer-table sum (vtx_csr_dense_sum) on --geno's CSR and on its transpose at 8, 16 and 64 columns — the call
with both tables (the E-step's shape) and the two single-table calls (the M-step's) — each result compared with a float64 matmul on the
host before it is timed, next to (b) torch on the device: two torch.sparse.mm of float64 CSR copies against float64 tables (or, where this
build has no device CSR x dense product, --geno's gather + index_add_ form; the record says which).  It ends with one whole
api.cluster_donors at that shape with k = 8 and one restart.
GPU box:   python tools/csr_profile.py --dense --json profiles/r27_csr_dense.json"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import scipy.io  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

from vartrix_amd import api, lib, synth  # noqa: E402
from vartrix_amd.abi import default_config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", required=True)
ap.add_argument("--loci", type=int, default=100_000)
ap.add_argument("--barcodes", type=int, default=10_000)
ap.add_argument("--reads-per-locus", type=int, default=256)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--skip-mmread", action="store_true", help="leave out the Matrix-Market round trip (minutes of parsing at config-3 size)")
ap.add_argument("--ops", action="store_true", help="measure vtx_csr_row_stats / vtx_csr_select instead of the hand-over")
ap.add_argument("--sweep", action="store_true", help="time csr_row_stats_kernel at every group size (developer library), no batch")
ap.add_argument("--group", action="store_true", help="measure vtx_csr_group_plan / vtx_csr_group_sum on synthetic CSRs, no batch")
ap.add_argument("--geno", action="store_true", help="measure vtx_csr_geno_tally on a synthetic cell-major CSR, no batch")
ap.add_argument("--pairs", action="store_true", help="measure vtx_csr_geno_pair_tally on --geno's synthetic cell-major CSR, no batch")
ap.add_argument("--dense", action="store_true", help="measure vtx_csr_dense_sum on --geno's synthetic CSR in both orientations, no batch")
args = ap.parse_args()

dev = torch.device("cuda", 0)


def timed(fn):
    """(host wall ms, result) of one call; every call timed here ends in a synchronise of its own."""
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def series(fn, phases=None):
    """phases: a callable that returns the device times of the call just made (Context.csr_ms: events on the context's stream)."""
    timed(fn)                                                    # warm-up: buffers of the context, page cache, allocator
    walls, devs = [], []
    for _ in range(args.runs):
        w, _ = timed(fn)
        walls.append(round(w, 3))
        if phases:
            devs.append({k: round(v, 4) for k, v in phases().items()})
    one = {"host_wall_ms": walls, "host_wall_ms_median": statistics.median(walls)}
    if phases:
        one["device_ms_by_phase"] = devs
        one["device_ms_by_phase_median"] = {k: statistics.median(d[k] for d in devs) for k in devs[0]}
        one["device_ms"] = [round(sum(d.values()), 4) for d in devs]
        one["device_ms_median"] = statistics.median(one["device_ms"])
    return one


def finish(res):
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    if args.sweep and os.path.exists(args.json):                 # the sweep joins the --ops record it belongs to
        whole = json.load(open(args.json))
        whole["group_size_sweep"] = res
        res = whole
    json.dump(res, open(args.json, "w"), indent=1)


def stats_buffers(n):
    from vartrix_amd import abi
    return {k: torch.empty(n, dtype=torch.int32 if k in abi.CSR_STAT_COUNTS else torch.int64, device=dev) for k in abi.CSR_STAT_NAMES}


def stats_call(ctx, csr, n_major, n_minor, out):
    nnz = int(csr["indices"].shape[0])
    return lambda: ctx.csr_row_stats(n_major, n_minor, nnz, csr["indptr"].data_ptr(), csr["indices"].data_ptr(), csr["alt"].data_ptr(),
                                     csr["ref"].data_ptr(), csr["unk"].data_ptr(), {k: v.data_ptr() for k, v in out.items()})


def host_stats(indptr, alt, ref, unk):
    """numpy's seven statistics of every row (counts by bincount, sums by add.reduceat in uint64)."""
    n, lens = len(indptr) - 1, np.diff(indptr)
    rows, full = np.repeat(np.arange(n), lens), lens > 0

    def total(a):
        o = np.zeros(n, np.uint64)
        o[full] = np.add.reduceat(a.astype(np.uint64), indptr[:-1][full])
        return o
    return {"n_entries": lens, "n_alt": np.bincount(rows[alt > 0], minlength=n), "n_ref": np.bincount(rows[ref > 0], minlength=n),
            "n_both": np.bincount(rows[(alt > 0) & (ref > 0)], minlength=n), "sum_alt": total(alt), "sum_ref": total(ref), "sum_unk": total(unk)}


def same_stats(out, want):
    for k, v in want.items():
        got = out[k].cpu().numpy()
        got = got.view(np.uint32) if got.dtype == np.int32 else got.view(np.uint64)
        assert np.array_equal(got.astype(np.uint64), v.astype(np.uint64)), k


if args.sweep:
    if lib.DEFAULT_VARIANT != "dev":
        sys.exit("--sweep needs the developer library: VTX_LIB_VARIANT=dev")
    # mean row lengths: 23.92 M entries (config 3) and 378 345 (4 reads per locus, profiles/r06_depth_noise.jsonl) over 100 000 x 10 000
    shapes = {"config3_variant_major": (args.loci, args.barcodes, 239.23), "config3_cell_major": (args.barcodes, args.loci, 2392.3),
              "four_reads_per_locus_variant_major": (args.loci, args.barcodes, 3.78), "four_reads_per_locus_cell_major": (args.barcodes, args.loci, 37.8)}
    res = {"what": "csr_row_stats_kernel<G> at every G (tools/csr_profile.py --sweep): device ms of the reduction (vtx_last_csr_ms[3]), median of "
                   "%d after one warm-up; synthetic CSRs with Poisson row lengths" % args.runs, "shapes": {}}
    gen = torch.Generator(device=dev).manual_seed(7)
    with lib.Context(default_config(n_barcodes=4)) as ctx:
        for name, (n_major, n_minor, mean) in shapes.items():
            lens = torch.poisson(torch.full((n_major,), mean, device=dev), generator=gen).clamp_(max=n_minor).to(torch.int64)
            indptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
            nnz = int(indptr[-1])
            csr = {"indptr": indptr, "indices": torch.zeros(nnz, dtype=torch.int32, device=dev)}       # read by the check only
            for k in ("alt", "ref", "unk"):
                csr[k] = torch.randint(0, 3, (nnz,), dtype=torch.int32, device=dev, generator=gen)
            out = stats_buffers(n_major)
            call = stats_call(ctx, csr, n_major, n_minor, out)
            want = host_stats(indptr.cpu().numpy(), *[csr[k].cpu().numpy() for k in ("alt", "ref", "unk")])
            one = {"n_major": n_major, "n_minor": n_minor, "nnz": nnz, "reduction_ms_by_G": {}}
            for G in ("rule", 1, 2, 4, 8, 16, 32, 64):
                if G == "rule":
                    os.environ.pop("VTX_CSR_STATS_G", None)
                else:
                    os.environ["VTX_CSR_STATS_G"] = str(G)
                for v in out.values():
                    v.fill_(-1)
                torch.cuda.synchronize(dev)
                call()
                same_stats(out, want)                            # every G gives numpy's answer before it is timed
                one["reduction_ms_by_G"][str(G)] = series(call, ctx.csr_ms)["device_ms_by_phase_median"]["place"]
                print(name, "G", G, one["reduction_ms_by_G"][str(G)], flush=True)
            os.environ.pop("VTX_CSR_STATS_G", None)
            res["shapes"][name] = one
            del csr, out
    finish(res)
    sys.exit(0)

if args.group:
    from vartrix_amd import abi
    W = lib.load().vtx_csr_group_window()
    shapes = {"config3_variant_major": (args.loci, args.barcodes, 239.23), "config3_cell_major": (args.barcodes, args.loci, 2392.3)}
    res = {"what": "vtx_csr_group_plan + vtx_csr_group_sum (tools/csr_profile.py --group): median of %d after one warm-up, one process; synthetic "
                   "CSRs with Poisson row lengths, uniform random columns and labels; device ms by phase from vtx_last_csr_ms" % args.runs,
           "window": W, "group_max": lib.load().vtx_csr_group_max(), "shapes": {}}
    gen = torch.Generator(device=dev).manual_seed(11)

    def model(indptr, indices, counts, label, n_groups):
        """numpy: the kept entries sorted by (row, group), add.reduceat in uint64 -> (offsets, groups, the seven arrays)."""
        rows = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
        key = rows * n_groups + label[indices]
        order = np.argsort(key, kind="stable")
        key = key[order]
        starts = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
        a, r, u = (c[order] for c in counts)
        cols = [np.ones(len(key), np.uint64), a > 0, r > 0, (a > 0) & (r > 0), a, r, u]
        return (np.searchsorted(key[starts] // n_groups, np.arange(len(indptr))), key[starts] % n_groups,
                [np.add.reduceat(c.astype(np.uint64), starts) for c in cols])

    with lib.Context(default_config(n_barcodes=4)) as ctx:
        for name, (n_major, n_minor, mean) in shapes.items():
            lens = torch.poisson(torch.full((n_major,), mean, device=dev), generator=gen).clamp_(max=n_minor).to(torch.int64)
            indptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
            nnz = int(indptr[-1])
            csr = {"indptr": indptr, "indices": torch.randint(0, n_minor, (nnz,), dtype=torch.int32, device=dev, generator=gen)}
            for k in ("alt", "ref", "unk"):
                csr[k] = torch.randint(0, 3, (nnz,), dtype=torch.int32, device=dev, generator=gen)
            host = {k: v.cpu().numpy() for k, v in csr.items()}
            one = {"n_major": n_major, "n_minor": n_minor, "nnz": nnz, "n_groups": {}}
            floor_out = stats_buffers(n_major)
            one["row_stats_floor"] = series(stats_call(ctx, csr, n_major, n_minor, floor_out), ctx.csr_ms)
            head = (n_major, n_minor, nnz, csr["indptr"].data_ptr(), csr["indices"].data_ptr())
            for n_groups in (8, 64, W, 4 * W):
                label = torch.randint(0, n_groups, (n_minor,), dtype=torch.int32, device=dev, generator=gen)
                torch.cuda.synchronize(dev)
                n_out = ctx.csr_group_plan(*head, label.data_ptr(), n_groups)
                out = {"indptr": torch.empty(n_major + 1, dtype=torch.int64, device=dev), "indices": torch.empty(n_out, dtype=torch.int32, device=dev)}
                out.update(stats_buffers(n_out))
                torch.cuda.synchronize(dev)

                def sum_call():
                    return ctx.csr_group_sum(*head, csr["alt"].data_ptr(), csr["ref"].data_ptr(), csr["unk"].data_ptr(), label.data_ptr(), n_groups, n_out,
                                             out["indptr"].data_ptr(), out["indices"].data_ptr(), {k: out[k].data_ptr() for k in abi.CSR_STAT_NAMES})
                sum_call()
                # ---- correctness first ----
                w_ptr, w_idx, w_cols = model(host["indptr"], host["indices"], [host[k] for k in ("alt", "ref", "unk")], label.cpu().numpy().astype(np.int64), n_groups)
                assert n_out == len(w_idx) and np.array_equal(out["indptr"].cpu().numpy(), w_ptr) and np.array_equal(out["indices"].cpu().numpy(), w_idx)
                same_stats(out, dict(zip(abi.CSR_STAT_NAMES, w_cols)))
                print("%s n_groups %d: equals the numpy model, %d entries" % (name, n_groups, n_out), flush=True)
                E = {"nnz_out": n_out}
                E["group_plan"] = series(lambda: ctx.csr_group_plan(*head, label.data_ptr(), n_groups), ctx.csr_ms)
                E["group_sum"] = series(sum_call, ctx.csr_ms)

                def torch_fold():
                    rows = torch.repeat_interleave(torch.arange(n_major, device=dev), csr["indptr"][1:] - csr["indptr"][:-1])
                    key = rows * n_groups + label[csr["indices"].to(torch.int64)].to(torch.int64)
                    a, r, u = csr["alt"], csr["ref"], csr["unk"]
                    o = [torch.zeros(n_major * n_groups, dtype=torch.int64, device=dev).index_add_(0, key, w.to(torch.int64))
                         for w in (torch.ones_like(a), a > 0, r > 0, (a > 0) & (r > 0), a, r, u)]
                    torch.cuda.synchronize(dev)
                    return o

                def host_fold():
                    h = {k: v.cpu().numpy() for k, v in csr.items()}
                    lab = label.cpu().numpy().astype(np.int64)
                    onehot = sp.csr_matrix((np.ones(n_minor, np.int64), (np.arange(n_minor), lab)), shape=(n_minor, n_groups))
                    mats = [sp.csr_matrix((d.astype(np.int64), h["indices"], h["indptr"]), shape=(n_major, n_minor))
                            for d in (np.ones(nnz), h["alt"] > 0, h["ref"] > 0, (h["alt"] > 0) & (h["ref"] > 0), h["alt"], h["ref"], h["unk"])]
                    return [m @ onehot for m in mats]
                try:
                    dense = torch_fold()
                    rows_out = torch.repeat_interleave(torch.arange(n_major, device=dev), out["indptr"][1:] - out["indptr"][:-1])
                    at = rows_out * n_groups + out["indices"].to(torch.int64)
                    for d, k in zip(dense, abi.CSR_STAT_NAMES):
                        assert torch.equal(d[at], out[k].to(torch.int64) & (0xFFFFFFFF if k in abi.CSR_STAT_COUNTS else -1)), k
                    del dense, rows_out, at
                    E["torch_index_add_dense"] = series(torch_fold)
                except Exception as e:                           # noqa: BLE001  (the record IS the error)
                    E["torch_index_add_dense"] = {"error": "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200] if str(e) else "")}
                if n_groups == W:                                # the host does not care much how many groups there are: one point
                    E["host_copy_scipy_onehot"] = series(host_fold)
                one["n_groups"][str(n_groups)] = E
                print(name, n_groups, "plan", E["group_plan"]["device_ms_by_phase_median"], "sum", E["group_sum"]["device_ms_by_phase_median"],
                      "torch", E["torch_index_add_dense"].get("host_wall_ms_median"), flush=True)
                del out, label
            res["shapes"][name] = one
            del csr, host, floor_out
    finish(res)
    sys.exit(0)

if args.geno:
    from vartrix_amd import abi
    n_major, n_minor, mean = args.barcodes, args.loci, 2392.3 * args.loci / 100_000
    res = {"what": "vtx_csr_geno_tally (tools/csr_profile.py --geno): median of %d after one warm-up, one process; a synthetic cell-major CSR "
                   "with Poisson row lengths and uniform random columns, a random genotype table (classes 0 / 1 / 2 / missing at 35 / 30 / 20 / "
                   "15 %%); device ms by phase from vtx_last_csr_ms" % args.runs, "geno_max": lib.load().vtx_csr_geno_max(), "n_donors": {}}
    gen = torch.Generator(device=dev).manual_seed(11)
    byte_of = torch.tensor([0, 1, 2, abi.VTX_GENO_NONE], dtype=torch.uint8, device=dev)
    with lib.Context(default_config(n_barcodes=4)) as ctx:
        lens = torch.poisson(torch.full((n_major,), mean, device=dev), generator=gen).clamp_(max=n_minor).to(torch.int64)
        indptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
        nnz = int(indptr[-1])
        csr = {"indptr": indptr, "indices": torch.randint(0, n_minor, (nnz,), dtype=torch.int32, device=dev, generator=gen)}
        for k in ("alt", "ref", "unk"):
            csr[k] = torch.randint(0, 3, (nnz,), dtype=torch.int32, device=dev, generator=gen)
        host = {k: v.cpu().numpy() for k, v in csr.items()}
        rows_host = np.repeat(np.arange(n_major, dtype=np.int64), np.diff(host["indptr"]))
        res.update({"n_major": n_major, "n_minor": n_minor, "nnz": nnz})
        floor_out = stats_buffers(n_major)
        res["row_stats_floor"] = series(stats_call(ctx, csr, n_major, n_minor, floor_out), ctx.csr_ms)
        for n_donors in (8, 64):
            cls = torch.multinomial(torch.tensor([0.35, 0.3, 0.2, 0.15], device=dev), n_minor * n_donors, replacement=True, generator=gen)
            table = byte_of[cls].reshape(n_minor, n_donors).contiguous()
            n = n_major * n_donors * 4
            out = {"sum_alt": torch.empty(n, dtype=torch.int64, device=dev), "sum_ref": torch.empty(n, dtype=torch.int64, device=dev),
                   "n_obs": torch.empty(n, dtype=torch.int32, device=dev)}
            torch.cuda.synchronize(dev)

            def tally_call():
                return ctx.csr_geno_tally(n_major, n_minor, nnz, csr["indptr"].data_ptr(), csr["indices"].data_ptr(), csr["alt"].data_ptr(),
                                          csr["ref"].data_ptr(), table.data_ptr(), n_donors, {k: v.data_ptr() for k, v in out.items()})
            tally_call()
            # ---- correctness first: per donor, numpy's bincount over (row, class) with the counts as weights (exact: sums far below 2^53) ----
            got = {k: v.cpu().numpy().reshape(n_major, n_donors, 4) for k, v in out.items()}
            cls_host = cls.reshape(n_minor, n_donors).cpu().numpy()
            seen = ((host["alt"] + host["ref"]) > 0).astype(np.float64)
            for d in range(n_donors):
                key = rows_host * 4 + cls_host[host["indices"], d]
                for k, w in (("sum_alt", host["alt"]), ("sum_ref", host["ref"]), ("n_obs", seen)):
                    want = np.bincount(key, weights=w, minlength=n_major * 4).astype(np.int64).reshape(n_major, 4)
                    assert np.array_equal(got[k][:, d].astype(np.int64), want), (n_donors, d, k)
            print("n_donors %d: equals the numpy model" % n_donors, flush=True)
            E = {"geno_tally": series(tally_call, ctx.csr_ms)}

            def torch_tally():
                rows = torch.repeat_interleave(torch.arange(n_major, device=dev), csr["indptr"][1:] - csr["indptr"][:-1])
                g = table[csr["indices"].to(torch.int64)].to(torch.int64)                  # nnz x n_donors: the gather of the genotype rows
                g = torch.where(g == abi.VTX_GENO_NONE, 3, g)
                key = ((rows[:, None] * n_donors + torch.arange(n_donors, device=dev)) * 4 + g).reshape(-1)
                a, r = csr["alt"].to(torch.int64), csr["ref"].to(torch.int64)
                o = [torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, key, w[:, None].expand(nnz, n_donors).reshape(-1))
                     for w in (a, r, ((a + r) > 0).to(torch.int64))]
                torch.cuda.synchronize(dev)
                return o
            try:
                dense = torch_tally()
                for d, k in zip(dense, abi.GENO_TALLY_NAMES):
                    assert torch.equal(d, out[k].to(torch.int64)), k
                del dense
                E["torch_gather_index_add_dense"] = series(torch_tally)
            except Exception as e:                               # noqa: BLE001  (the record IS the error)
                E["torch_gather_index_add_dense"] = {"error": "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200] if str(e) else "")}
            res["n_donors"][str(n_donors)] = E
            print(n_donors, "tally", E["geno_tally"]["device_ms_by_phase_median"], "wall", E["geno_tally"]["host_wall_ms_median"], "torch",
                  E["torch_gather_index_add_dense"].get("host_wall_ms_median", E["torch_gather_index_add_dense"].get("error")), flush=True)
            del out, table, cls
    finish(res)
    sys.exit(0)

if args.pairs:
    from concurrent.futures import ThreadPoolExecutor
    from vartrix_amd import abi
    C6 = abi.GENO_PAIR_CLASSES
    n_major, n_minor, mean = args.barcodes, args.loci, 2392.3 * args.loci / 100_000
    res = {"what": "vtx_csr_geno_pair_tally (tools/csr_profile.py --pairs): median of %d after one warm-up, one process; --geno's synthetic "
                   "cell-major CSR (Poisson row lengths, uniform random columns) and random genotype table (classes 0 / 1 / 2 / missing at 35 / "
                   "30 / 20 / 15 %%); device ms by phase from vtx_last_csr_ms" % args.runs, "geno_pair_max": lib.load().vtx_csr_geno_pair_max(),
           "sizes": {}}
    gen = torch.Generator(device=dev).manual_seed(11)
    byte_of = torch.tensor([0, 1, 2, abi.VTX_GENO_NONE], dtype=torch.uint8, device=dev)
    with lib.Context(default_config(n_barcodes=4)) as ctx:
        lens = torch.poisson(torch.full((n_major,), mean, device=dev), generator=gen).clamp_(max=n_minor).to(torch.int64)
        indptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
        nnz = int(indptr[-1])
        csr = {"indptr": indptr, "indices": torch.randint(0, n_minor, (nnz,), dtype=torch.int32, device=dev, generator=gen)}
        for k in ("alt", "ref", "unk"):
            csr[k] = torch.randint(0, 3, (nnz,), dtype=torch.int32, device=dev, generator=gen)
        host = {k: v.cpu().numpy() for k, v in csr.items()}
        rows_host = np.repeat(np.arange(n_major, dtype=np.int64), np.diff(host["indptr"]))
        # the three numbers of an entry in one float64 weight: every (row, class) sum of each stays below 2^17, the whole below 2^53
        assert int(np.diff(host["indptr"]).max()) * 2 < 1 << 17
        packed = (host["alt"].astype(np.int64) + (host["ref"].astype(np.int64) << 17)
                  + (((host["alt"] + host["ref"]) > 0).astype(np.int64) << 34)).astype(np.float64)
        res.update({"n_major": n_major, "n_minor": n_minor, "nnz": nnz})
        for n_donors, listed in ((8, None), (16, None), (64, 64)):
            cls = torch.multinomial(torch.tensor([0.35, 0.3, 0.2, 0.15], device=dev), n_minor * n_donors, replacement=True, generator=gen)
            table = byte_of[cls].reshape(n_minor, n_donors).contiguous()
            if listed is None:
                pairs_host = np.stack(np.triu_indices(n_donors, 1), axis=1).astype(np.int64)
            else:
                pairs_host = torch.randint(0, n_donors, (listed, 2), device=dev, generator=gen).cpu().numpy().astype(np.int64)
            n_pairs = len(pairs_host)
            pairs = torch.from_numpy(pairs_host.astype(np.int32).reshape(-1).copy()).to(dev)
            n = n_major * n_pairs * C6
            out = {"sum_alt": torch.empty(n, dtype=torch.int64, device=dev), "sum_ref": torch.empty(n, dtype=torch.int64, device=dev),
                   "n_obs": torch.empty(n, dtype=torch.int32, device=dev)}
            torch.cuda.synchronize(dev)

            def pair_call():
                return ctx.csr_geno_pair_tally(n_major, n_minor, nnz, csr["indptr"].data_ptr(), csr["indices"].data_ptr(), csr["alt"].data_ptr(),
                                               csr["ref"].data_ptr(), table.data_ptr(), n_donors, pairs.data_ptr(), n_pairs,
                                               {k: v.data_ptr() for k, v in out.items()})
            pair_call()
            # ---- correctness first: per pair, numpy's bincount over (row, class) with the packed counts as weights (exact) ----
            got = {k: v.cpu().numpy().reshape(n_major, n_pairs, C6).astype(np.int64) for k, v in out.items()}
            dosage = np.array([0, 1, 2, 50], np.int8)[cls.reshape(n_minor, n_donors).cpu().numpy()]
            per_entry = [np.ascontiguousarray(dosage[:, d])[host["indices"]] for d in range(n_donors)]      # one gather per donor, shared by its pairs

            def check_pair(p):
                two = per_entry[pairs_host[p, 0]] + per_entry[pairs_host[p, 1]]
                key = rows_host * C6 + np.where(two > 4, 5, two)
                want = np.bincount(key, weights=packed, minlength=n_major * C6).astype(np.int64).reshape(n_major, C6)
                for k, shift in (("sum_alt", 0), ("sum_ref", 17), ("n_obs", 34)):
                    assert np.array_equal(got[k][:, p], (want >> shift) & 0x1FFFF), (n_donors, p, k)
            with ThreadPoolExecutor(8) as pool:
                list(pool.map(check_pair, range(n_pairs)))
            del per_entry, dosage, got
            print("%d donors, %d pairs: equals the numpy model" % (n_donors, n_pairs), flush=True)
            E = {"n_pairs": n_pairs, "geno_pair_tally": series(pair_call, ctx.csr_ms)}
            # (a) the one-donor tally on the same CSR and table: the cost of a (entry, donor) slot
            n1 = n_major * n_donors * 4
            out1 = {"sum_alt": torch.empty(n1, dtype=torch.int64, device=dev), "sum_ref": torch.empty(n1, dtype=torch.int64, device=dev),
                    "n_obs": torch.empty(n1, dtype=torch.int32, device=dev)}
            torch.cuda.synchronize(dev)

            def tally_call():
                return ctx.csr_geno_tally(n_major, n_minor, nnz, csr["indptr"].data_ptr(), csr["indices"].data_ptr(), csr["alt"].data_ptr(),
                                          csr["ref"].data_ptr(), table.data_ptr(), n_donors, {k: v.data_ptr() for k, v in out1.items()})
            E["geno_tally"] = series(tally_call, ctx.csr_ms)
            del out1
            pair_ms, one_ms = (E[k]["device_ms_by_phase_median"]["place"] for k in ("geno_pair_tally", "geno_tally"))
            E["ns_per_entry_pair"] = round(pair_ms * 1e6 / (nnz * n_pairs), 5)
            E["ns_per_entry_donor"] = round(one_ms * 1e6 / (nnz * n_donors), 5)

            # (b) torch on the device: per pair two gathered genotype columns, the dosage, three index_add_ into the dense buffer
            def torch_tally():
                rows = torch.repeat_interleave(torch.arange(n_major, device=dev), csr["indptr"][1:] - csr["indptr"][:-1])
                cols = csr["indices"].to(torch.int64)
                a, r = csr["alt"].to(torch.int64), csr["ref"].to(torch.int64)
                w = (a, r, ((a + r) > 0).to(torch.int64))
                o = [torch.zeros(n, dtype=torch.int64, device=dev) for _ in w]
                for p in range(n_pairs):
                    ga, gb = (table[:, int(pairs_host[p, s])][cols].to(torch.int64) for s in (0, 1))
                    c = torch.where((ga == abi.VTX_GENO_NONE) | (gb == abi.VTX_GENO_NONE), 5, ga + gb)
                    key = (rows * n_pairs + p) * C6 + c
                    for dst, src in zip(o, w):
                        dst.index_add_(0, key, src)
                torch.cuda.synchronize(dev)
                return o
            try:
                dense = torch_tally()
                for d, k in zip(dense, abi.GENO_TALLY_NAMES):
                    assert torch.equal(d, out[k].to(torch.int64)), k
                del dense
                E["torch_gather_index_add_dense"] = series(torch_tally)
                E["torch_over_call"] = round(E["torch_gather_index_add_dense"]["host_wall_ms_median"] / E["geno_pair_tally"]["host_wall_ms_median"], 2)
            except Exception as e:                               # noqa: BLE001  (the record IS the error)
                E["torch_gather_index_add_dense"] = {"error": "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200] if str(e) else "")}
            res["sizes"]["%d_donors_%d_pairs" % (n_donors, n_pairs)] = E
            print(n_donors, n_pairs, "pair tally", E["geno_pair_tally"]["device_ms_by_phase_median"], "wall", E["geno_pair_tally"]["host_wall_ms_median"],
                  "donor tally", E["geno_tally"]["device_ms_by_phase_median"], "ns per (entry, pair)", E["ns_per_entry_pair"], "per (entry, donor)",
                  E["ns_per_entry_donor"], "torch", E["torch_gather_index_add_dense"].get("host_wall_ms_median", E["torch_gather_index_add_dense"].get("error")),
                  flush=True)
            del out, table, cls, pairs
    finish(res)
    sys.exit(0)

if args.dense:
    n_cell, n_var, mean = args.barcodes, args.loci, 2392.3 * args.loci / 100_000
    res = {"what": "vtx_csr_dense_sum (tools/csr_profile.py --dense): median of %d after one warm-up, one process; --geno's synthetic cell-major "
                   "CSR (Poisson row lengths, uniform random columns, counts 0 - 2) and its transpose, int32 tables uniform in [-2^20, 2^20); every "
                   "result compared with a float64 matmul on the host (the sums stay below 2^53) before it is timed; device ms by phase from "
                   "vtx_last_csr_ms" % args.runs, "dense_max": lib.load().vtx_csr_dense_max(), "library": os.path.basename(lib.LIB_PATH), "shapes": {}}
    gen = torch.Generator(device=dev).manual_seed(11)
    with lib.Context(default_config(n_barcodes=4)) as ctx:
        lens = torch.poisson(torch.full((n_cell,), mean, device=dev), generator=gen).clamp_(max=n_var).to(torch.int64)
        indptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
        nnz = int(indptr[-1])
        cells = {"indptr": indptr, "indices": torch.randint(0, n_var, (nnz,), dtype=torch.int32, device=dev, generator=gen)}
        for k in ("alt", "ref"):
            cells[k] = torch.randint(0, 3, (nnz,), dtype=torch.int32, device=dev, generator=gen)
        variants = api._transpose(ctx, torch, dev, cells, n_cell, n_var, ("alt", "ref"))
        res.update({"n_cells": n_cell, "n_variants": n_var, "nnz": nnz})
        for name, csr, n_major, n_minor in (("cells_x_variants", cells, n_cell, n_var), ("variants_x_cells", variants, n_var, n_cell)):
            host = {k: v.cpu().numpy() for k, v in csr.items()}
            mats = [sp.csr_matrix((host[k].astype(np.float64), host["indices"], host["indptr"]), shape=(n_major, n_minor)) for k in ("alt", "ref")]
            rows = torch.repeat_interleave(torch.arange(n_major, device=dev), csr["indptr"][1:] - csr["indptr"][:-1])
            cols = csr["indices"].to(torch.int64)
            one = {"n_major": n_major, "n_minor": n_minor, "n_cols": {}}
            for n_cols in (8, 16, 64):
                w = [torch.randint(-(1 << 20), 1 << 20, (n_minor, n_cols), dtype=torch.int32, device=dev, generator=gen) for _ in range(2)]
                out = torch.empty((n_major, n_cols), dtype=torch.int64, device=dev)
                torch.cuda.synchronize(dev)

                def call(w_alt, w_ref):
                    return lambda: ctx.csr_dense_sum(n_major, n_minor, nnz, csr["indptr"].data_ptr(), csr["indices"].data_ptr(), csr["alt"].data_ptr(),
                                                     csr["ref"].data_ptr(), w_alt.data_ptr() if w_alt is not None else 0,
                                                     w_ref.data_ptr() if w_ref is not None else 0, n_cols, out.data_ptr())
                calls = {"both_tables": call(*w), "w_alt_only": call(w[0], None), "w_ref_only": call(None, w[1])}
                # ---- correctness first: float64 matmuls on the host, exact below 2^53 ----
                want = [m @ t.cpu().numpy().astype(np.float64) for m, t in zip(mats, w)]
                assert max(float(np.abs(x).max()) for x in want) * 2 < 1 << 53
                for key, model in (("both_tables", want[0] + want[1]), ("w_alt_only", want[0]), ("w_ref_only", want[1])):
                    out.fill_(-1)
                    torch.cuda.synchronize(dev)
                    calls[key]()
                    assert np.array_equal(out.cpu().numpy(), model.astype(np.int64)), (name, n_cols, key)
                print("%s, %d columns: equals the float64 matmul on the host" % (name, n_cols), flush=True)
                E = {key: series(fn, ctx.csr_ms) for key, fn in calls.items()}
                for key in calls:
                    tables = 2 if key == "both_tables" else 1
                    E[key]["ps_per_entry_column"] = round(E[key]["device_ms_by_phase_median"]["place"] * 1e9 / (nnz * n_cols), 3)
                    E[key]["ps_per_entry_column_table"] = round(E[key]["ps_per_entry_column"] / tables, 3)
                # (b) torch on the device: two torch.sparse.mm of float64 CSR copies against float64 tables; where this build has no device
                # CSR x dense product, --geno's form: rows by repeat_interleave, a gather of the table rows, index_add_ into a dense buffer
                wf = [t.to(torch.float64) for t in w]
                both = calls["both_tables"]
                both()
                mine = out.to(torch.float64)

                def torch_spmm():
                    o = torch.sparse.mm(spm[0], wf[0]) + torch.sparse.mm(spm[1], wf[1])
                    torch.cuda.synchronize(dev)
                    return o

                def torch_index_add():
                    o = torch.zeros((n_major, n_cols), dtype=torch.float64, device=dev)
                    for counts, t in zip((csr["alt"], csr["ref"]), wf):
                        o.index_add_(0, rows, counts.to(torch.float64)[:, None] * t[cols])
                    torch.cuda.synchronize(dev)
                    return o
                try:
                    spm = [torch.sparse_csr_tensor(csr["indptr"], cols, csr[k].to(torch.float64), size=(n_major, n_minor)) for k in ("alt", "ref")]
                    assert torch.equal(torch_spmm(), mine)
                    E["torch_sparse_mm_f64"] = series(torch_spmm)
                    baseline = "torch_sparse_mm_f64"
                    del spm
                except Exception as e:                           # noqa: BLE001  (the record IS the error)
                    E["torch_sparse_mm_f64"] = {"error": "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200] if str(e) else "")}
                    baseline = "torch_gather_index_add_f64"
                    try:
                        assert torch.equal(torch_index_add(), mine)
                        E[baseline] = series(torch_index_add)
                    except Exception as e2:                      # noqa: BLE001
                        E[baseline] = {"error": "%s: %s" % (type(e2).__name__, str(e2).splitlines()[0][:200] if str(e2) else "")}
                E["torch_baseline"] = baseline
                if "host_wall_ms_median" in E[baseline]:
                    E["torch_over_call"] = round(E[baseline]["host_wall_ms_median"] / E["both_tables"]["host_wall_ms_median"], 2)
                one["n_cols"][str(n_cols)] = E
                print(name, n_cols, {key: (E[key]["host_wall_ms_median"], E[key]["device_ms_by_phase_median"]["place"], E[key]["ps_per_entry_column"])
                                     for key in calls}, baseline, E[baseline].get("host_wall_ms_median", E[baseline].get("error")), flush=True)
                del w, wf, out, mine, want
            res["shapes"][name] = one
            del host, mats, rows, cols
        del variants
    # one whole clustering at this shape, of the torch result run(to="torch") would hand over.  The uniform counts above carry no donors
    # (at 2 400 entries a cell a random start is a fixed point of the EM at once: a cell's own reads dominate its cluster's theta), so
    # eight donors are planted on the same sparsity: genotypes uniform in {0, 1, 2}, depth 1 - 3, alt reads binomial at 0.01 / 0.5 / 0.99
    k = 8
    donor = torch.arange(n_cell, device=dev) % k
    rows = torch.repeat_interleave(torch.arange(n_cell, device=dev), cells["indptr"][1:] - cells["indptr"][:-1])
    geno = torch.randint(0, 3, (n_var, k), device=dev, generator=gen)
    p_alt = torch.tensor([0.01, 0.5, 0.99], dtype=torch.float64, device=dev)[geno[cells["indices"].to(torch.int64), donor[rows]]]
    depth = torch.randint(1, 4, (nnz,), device=dev, generator=gen)
    alt = torch.binomial(depth.to(torch.float64), p_alt, generator=gen).to(torch.int32)
    counts = {"alt": alt, "ref": depth.to(torch.int32) - alt}
    del rows, geno, p_alt
    as_csr = [torch.sparse_csr_tensor(cells["indptr"], cells["indices"].to(torch.int64), counts[f], size=(n_cell, n_var)) for f in ("alt", "ref")]
    result = api.Result(matrix=None, ref_matrix=None, alt_counts=as_csr[0], ref_counts=as_csr[1], unknown_counts=None, variants=[""] * n_var,
                        barcodes=[""] * n_cell, metrics={}, shape=(n_cell, n_var), orient="cells")
    timed(lambda: api.cluster_donors(result, k, n_init=1, max_iter=1))      # warm-up: torch's kernels, the allocator
    wall, c = timed(lambda: api.cluster_donors(result, k, n_init=1))
    pairs = set(zip(donor.cpu().tolist(), c.labels.cpu().tolist()))
    res["cluster_donors"] = {"k": k, "n_init": 1, "rounds": c.n_iter, "converged": c.converged, "total_ms": round(wall, 1),
                             "ms_per_round": round(wall / c.n_iter, 2), "plant_recovered": len(pairs) == k and len({b for _, b in pairs}) == k,
                             "note": "one restart, after a warm-up call of one round; the total includes the bare context, one vtx_csr_transpose "
                             "and the row sums of the guard; eight planted donors on the sparsity of the sums above"}
    print("cluster_donors", res["cluster_donors"], flush=True)
    finish(res)
    sys.exit(0)

spec = synth.SynthSpec(n_loci=args.loci, n_barcodes=args.barcodes, reads_per_locus=args.reads_per_locus, read_len=150, padding=100,
                       use_umi=False, indel_frac=0.0, sub_error=0.005, depth_sigma=0.0, seed=20260926)      # bench.py's config 3, its defaults spelled out
t0 = time.perf_counter()
batch = synth.make_batch(spec)
print("batch: %d records in %.1f s" % (batch.n_records, time.perf_counter() - t0), flush=True)
n_rows, n_cols = args.loci, args.barcodes


res = {"what": "CSR hand-over of a config-3 run (tools/csr_profile.py): median of %d after one warm-up, one process" % args.runs,
       "loci": n_rows, "barcodes": n_cols, "records": int(batch.n_records), "entries": {}}
with lib.Context(default_config(n_barcodes=n_cols)) as ctx:
    ctx.submit(batch)
    ctx.run()
    res["vtx_run_total_ms"] = round(float(ctx.timing().total_ms), 3)
    part = api._device_part(ctx, torch, dev, 0, n_rows)
    nnz = int(part["indices"].shape[0])
    res["nnz"] = nnz
    if args.ops:
        res["what"] = "summaries and selections of a config-3 run's CSR (tools/csr_profile.py --ops): median of %d after one warm-up, one process" % args.runs
        E = res["entries"]
        t = api._transpose(ctx, torch, dev, part, n_rows, n_cols)
        coo = ctx.fetch_coo()
        indptr_h, indices_h = part["indptr"].cpu().numpy(), part["indices"].cpu().numpy()
        # ---- correctness first ----
        v_out, c_out = stats_buffers(n_rows), stats_buffers(n_cols)
        v_call, c_call = stats_call(ctx, part, n_rows, n_cols, v_out), stats_call(ctx, t, n_cols, n_rows, c_out)
        torch.cuda.synchronize(dev)
        v_call()
        c_call()
        v_want = host_stats(indptr_h, coo["alt"], coo["ref"], coo["unk"])
        same_stats(v_out, v_want)
        order = np.argsort(coo["col"], kind="stable")
        same_stats(c_out, host_stats(np.searchsorted(coo["col"][order], np.arange(n_cols + 1)), coo["alt"][order], coo["ref"][order], coo["unk"][order]))
        positions = sp.csr_matrix((np.arange(nnz, dtype=np.float64), indices_h, indptr_h), shape=(n_rows, n_cols))
        res["select"] = {}

        def selection(label, rule, keep_h):
            """One selection of variants: checked against scipy's indexing, then ready to be timed -> (plan call, select call, outputs)."""
            keep = torch.from_numpy(keep_h).to(dev)
            head = (n_rows, n_cols, nnz, part["indptr"].data_ptr(), part["indices"].data_ptr(), keep.data_ptr(), 0)
            torch.cuda.synchronize(dev)
            sizes = ctx.csr_select_plan(*head)
            sel = {"indptr": torch.empty(sizes[0] + 1, dtype=torch.int64, device=dev), "indices": torch.empty(sizes[2], dtype=torch.int32, device=dev)}
            for k in api.DATA_FIELDS:
                sel[k] = torch.empty(sizes[2], dtype=part[k].dtype, device=dev)
            ids = torch.empty(sizes[0], dtype=torch.int32, device=dev)
            pay = [(part[k].data_ptr(), sel[k].data_ptr(), part[k].element_size()) for k in api.DATA_FIELDS]
            torch.cuda.synchronize(dev)

            def select_call():
                return ctx.csr_select(*head, sizes, sel["indptr"].data_ptr(), sel["indices"].data_ptr(), ids.data_ptr(), 0, pay)
            select_call()
            want = positions[keep_h]
            assert sizes == (int(keep_h.sum()), n_cols, want.nnz)
            assert np.array_equal(sel["indptr"].cpu().numpy(), want.indptr) and np.array_equal(sel["indices"].cpu().numpy(), want.indices)
            src = want.data.astype(np.int64)
            for k in api.DATA_FIELDS:
                assert np.array_equal(sel[k].cpu().numpy().view(np.uint8), np.ascontiguousarray(coo[k][src]).view(np.uint8)), k
            assert np.array_equal(ids.cpu().numpy(), np.flatnonzero(keep_h))
            res["select"][label] = {"rule": rule, "variants_kept": sizes[0], "entries_kept": sizes[2]}
            print("%s: selection equals scipy's: %d of %d variants, %d of %d entries kept" % (label, sizes[0], n_rows, sizes[2], nnz), flush=True)
            return keep, (lambda: ctx.csr_select_plan(*head)), select_call, sel, (keep, ids, pay)
        # the issue's rule, and — it keeps every variant of this batch, 239 cells a row — the median of n_alt, which keeps about half
        med = int(np.median(v_want["n_alt"]))
        keep, plan_call, select_call, sel, _hold = selection("min10", "n_alt >= 10 and n_ref >= 10", (v_want["n_alt"] >= 10) & (v_want["n_ref"] >= 10))
        keep_h = v_want["n_alt"] > med
        keep2, plan2, select2, sel2, _hold2 = selection("above_median", "n_alt > %d (the median)" % med, keep_h)
        sizes = (int(keep_h.sum()), n_cols, int(sel2["indices"].shape[0]))
        del order
        # ---- the device calls ----
        E["row_stats_variant_major"] = series(v_call, ctx.csr_ms)
        E["row_stats_cell_major"] = series(c_call, ctx.csr_ms)
        E["select_plan_min10"] = series(plan_call, ctx.csr_ms)
        E["select_five_payloads_min10"] = series(select_call, ctx.csr_ms)
        E["select_plan_above_median"] = series(plan2, ctx.csr_ms)
        E["select_five_payloads_above_median"] = series(select2, ctx.csr_ms)
        keep, sel = keep2, sel2                                  # the baselines below make the selection that drops rows
        E["api_row_stats_variant_major"] = series(lambda: api._row_stats(ctx, torch, dev, part, n_rows, n_cols))
        E["api_select"] = series(lambda: api._select(ctx, torch, dev, part, n_rows, n_cols, keep, None))
        # ---- which operations this torch build offers on a sparse CSR tensor ----
        m = torch.sparse_csr_tensor(part["indptr"], part["indices"].to(torch.int64), part["alt"].to(torch.float64), size=(n_rows, n_cols))
        probes = {"sum(dim=1)": lambda: m.sum(dim=1), "sum()": lambda: m.sum(), "boolean row selection m[mask]": lambda: m[keep],
                  "index_select(0, ids)": lambda: m.index_select(0, torch.nonzero(keep).ravel()), "to_sparse_coo()": lambda: m.to_sparse_coo(),
                  "(m != 0)": lambda: m != 0, "select(0, 5)": lambda: m.select(0, 5), "transpose(0, 1)": lambda: m.transpose(0, 1),
                  "int32 values": lambda: torch.sparse_csr_tensor(part["indptr"], part["indices"].to(torch.int64), part["alt"], size=(n_rows, n_cols)).sum()}
        res["torch_sparse_csr_support"] = {"torch": torch.__version__}
        for name, fn in probes.items():
            try:
                fn()
                torch.cuda.synchronize(dev)
                res["torch_sparse_csr_support"][name] = "ok"
            except Exception as e:                               # noqa: BLE001  (the record IS the error)
                res["torch_sparse_csr_support"][name] = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:160])
        del m
        # ---- what a user does today, on the device in torch: rows from the offsets (the COO view), index_add_, boolean masking ----
        def torch_rows():
            return torch.repeat_interleave(torch.arange(n_rows, device=dev), part["indptr"][1:] - part["indptr"][:-1])

        def torch_stats():
            rows = torch_rows()
            a, r, u = part["alt"], part["ref"], part["unk"]
            out = {}
            for k, w in (("n_entries", torch.ones_like(a, dtype=torch.int64)), ("n_alt", (a > 0).to(torch.int64)), ("n_ref", (r > 0).to(torch.int64)),
                         ("n_both", ((a > 0) & (r > 0)).to(torch.int64)), ("sum_alt", a.to(torch.int64)), ("sum_ref", r.to(torch.int64)),
                         ("sum_unk", u.to(torch.int64))):
                out[k] = torch.zeros(n_rows, dtype=torch.int64, device=dev).index_add_(0, rows, w)
            torch.cuda.synchronize(dev)
            return out

        def torch_select():
            rows = torch_rows()
            k = keep[rows]
            out = {f: part[f][k] for f in ("indices",) + api.DATA_FIELDS}
            new_row = (torch.cumsum(keep.to(torch.int64), 0) - 1)[rows[k]]
            out["indptr"] = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(torch.bincount(new_row, minlength=sizes[0]), 0)])
            torch.cuda.synchronize(dev)
            return out
        def same_selection(o):
            for f in sel:
                assert torch.equal(o[f], sel[f]), f
        for name, fn, check in (("torch_index_add_stats", torch_stats, lambda o: same_stats(o, v_want)), ("torch_mask_select", torch_select, same_selection)):
            try:
                check(fn())
                E[name] = series(fn)
            except Exception as e:                               # noqa: BLE001
                E[name] = {"error": "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200] if str(e) else "")}
        # ---- ... and on the host: fetch + numpy / scipy ----
        def host_stats_today():
            c = ctx.fetch_coo()
            return host_stats(np.searchsorted(c["row"], np.arange(n_rows + 1)), c["alt"], c["ref"], c["unk"])

        def host_select_today():
            c = ctx.fetch_coo()
            return [sp.coo_matrix((c[f], (c["row"], c["col"])), shape=(n_rows, n_cols)).tocsr()[keep_h] for f in api.DATA_FIELDS]
        E["fetch_numpy_stats"] = series(host_stats_today)
        E["fetch_scipy_select_five_matrices"] = series(host_select_today)
        E["fetch_coo_alone"] = series(ctx.fetch_coo)
        finish(res)
        sys.exit(0)
    # ---- correctness first: the device's offsets and transpose against scipy's ----
    coo = ctx.fetch_coo()
    want = sp.coo_matrix((coo["value"], (coo["row"], coo["col"])), shape=(n_rows, n_cols)).tocsr()
    assert np.array_equal(part["indptr"].cpu().numpy(), want.indptr) and np.array_equal(part["indices"].cpu().numpy(), want.indices)
    t = api._transpose(ctx, torch, dev, part, n_rows, n_cols)
    pos = sp.csr_matrix((np.arange(1, nnz + 1, dtype=np.float64), want.indices, want.indptr), shape=want.shape).T.tocsr()
    assert np.array_equal(t["indptr"].cpu().numpy(), pos.indptr) and np.array_equal(t["indices"].cpu().numpy(), pos.indices)
    order = pos.data.astype(np.int64) - 1
    for k, f in (("value", "value"), ("ref_value", "ref_value"), ("alt", "alt"), ("ref", "ref"), ("unk", "unk")):
        assert np.array_equal(t[k].cpu().numpy().view(np.uint8), np.ascontiguousarray(coo[f][order]).view(np.uint8)), k
    del t, pos, order, want
    print("device CSR and transpose equal scipy's (%d entries)" % nnz, flush=True)
    # ---- the device calls ----
    res["entries"]["device_csr"] = series(lambda: ctx.device_csr(0, n_rows), ctx.csr_ms)
    out = {"indptr": torch.empty(n_cols + 1, dtype=torch.int64, device=dev), "indices": torch.empty(nnz, dtype=torch.int32, device=dev)}
    for k in api.DATA_FIELDS:
        out[k] = torch.empty_like(part[k])
    payloads = [(part[k].data_ptr(), out[k].data_ptr(), 8 if part[k].dtype == torch.float64 else 4) for k in api.DATA_FIELDS]
    res["entries"]["csr_transpose"] = series(lambda: ctx.csr_transpose(n_rows, n_cols, nnz, part["indptr"].data_ptr(), part["indices"].data_ptr(),
                                                                        out["indptr"].data_ptr(), out["indices"].data_ptr(), 0, payloads), ctx.csr_ms)
    res["entries"]["csr_transpose"]["payload_arrays"] = len(payloads)
    res["entries"]["csr_transpose_no_payload"] = series(lambda: ctx.csr_transpose(n_rows, n_cols, nnz, part["indptr"].data_ptr(), part["indices"].data_ptr(),
                                                                                   out["indptr"].data_ptr(), out["indices"].data_ptr(), 0, []), ctx.csr_ms)
    # ---- what a user does today ----
    def today_csr():
        c = ctx.fetch_coo()
        return sp.coo_matrix((c["value"], (c["row"], c["col"])), shape=(n_rows, n_cols)).tocsr()

    def today_csr_t():
        return today_csr().T.tocsr()
    res["entries"]["fetch_coo_to_csr"] = series(today_csr)
    res["entries"]["fetch_coo_to_csr_T"] = series(today_csr_t)
    res["entries"]["fetch_coo_alone"] = series(ctx.fetch_coo)
    if not args.skip_mmread:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "m.mtx")

            def today_file():
                ctx.write_mtx(path, n_rows, n_cols, 0)
                return scipy.io.mmread(path).tocsr()
            res["entries"]["write_mtx_mmread"] = series(today_file)
            res["entries"]["write_mtx_mmread"]["file_bytes"] = os.path.getsize(path)
finish(res)
