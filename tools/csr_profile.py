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
GPU box:   python tools/csr_profile.py --json profiles/r12_csr.json"""
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
args = ap.parse_args()

dev = torch.device("cuda", 0)
spec = synth.SynthSpec(n_loci=args.loci, n_barcodes=args.barcodes, reads_per_locus=args.reads_per_locus, read_len=150, padding=100,
                       use_umi=False, indel_frac=0.0, sub_error=0.005, depth_sigma=0.0, seed=20260926)      # bench.py's config 3, its defaults spelled out
t0 = time.perf_counter()
batch = synth.make_batch(spec)
print("batch: %d records in %.1f s" % (batch.n_records, time.perf_counter() - t0), flush=True)
n_rows, n_cols = args.loci, args.barcodes


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


res = {"what": "CSR hand-over of a config-3 run (tools/csr_profile.py): median of %d after one warm-up, one process" % args.runs,
       "loci": n_rows, "barcodes": n_cols, "records": int(batch.n_records), "entries": {}}
with lib.Context(default_config(n_barcodes=n_cols)) as ctx:
    ctx.submit(batch)
    ctx.run()
    res["vtx_run_total_ms"] = round(float(ctx.timing().total_ms), 3)
    part = api._device_part(ctx, torch, dev, 0, n_rows)
    nnz = int(part["indices"].shape[0])
    res["nnz"] = nnz
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
print(json.dumps(res), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
json.dump(res, open(args.json, "w"), indent=1)
