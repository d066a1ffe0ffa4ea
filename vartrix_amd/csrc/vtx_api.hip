// vtx_api.hip — C-ABI layer of libvtx.so (see include/vtx.h for the contract).
//
// Owns the HIP context state: device buffers sized for the resident batch, the
// per-bucket work lists, one stream, hipEvents for timing.  No CPU compute
// path exists here: without a device every entry point fails.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <rccl/rccl.h>      // types and prototypes only: the library is dlopen'ed on first use (vtx_comm_*)
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <mutex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "vtx_device.h"
#include "vtx_ingest.h"
#include "vtx_deflate_core.h"
#include "vtx_inflate_core.h"
#include "vtx_mtx_join.h"
#include "vtx_csr_core.h"
#include "vtx_csr_ops_core.h"
#include "vtx_csr_group_core.h"
#include "vtx_csr_geno_core.h"
#include "vtx_csr_geno_pair_core.h"
#include "vtx_csr_dense_core.h"
#include "../../include/vtx_band_semantics.h"

extern "C" hipError_t vtxk_inclusive_scan_u32(const uint32_t* in, uint32_t* out, uint32_t n, void* temp,
                                              size_t temp_bytes, hipStream_t s) {
    if (!n) return hipSuccess;
    return hipcub::DeviceScan::InclusiveSum(temp, temp_bytes, in, out, (int)n, s);
}
extern "C" size_t vtxk_scan_temp_bytes(uint32_t n) {
    size_t bytes = 0;
    hipcub::DeviceScan::InclusiveSum(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)std::max(n, 1u));
    return bytes;
}

namespace {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <typename T> T* as() const { return (T*)p; }
};

struct Bucket { int R, GL; uint32_t offset, count; bool lut; bool duo = false; bool pair = false; };
const uint32_t kLutLociCap = 4;     // loci tables per workgroup of the LUT kernel (6 KiB each at 257 columns)
const uint32_t kDuoLociCap = 8;     // the duo kernel runs 3 workgroups per CU (VGPRs), so up to 52 KiB of tables cost no occupancy

// (rows per lane, lanes per record) choices; capacity = R * GL read bases.
const int kShapes[][2] = {{2, 16}, {4, 16}, {6, 16}, {8, 16}, {10, 16}, {12, 16}, {16, 16}, {8, 64}, {16, 64}};
const int kNumShapes = sizeof(kShapes) / sizeof(kShapes[0]);
const uint32_t kFastReadLen = VTX_FAST_READ_LEN;   // 16 rows x 64 lanes
const uint32_t kFastHapLen = VTX_FAST_HAP_LEN;     // 16 record slots x (len + 35) words must fit 160 KiB of LDS
// Beyond the fast limits a record is scored by slow_align_kernel (exact, one lane per alignment); its 16-bit coordinates
// set the hard limits.
// Slack behind the compressed BAM bytes (d_bam_comp) and behind the inflated ones (d_bam_data): bgzf_inflate_kernel loads whole
// words, up to IN_PAD bytes behind a block's payload and OUT_PAD bytes behind its output (vtx_inflate_core.h), and the last block
// of an upload has nothing else behind it.
const size_t kBamPad = 64;
static_assert(kBamPad >= vtxi::IN_PAD && kBamPad >= vtxi::OUT_PAD, "the inflater's loads must stay inside d_bam_comp / d_bam_data");
const uint32_t kMaxReadLen = 30000;
const uint32_t kMaxHapLen = 30000;
// The call reduction runs one thread per (row, cell) group when the batch's mean group is at most this many records, and the
// histogram kernels (one thread per record, atomics) above it.  4 is the starting value: the crossing has not been measured yet.
const uint32_t kReduceMeanGroupMax = 4;

// vtx_ctx::ev.  vtx_run's slots; the entry points that prepare a batch run at other times and reuse the first four.
enum EvSlot {
    EV_START = 0,           // run_prologue records; run_epilogue reads (full_ms, sw_ms)
    EV_DP_END = 1,          // vtx_run records after the slow path; run_epilogue reads (sw_ms, reduce_ms)
    EV_REDUCE_END = 2,      // run_reduce records; run_epilogue reads (reduce_ms)
    EV_FULL_END = 3,        // run_full_dp records; run_epilogue reads (full_ms)
    EV_CHUNK_START = 4,     // BandPass::resident_tables records; run_stage reads (diag_ms, band_run_ms of a chunk without a sweep)
    EV_BAND_RUN_END = 5,    // run_stage / second_chance record behind band_run_kernel; run_stage reads (band_run_ms)
    EV_DIAG_END = 6,        // diag_sweep_path / diag_round3_path record; run_stage reads (diag_ms); the side stream waits for it (behind band_diag_kernel when
                            // band_tail_kernel runs on the side stream, else behind band_tail_kernel)
    EV_BRANCH_START = 7,    // diag_sweep_path records on the one-diagonal branch's stream, in front of band_tail_kernel when that runs there; collect_sweep_times reads (check_ms)
    EV_SWEEP_END = 8,       // diag_sweep_path records after the join; collect_sweep_times waits for it and reads (sweep_ms)
    EV_BRANCH_END = 9,      // diag_sweep_path records on the branch's stream; the main stream joins on it; collect_sweep_times reads
    EV_BAND_RUN_START = 10, // run_stage records in front of band_run_kernel; run_stage reads (band_run_ms of a swept chunk)
    EV_FORK_START = 11,     // diag_sweep_path records where the main stream's branch starts (forked); collect_sweep_times reads
    EV_COUNT = 12
};
enum PrepEv { EV_PREP_START = 0, EV_PREP_END = 1 };                                                // the same array in vtx_submit_raw: around the preparation
enum IngestEv { EV_INGEST_START = 0, EV_INFLATE_END = 1, EV_INDEX_END = 2, EV_FILTER_END = 3 };    // ... and in vtx_submit_bam: its phases
// vtx_ctx::h_pin: the counters of the banded stage that are read back asynchronously.  A member has the type of the vtx_band_counters member it mirrors (read_back).
struct PinnedCounters {
    vtx_cnt_pair general;                   // GeneralFallback::launch copies (side stream); finish reads
    vtx_band_counters::lists_t lists;       // diag_sweep_path copies the group and reads it; diag_round3_path copies and reads run_left and refine, the two lists that path has
    uint32_t tail;                          // diag_sweep_path copies (band_tail_kernel on the side stream) and reads: what that kernel may still append
    uint32_t fork_tight, fork_refine;       // diag_sweep_path copies lists.tight (forked) and lists.refine (band_tail_kernel there) on the side stream; collect_sweep_times reads
    vtx_band_counters::diag2_t diag2;       // second_stage copies and reads
    uint32_t streamed;                      // likewise
};

thread_local std::string g_create_err;

}  // namespace

template <class T>
struct HostArr {
    T* p = nullptr;
    size_t n = 0;
    ~HostArr() { free(p); }
    bool alloc(size_t count) {
        if (count > n || !p) { free(p); p = (T*)malloc(std::max<size_t>(count, 1) * sizeof(T)); n = p ? count : 0; }
        return p != nullptr;
    }
    T* data() { return p; }
};

// ---- what the CSR calls keep in the context (vtx_device_csr, vtx_csr_*: "the matrices as CSR on the device" below) ----
// Device times: events on the context's stream.  enum CsrEv names what lies between two of them.
enum CsrEv { EV_CSR_CHECK0 = 0, EV_CSR_CHECK1, EV_CSR_SORT0, EV_CSR_SORT1, EV_CSR_OFFSETS1, EV_CSR_PLACE1, EV_CSR_COUNT };
// The verdicts of a call's check kernels: one 64-bit word each in ONE buffer, set by one copy in front of the checks (kCsrVerdictInit)
// and read by one copy behind them (csr_judged).  A word is the OR of bad bits (from zero) or the minimum over the offenders (from all ones).
enum CsrVerdict {
    V_CSR_BAD = 0,         // vtxr_check / vtxr_window_check: the OR of vtxr::Bad bits, in the low 32 bits
    V_LABEL,               // vtxr_group_check: the lowest column with a bad label (a 32-bit atomicMin on the low 32 bits)
    V_GENO,                // vtxr_geno_check: the lowest flat index of a bad genotype byte
    V_PAIR,                // vtxr_geno_pair_check: the lowest pair with a donor out of range
    V_COUNT
};
struct CsrWork {
    hipEvent_t ev[EV_CSR_COUNT] = {};        // created on first use (csr_events)
    float ms[4] = {};                        // vtx_last_csr_ms: check, sort, offsets, place
    DevBuf d_verdict;                        // V_COUNT words
    DevBuf d_indptr;                         // vtx_device_csr: the row offsets of d_o_row (a buffer of its own: no other call works in it)
    DevBuf d_keys, d_iota, d_perm, d_tmp;    // vtx_csr_transpose: sorted columns, positions, perm (when the caller wants none), the sort's work space
    DevBuf d_sel_pos, d_sel_major, d_sel_minor, d_sel_tmp;   // vtx_csr_select_plan / vtx_csr_select: pos[nnz + 1], major_map[n_major + 1], minor_map[n_minor + 1], the scan's work space
    DevBuf d_grp_pos, d_grp_tmp;             // vtx_csr_group_plan / vtx_csr_group_sum: pos[n_major + 1], the scan's work space
    template <typename T> T* verdict(CsrVerdict v) const { return (T*)(d_verdict.as<uint64_t>() + v); }
    void release() {
        for (DevBuf* b : {&d_verdict, &d_indptr, &d_keys, &d_iota, &d_perm, &d_tmp, &d_sel_pos, &d_sel_major, &d_sel_minor, &d_sel_tmp, &d_grp_pos, &d_grp_tmp}) b->release();
    }
    void destroy_events() { for (auto& e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; } }
};

struct vtx_ctx {
    vtx_config cfg{};
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;           // side stream: the general band kernel runs beside the pending / masked kernels
    hipEvent_t ev2 = nullptr;
    // multi-GPU row gather (vtx_comm_init / vtx_gather_coo)
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 0;
    DevBuf d_g_cnt, d_g_row, d_g_col, d_g_alt, d_g_ref, d_g_unk, d_g_val, d_g_refval;
    uint64_t g_nnz = 0;
    PinnedCounters* h_pin = nullptr;         // pinned memory for counters read back asynchronously (a D2H copy into pageable
                                             // memory blocks the host until the stream reaches it)
    hipEvent_t ev[EV_COUNT] = {};
    hipEvent_t ev_crc[2] = {};               // around bgzf_crc32_kernel (vtx_submit_bam, vtx_debug_crc32)
    float crc_ms = 0;                        // vtx_last_crc_ms
    CsrWork csr;                             // vtx_device_csr and the vtx_csr_* calls: events, phase times, verdict words, work space
    std::string err;
    bool submitted = false, ran = false;
    uint32_t n_loci = 0, n_records = 0, n_cell_groups = 0, n_umi_groups = 0, max_hap_len = 0;
    uint64_t cells = 0, nnz = 0;
    std::vector<Bucket> buckets;
    vtx_timing timing{};
    DevBuf d_loci, d_records, d_rec_locus, d_hap, d_read, d_work, d_ref, d_alt;
    DevBuf d_head_cell, d_head_umi, d_cell_scan, d_umi_scan, d_grp_row, d_grp_col, d_umi_cellgrp;
    DevBuf d_grp_start;                      // first record of every (row, cell) group + one last entry, n_records (build_groups)
    int reduce_path = 0;                     // the last vtx_run's call reduction: 1 = histogram kernels (atomics), 2 = one pass per group
    DevBuf d_cell_cnt, d_umi_cnt, d_keep, d_keep_scan, d_scan_tmp;
    DevBuf d_o_row, d_o_col, d_o_alt, d_o_ref, d_o_unk, d_o_val, d_o_refval;
    bool band_long_lists = false;      // (performance feedback between runs: see vtx_run)
    int read_format = VTX_READS_BYTES;     // vtx_set_read_format
    DevBuf d_read_packed;                  // VTX_READS_NIBBLES: the arena as uploaded, unpacked into d_read
    uint64_t gt_used = 0;      // bytes of d_gtables the last banded run's table kernel wrote (vtx_debug_tables)
    DevBuf d_band_ws, d_band_ws2, d_band, d_poly, d_gtables, d_hard, d_over, d_over2, d_pend, d_pend_buf, d_cnt, d_band2, d_hard2, d_fail, d_fail_tmp, d_refine, d_tail, d_recheck;   // banded flavour
    DevBuf d_tight2, d_tight2_pack;                                          // band_diag2_kernel: tasks whose band is one diagonal stretch after all
    DevBuf d_recheck2, d_recheck2_pack;                                      // ... of which the full-matrix check did not settle (full != certificate); first they hold band_stream_kernel's task list and diagonals
    DevBuf d_sweep_log;                                                      // band_sweep_kernel: the section logs of the resident workgroups (48 MB: 1 536 x 8 x 1 024 words)
    DevBuf d_tight, d_tight_pack, d_dband, d_dband_pack, d_dense, d_stage;                                                 // round 4: tasks with a provisional score (full-matrix check); stage bytes (vtx_fetch_stage)
    bool stage_trace = false, poison = false;                                // test / audit hooks (vtx_set_debug)
    int32_t poison_value = 0;
    DevBuf d_redo, d_redo_cnt;                                               // LUT kernel: records with non-ACGTN bytes
    // raw batches (vtx_submit_raw): barcode table + preparation scratch
    DevBuf d_bc_slots, d_bc_hash, d_bc_off, d_bc_bytes;
    uint32_t bc_mask = 0;
    bool bc_ready = false;
    DevBuf d_raw, d_tags, d_raw_locus, d_key_lc, d_key_lc2, d_key_umi, d_key_umi2, d_idx, d_idx2, d_shape, d_shape2, d_seq,
        d_locus_cnt, d_locus_scan, d_prep_cnt, d_sort_tmp;
    // device-side BAM ingest (vtx_submit_bam, vtx_ingest.hip): compressed range, inflated stream, record offsets, per-record counts / scans
    DevBuf d_bam_comp, d_bam_data, d_bam_blocks, d_bam_seeds, d_bam_seed_cnt, d_bam_seed_scan, d_bam_iv, d_bam_cnt, d_bam_rec, d_bam_nhit,
        d_bam_rsz, d_bam_tsz, d_bam_hscan, d_bam_rscan, d_bam_tscan, d_bam_info, d_bam_segs;
    // vtx_prefetch_file: bytes [pf_off, pf_off + pf_n) of the BAM on their way into d_bam_comp (a library thread drives the copy workers)
    std::thread pf_thread;
    uint64_t pf_off = 0, pf_n = 0;
    int pf_rc = 0;
    void* pf_map = nullptr;           // the mapping the prefetch reads from (unmapped by the next prefetch / vtx_destroy)
    size_t pf_map_bytes = 0;
    float pf_ms = 0;                  // how long the prefetch's copy took
    bool pf_valid = false;
    std::atomic<bool> pf_cancel{false};      // vtx_submit_bam_segments: the prefetch still in flight stops at its next chunk
    uint32_t bam_n_rec = 0, bam_n_raw = 0;
    uint64_t bam_utotal = 0, bam_read_bases = 0, bam_tag_bytes = 0;
    uint32_t max_read_len = 0, fast_overflow = 0;
    uint32_t slow_off = 0, slow_cnt = 0, max_hap_all = 0, max_read_all = 0;   // records of the slow list (d_work[slow_off ..])
    // a batch that mixes haplotypes of <= 255 bases with longer ones (note_long_loci; vtx_run's two banded passes): the longest haplotype
    // among the former, how many loci the latter are, the first and the last of them
    uint32_t hap_short_max = 0, n_long_loci = 0, long_first = 0, long_last = 0;
    DevBuf d_slow_ws, d_slow_retry;
    // host -> device feed: pinned staging buffers + one stream per copy worker (see upload())
    static constexpr int kUpWorkers = 6, kUpSlots = 2;
    static constexpr size_t kUpChunk = 8u << 20;
    void* up_pin[kUpWorkers][kUpSlots] = {};
    hipEvent_t up_ev[kUpWorkers][kUpSlots] = {};
    hipStream_t up_stream[kUpWorkers] = {};
    bool up_ready = false;
    HostArr<uint32_t> h_row, h_col, h_alt, h_ref, h_unk;   // fetched triplets (uninitialised storage: written by the download)
    HostArr<double> h_val, h_refval;
};

namespace {

int fail(vtx_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_err = buf;
    return code;
}

#define HIP_TRY(c, expr)                                                                       \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return fail((c), _e == hipErrorOutOfMemory ? VTX_E_NOMEM : VTX_E_HIP, "%s: %s", #expr, \
                        hipGetErrorString(_e));                                                \
    } while (0)

// ---- host -> device feed ------------------------------------------------------------------------------------
// The caller's arrays are pageable: a plain hipMemcpy of 3.65 GB (config 3's read arena) runs at ~17 GB/s through
// the runtime's single staging path.  Here kUpWorkers threads each copy 8 MiB chunks into their own pinned buffers
// (two per worker, so the memcpy of chunk k+1 overlaps the DMA of chunk k) and push them on their own stream: the
// host memcpys and the DMAs of different workers overlap, and the link — not one core's memcpy — is the limit.
struct UploadJob { void* dst; const void* src; size_t bytes; };

int upload_init(vtx_ctx* c) {
    if (c->up_ready) return VTX_OK;
    for (int w = 0; w < vtx_ctx::kUpWorkers; ++w) {
        HIP_TRY(c, hipStreamCreateWithFlags(&c->up_stream[w], hipStreamNonBlocking));
        for (int k = 0; k < vtx_ctx::kUpSlots; ++k) {
            HIP_TRY(c, hipHostMalloc(&c->up_pin[w][k], vtx_ctx::kUpChunk, hipHostMallocDefault));
            HIP_TRY(c, hipEventCreateWithFlags(&c->up_ev[w][k], hipEventDisableTiming));
        }
    }
    c->up_ready = true;
    return VTX_OK;
}

void upload_release(vtx_ctx* c) {
    for (int w = 0; w < vtx_ctx::kUpWorkers; ++w) {
        for (int k = 0; k < vtx_ctx::kUpSlots; ++k) {
            if (c->up_pin[w][k]) (void)hipHostFree(c->up_pin[w][k]);
            if (c->up_ev[w][k]) (void)hipEventDestroy(c->up_ev[w][k]);
            c->up_pin[w][k] = nullptr; c->up_ev[w][k] = nullptr;
        }
        if (c->up_stream[w]) (void)hipStreamDestroy(c->up_stream[w]);
        c->up_stream[w] = nullptr;
    }
    c->up_ready = false;
}

// Copies every job to the device and returns when all bytes have landed.
int upload(vtx_ctx* c, const std::vector<UploadJob>& jobs, const std::atomic<bool>* cancel = nullptr) {
    struct Chunk { char* dst; const char* src; size_t bytes; };
    std::vector<Chunk> chunks;
    size_t total = 0;
    for (const UploadJob& j : jobs)
        for (size_t o = 0; o < j.bytes; o += vtx_ctx::kUpChunk) {
            chunks.push_back(Chunk{(char*)j.dst + o, (const char*)j.src + o, std::min(vtx_ctx::kUpChunk, j.bytes - o)});
            total += chunks.back().bytes;
        }
    if (chunks.empty()) return VTX_OK;
    if (total < (4u << 20)) {                    // small batches: not worth the threads
        for (const Chunk& ch : chunks) HIP_TRY(c, hipMemcpyAsync(ch.dst, ch.src, ch.bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return VTX_OK;
    }
    if (int rc = upload_init(c)) return rc;
    std::atomic<size_t> next{0};
    std::atomic<int> err{(int)hipSuccess};
    const int device = c->cfg.device;
    auto worker = [&](int w) {
        if (hipSetDevice(device) != hipSuccess) { err = (int)hipErrorInvalidDevice; return; }
        bool used[vtx_ctx::kUpSlots] = {};
        int slot = 0;
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= chunks.size() || err.load() != (int)hipSuccess) break;
            if (cancel && cancel->load()) { err = (int)hipErrorNotReady; break; }           // (vtx_prefetch_file: nobody wants the rest)
            hipError_t e = used[slot] ? hipEventSynchronize(c->up_ev[w][slot]) : hipSuccess;   // the DMA out of this buffer is done
            if (e == hipSuccess) {
                memcpy(c->up_pin[w][slot], chunks[i].src, chunks[i].bytes);
                e = hipMemcpyAsync(chunks[i].dst, c->up_pin[w][slot], chunks[i].bytes, hipMemcpyHostToDevice, c->up_stream[w]);
            }
            if (e == hipSuccess) e = hipEventRecord(c->up_ev[w][slot], c->up_stream[w]);
            if (e != hipSuccess) { err = (int)e; break; }
            used[slot] = true;
            slot = (slot + 1) % vtx_ctx::kUpSlots;
        }
        const hipError_t e = hipStreamSynchronize(c->up_stream[w]);
        if (e != hipSuccess) err = (int)e;
    };
    const int nw = (int)std::min<size_t>(vtx_ctx::kUpWorkers, chunks.size());
    std::vector<std::thread> th;
    for (int w = 1; w < nw; ++w) th.emplace_back(worker, w);
    worker(0);
    for (auto& t : th) t.join();
    if (err.load() != (int)hipSuccess)
        return fail(c, VTX_E_HIP, "upload: %s", hipGetErrorString((hipError_t)err.load()));
    return VTX_OK;
}

// vtx_prefetch_file's thread runs upload(): it uses the context's pinned buffers, events and copy streams, runs the lazy upload_init and
// writes c->err, all without a lock.  So every entry point that uploads, downloads through the copy workers or takes d_bam_comp calls
// this first — the ONE place the thread is waited for.  Keep: the prefetched bytes stay valid for a later vtx_submit_bam (the caller
// leaves d_bam_comp alone).  Drop: the caller is about to overwrite d_bam_comp.  Cancel: nobody wants the bytes — the copy stops at its
// next chunk instead of being waited for as a whole — and they are dropped.
enum class Prefetch { Keep, Drop, Cancel };
void prefetch_settle(vtx_ctx* c, Prefetch mode) {
    if (mode == Prefetch::Cancel) c->pf_cancel = true;
    if (c->pf_thread.joinable()) c->pf_thread.join();
    c->pf_cancel = false;
    if (mode != Prefetch::Keep) c->pf_valid = false;
}

// Gathers byte ranges of one host mapping (src) into ONE compact device buffer: piece k, the bytes at src + file_off, lands at
// dst + dst_off (dst_off ascending, pieces back to back: vtxp::Piece).  The destination is cut into kUpChunk chunks; a worker copies whatever pieces (or parts of them) fall into its chunk
// into its pinned buffer and pushes the chunk with one DMA — ten thousand segments of a sparse plan cost ten thousand memcpys on the
// host, not ten thousand DMAs.
int upload_gather(vtx_ctx* c, void* dst, const uint8_t* src, const std::vector<vtxp::Piece>& pieces) {
    if (pieces.empty()) return VTX_OK;
    const size_t total = (size_t)(pieces.back().dst_off + pieces.back().bytes);
    const size_t n_chunks = (total + vtx_ctx::kUpChunk - 1) / vtx_ctx::kUpChunk;
    if (!n_chunks) return VTX_OK;
    if (int rc = upload_init(c)) return rc;
    std::atomic<size_t> next{0};
    std::atomic<int> err{(int)hipSuccess};
    const int device = c->cfg.device;
    auto worker = [&](int w) {
        if (hipSetDevice(device) != hipSuccess) { err = (int)hipErrorInvalidDevice; return; }
        bool used[vtx_ctx::kUpSlots] = {};
        int slot = 0;
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= n_chunks || err.load() != (int)hipSuccess) break;
            const size_t lo = i * vtx_ctx::kUpChunk, hi = std::min(total, lo + vtx_ctx::kUpChunk);
            hipError_t e = used[slot] ? hipEventSynchronize(c->up_ev[w][slot]) : hipSuccess;   // the DMA out of this buffer is done
            if (e == hipSuccess) {
                // first piece that ends behind lo
                size_t k = (size_t)(std::upper_bound(pieces.begin(), pieces.end(), lo, [](size_t v, const vtxp::Piece& g) { return v < g.dst_off + g.bytes; }) - pieces.begin());
                for (; k < pieces.size() && pieces[k].dst_off < hi; ++k) {
                    const size_t a = std::max<size_t>(lo, pieces[k].dst_off), b = std::min<size_t>(hi, pieces[k].dst_off + pieces[k].bytes);
                    memcpy((char*)c->up_pin[w][slot] + (a - lo), src + pieces[k].file_off + (a - pieces[k].dst_off), b - a);
                }
                e = hipMemcpyAsync((char*)dst + lo, c->up_pin[w][slot], hi - lo, hipMemcpyHostToDevice, c->up_stream[w]);
            }
            if (e == hipSuccess) e = hipEventRecord(c->up_ev[w][slot], c->up_stream[w]);
            if (e != hipSuccess) { err = (int)e; break; }
            used[slot] = true;
            slot = (slot + 1) % vtx_ctx::kUpSlots;
        }
        const hipError_t e = hipStreamSynchronize(c->up_stream[w]);
        if (e != hipSuccess) err = (int)e;
    };
    const int nw = (int)std::min<size_t>(vtx_ctx::kUpWorkers, n_chunks);
    std::vector<std::thread> th;
    for (int w = 1; w < nw; ++w) th.emplace_back(worker, w);
    worker(0);
    for (auto& t : th) t.join();
    if (err.load() != (int)hipSuccess)
        return fail(c, VTX_E_HIP, "upload: %s", hipGetErrorString((hipError_t)err.load()));
    return VTX_OK;
}

// The way back: device arrays into the caller-visible (pageable, freshly allocated) host arrays.  Same workers and
// pinned buffers as the upload: a worker keeps one DMA in flight while it copies the previous chunk out of its other
// pinned buffer, so the page faults of the fresh host pages are spread over the workers.
int download(vtx_ctx* c, const std::vector<UploadJob>& jobs) {     // dst = host, src = device
    struct Chunk { char* dst; const char* src; size_t bytes; };
    std::vector<Chunk> chunks;
    size_t total = 0;
    for (const UploadJob& j : jobs)
        for (size_t o = 0; o < j.bytes; o += vtx_ctx::kUpChunk) {
            chunks.push_back(Chunk{(char*)j.dst + o, (const char*)j.src + o, std::min(vtx_ctx::kUpChunk, j.bytes - o)});
            total += chunks.back().bytes;
        }
    if (chunks.empty()) return VTX_OK;
    if (total < (4u << 20)) {
        for (const Chunk& ch : chunks) HIP_TRY(c, hipMemcpy(ch.dst, ch.src, ch.bytes, hipMemcpyDeviceToHost));
        return VTX_OK;
    }
    if (int rc = upload_init(c)) return rc;
    std::atomic<size_t> next{0};
    std::atomic<int> err{(int)hipSuccess};
    const int device = c->cfg.device;
    auto worker = [&](int w) {
        if (hipSetDevice(device) != hipSuccess) { err = (int)hipErrorInvalidDevice; return; }
        size_t held[vtx_ctx::kUpSlots];
        bool used[vtx_ctx::kUpSlots] = {};
        auto drain = [&](int slot) -> hipError_t {
            if (!used[slot]) return hipSuccess;
            used[slot] = false;
            const hipError_t e = hipEventSynchronize(c->up_ev[w][slot]);
            if (e == hipSuccess) memcpy(chunks[held[slot]].dst, c->up_pin[w][slot], chunks[held[slot]].bytes);
            return e;
        };
        int slot = 0;
        for (;;) {
            const size_t i = next.fetch_add(1);
            hipError_t e = drain(slot);
            if (e == hipSuccess && i < chunks.size() && err.load() == (int)hipSuccess) {
                e = hipMemcpyAsync(c->up_pin[w][slot], chunks[i].src, chunks[i].bytes, hipMemcpyDeviceToHost, c->up_stream[w]);
                if (e == hipSuccess) e = hipEventRecord(c->up_ev[w][slot], c->up_stream[w]);
                if (e == hipSuccess) { used[slot] = true; held[slot] = i; }
            } else {
                for (int k = 1; k < vtx_ctx::kUpSlots && e == hipSuccess; ++k) e = drain((slot + k) % vtx_ctx::kUpSlots);
                if (e != hipSuccess) err = (int)e;
                break;
            }
            if (e != hipSuccess) { err = (int)e; break; }
            slot = (slot + 1) % vtx_ctx::kUpSlots;
        }
        (void)hipStreamSynchronize(c->up_stream[w]);
    };
    const int nw = (int)std::min<size_t>(vtx_ctx::kUpWorkers, chunks.size());
    std::vector<std::thread> th;
    for (int w = 1; w < nw; ++w) th.emplace_back(worker, w);
    worker(0);
    for (auto& t : th) t.join();
    if (err.load() != (int)hipSuccess)
        return fail(c, VTX_E_HIP, "download: %s", hipGetErrorString((hipError_t)err.load()));
    return VTX_OK;
}

// Device bytes straight into a file: the copy workers pwrite() their pinned buffers at the chunk's file offset — one host copy (pinned
// buffer -> page cache), spread over the workers, instead of two (pinned -> caller's array -> page cache).
int download_to_fd(vtx_ctx* c, int fd, uint64_t file_off, const void* d_src, size_t bytes) {
    if (!bytes) return VTX_OK;
    if (int rc = upload_init(c)) return rc;
    const size_t n_chunks = (bytes + vtx_ctx::kUpChunk - 1) / vtx_ctx::kUpChunk;
    std::atomic<size_t> next{0};
    std::atomic<int> err{(int)hipSuccess};
    std::atomic<bool> io_err{false};
    const int device = c->cfg.device;
    auto worker = [&](int w) {
        if (hipSetDevice(device) != hipSuccess) { err = (int)hipErrorInvalidDevice; return; }
        size_t held[vtx_ctx::kUpSlots];
        bool used[vtx_ctx::kUpSlots] = {};
        auto drain = [&](int slot) -> hipError_t {
            if (!used[slot]) return hipSuccess;
            used[slot] = false;
            const hipError_t e = hipEventSynchronize(c->up_ev[w][slot]);
            if (e != hipSuccess) return e;
            const size_t o = held[slot] * vtx_ctx::kUpChunk, n = std::min(vtx_ctx::kUpChunk, bytes - o);
            const char* p = (const char*)c->up_pin[w][slot];
            size_t done = 0;
            while (done < n) {
                const ssize_t k = pwrite(fd, p + done, n - done, (off_t)(file_off + o + done));
                if (k <= 0) { io_err = true; break; }
                done += (size_t)k;
            }
            return hipSuccess;
        };
        int slot = 0;
        for (;;) {
            const size_t i = next.fetch_add(1);
            hipError_t e = drain(slot);
            if (e == hipSuccess && i < n_chunks && err.load() == (int)hipSuccess && !io_err.load()) {
                const size_t o = i * vtx_ctx::kUpChunk, n = std::min(vtx_ctx::kUpChunk, bytes - o);
                e = hipMemcpyAsync(c->up_pin[w][slot], (const char*)d_src + o, n, hipMemcpyDeviceToHost, c->up_stream[w]);
                if (e == hipSuccess) e = hipEventRecord(c->up_ev[w][slot], c->up_stream[w]);
                if (e == hipSuccess) { used[slot] = true; held[slot] = i; }
            } else {
                for (int k = 1; k < vtx_ctx::kUpSlots && e == hipSuccess; ++k) e = drain((slot + k) % vtx_ctx::kUpSlots);
                if (e != hipSuccess) err = (int)e;
                break;
            }
            if (e != hipSuccess) { err = (int)e; break; }
            slot = (slot + 1) % vtx_ctx::kUpSlots;
        }
        (void)hipStreamSynchronize(c->up_stream[w]);
    };
    const int nw = (int)std::min<size_t>(vtx_ctx::kUpWorkers, n_chunks);
    std::vector<std::thread> th;
    for (int w = 1; w < nw; ++w) th.emplace_back(worker, w);
    worker(0);
    for (auto& t : th) t.join();
    if (err.load() != (int)hipSuccess) return fail(c, VTX_E_HIP, "download: %s", hipGetErrorString((hipError_t)err.load()));
    if (io_err.load()) return fail(c, VTX_E_INVAL, "error writing the output file");
    return VTX_OK;
}

// the seven triplet arrays of n entries, device -> host
int fetch_arrays(vtx_ctx* c, size_t n, const void* row, const void* col, const void* alt, const void* ref, const void* unk,
                 const void* val, const void* refval, vtx_coo* out) {
    if (!c->h_row.alloc(n) || !c->h_col.alloc(n) || !c->h_alt.alloc(n) || !c->h_ref.alloc(n) || !c->h_unk.alloc(n) ||
        !c->h_val.alloc(n) || !c->h_refval.alloc(n))
        return fail(c, VTX_E_NOMEM, "out of host memory for %zu triplets", n);
    if (n) {
        if (int rc = download(c, {{c->h_row.data(), row, n * 4}, {c->h_col.data(), col, n * 4}, {c->h_alt.data(), alt, n * 4},
                                  {c->h_ref.data(), ref, n * 4}, {c->h_unk.data(), unk, n * 4}, {c->h_val.data(), val, n * 8},
                                  {c->h_refval.data(), refval, n * 8}}))
            return rc;
    }
    out->row = c->h_row.data(); out->col = c->h_col.data(); out->alt = c->h_alt.data(); out->ref = c->h_ref.data();
    out->unk = c->h_unk.data(); out->value = c->h_val.data(); out->ref_value = c->h_refval.data();
    out->nnz = n;
    return VTX_OK;
}

#ifdef VTX_DEVTOOLS
extern "C" void* vtxt_comm_test_table(void** fns);          // vtx_comm_test.hip (linked into libvtx_dev.so only)
#endif
// ---- RCCL, opened on first use ---------------------------------------------------------------------------------
struct Rccl {
    void* lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
};
Rccl* rccl() {
    static Rccl r;
    static std::once_flag once;          // vtx_comm_init is called from several threads at once (one context per GPU)
    std::call_once(once, [] {
#ifdef VTX_DEVTOOLS
        if (VTX_DEV_ENV("VTX_COMM_TEST_TRANSPORT")) {
            // TEST TRANSPORT (vtx_comm_test.hip, libvtx_dev.so only): ranks = processes that may share one device, payloads over Unix
            // sockets in that directory — the exchange's own logic with world > 1 on a one-GPU box.  Not in the production library.
            void* f[10];
            r.lib = vtxt_comm_test_table(f);
            r.GetUniqueId = (decltype(r.GetUniqueId))f[0]; r.CommInitRank = (decltype(r.CommInitRank))f[1];
            r.CommDestroy = (decltype(r.CommDestroy))f[2]; r.AllGather = (decltype(r.AllGather))f[3];
            r.Send = (decltype(r.Send))f[4]; r.Recv = (decltype(r.Recv))f[5]; r.GroupStart = (decltype(r.GroupStart))f[6];
            r.GroupEnd = (decltype(r.GroupEnd))f[7]; r.GetErrorString = (decltype(r.GetErrorString))f[8]; r.CommCount = (decltype(r.CommCount))f[9];
            return;
        }
#endif
        for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
            r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (r.lib) break;
        }
        if (r.lib) {
#define VTX_SYM(f) r.f = (decltype(r.f))dlsym(r.lib, "nccl" #f)
            VTX_SYM(GetUniqueId); VTX_SYM(CommInitRank); VTX_SYM(CommDestroy); VTX_SYM(AllGather); VTX_SYM(Send); VTX_SYM(Recv);
            VTX_SYM(GroupStart); VTX_SYM(GroupEnd); VTX_SYM(GetErrorString); VTX_SYM(CommCount);
#undef VTX_SYM
            if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllGather || !r.Send || !r.Recv || !r.GroupStart ||
                !r.GroupEnd || !r.GetErrorString) { dlclose(r.lib); r.lib = nullptr; }
        }
    });
    return r.lib ? &r : nullptr;
}
#define NCCL_TRY(c, expr)                                                                                   \
    do {                                                                                                    \
        ncclResult_t _r = (expr);                                                                           \
        if (_r != ncclSuccess) return fail((c), VTX_E_HIP, "%s: %s", #expr, rccl()->GetErrorString(_r));    \
    } while (0)

void comm_release(vtx_ctx* c) {
    if (c->comm && rccl()) (void)rccl()->CommDestroy(c->comm);
    c->comm = nullptr; c->comm_world = 0;
}

// d_bam_cnt: the ingest's VTXG_N_COUNTERS 64-bit counters (vtx_ingest.h), then four 32-bit words — the ingest's err[], the matrix
// writers' flag.  The ONE place that knows how the buffer is carved.
struct BamCounters {
    unsigned long long* counters;
    uint32_t* err;
    static constexpr size_t kBytes = VTXG_N_COUNTERS * sizeof(uint64_t) + 4 * sizeof(uint32_t);
};
int reserve_bam_counters(vtx_ctx* c, BamCounters* out) {
    HIP_TRY(c, c->d_bam_cnt.reserve(BamCounters::kBytes));
    out->counters = c->d_bam_cnt.as<unsigned long long>();
    out->err = (uint32_t*)(out->counters + VTXG_N_COUNTERS);
    return VTX_OK;
}

// per-record device buffers of the resident batch (scores, group structure, COO staging)
int reserve_record_buffers(vtx_ctx* c, uint32_t nr) {
    const size_t u32 = sizeof(uint32_t);
    HIP_TRY(c, c->d_records.reserve((size_t)nr * sizeof(vtx_record)));
    HIP_TRY(c, c->d_rec_locus.reserve(nr * u32));
    HIP_TRY(c, c->d_work.reserve(nr * u32));
    HIP_TRY(c, c->d_redo.reserve(nr * u32));
    HIP_TRY(c, c->d_redo_cnt.reserve(16 * u32));
    HIP_TRY(c, c->d_ref.reserve(nr * sizeof(int32_t)));
    HIP_TRY(c, c->d_alt.reserve(nr * sizeof(int32_t)));
    DevBuf* per_rec[] = {&c->d_head_cell, &c->d_head_umi, &c->d_cell_scan, &c->d_umi_scan, &c->d_grp_row, &c->d_grp_col,
                         &c->d_umi_cellgrp, &c->d_keep, &c->d_keep_scan, &c->d_o_row, &c->d_o_col, &c->d_o_alt,
                         &c->d_o_ref, &c->d_o_unk};
    for (DevBuf* d : per_rec) HIP_TRY(c, d->reserve(nr * u32));
    HIP_TRY(c, c->d_grp_start.reserve(((size_t)nr + 1) * u32));
    HIP_TRY(c, c->d_cell_cnt.reserve(3 * (size_t)nr * u32));
    HIP_TRY(c, c->d_umi_cnt.reserve(3 * (size_t)nr * u32));
    HIP_TRY(c, c->d_o_val.reserve(nr * sizeof(double)));
    HIP_TRY(c, c->d_o_refval.reserve(nr * sizeof(double)));
    HIP_TRY(c, c->d_scan_tmp.reserve(vtxk_scan_temp_bytes(nr)));
    return VTX_OK;
}

// (row, cell) / (row, cell, umi) group structure of the resident records: depends only on the records.
// Leaves the two group counts in flight on the stream (the caller synchronises).
int build_groups(vtx_ctx* c, uint32_t nr) {
    hipStream_t s = c->stream;
    const size_t tmp_bytes = vtxk_scan_temp_bytes(nr);
    c->n_cell_groups = c->n_umi_groups = 0;
    if (!nr) return VTX_OK;
    HIP_TRY(c, vtxk_group_heads(c->d_records.as<vtx_record>(), c->d_rec_locus.as<uint32_t>(), nr,
                                c->d_head_cell.as<uint32_t>(), c->d_head_umi.as<uint32_t>(), s));
    HIP_TRY(c, vtxk_inclusive_scan_u32(c->d_head_cell.as<uint32_t>(), c->d_cell_scan.as<uint32_t>(), nr, c->d_scan_tmp.p, tmp_bytes, s));
    HIP_TRY(c, vtxk_inclusive_scan_u32(c->d_head_umi.as<uint32_t>(), c->d_umi_scan.as<uint32_t>(), nr, c->d_scan_tmp.p, tmp_bytes, s));
    HIP_TRY(c, vtxk_group_table(c->d_records.as<vtx_record>(), c->d_rec_locus.as<uint32_t>(), c->d_loci.as<vtx_locus>(), nr,
                                c->d_head_cell.as<uint32_t>(), c->d_head_umi.as<uint32_t>(), c->d_cell_scan.as<uint32_t>(),
                                c->d_umi_scan.as<uint32_t>(), c->d_grp_row.as<uint32_t>(), c->d_grp_col.as<uint32_t>(),
                                c->d_umi_cellgrp.as<uint32_t>(), c->d_grp_start.as<uint32_t>(), s));
    HIP_TRY(c, hipMemcpyAsync(&c->n_cell_groups, c->d_cell_scan.as<uint32_t>() + (nr - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&c->n_umi_groups, c->d_umi_scan.as<uint32_t>() + (nr - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    return VTX_OK;
}

// tables per workgroup of the duo kernel for this haplotype length: as many as fit 52 KiB, at most kDuoLociCap
uint32_t duo_loci_cap(uint32_t max_hap) {
    const size_t table_bytes = ((size_t)std::max(max_hap, 16u) + 36) * 6 * 4;
    return (uint32_t)std::min<size_t>(kDuoLociCap, (52 * 1024) / table_bytes);
}

// pair-table mode of the duo kernel (deep data: a 32-record workgroup spans <= 2 loci): columns of the per-locus
// pair table (16 sentinels + prefix) that fit the same 52 KiB next to the two single tables; 0 = mode not available
const uint32_t kPairLociCap = 2;
uint32_t duo_pair_cols(uint32_t max_hap) {
    const size_t lcols = 16 + (size_t)std::max(max_hap, 16u) + 16 + 4;
    const size_t single = kPairLociCap * lcols * 6 * 4;
    if (single + kPairLociCap * (16 + 32) * 38 * 4 > 52 * 1024) return 0;
    const size_t fit = (52 * 1024 - single) / (kPairLociCap * 38 * 4);
    const size_t cols = std::min<size_t>(fit, 16 + (size_t)max_hap);
    // the shared prefix is about half of the haplotype (the padding): a pair table that cannot hold it would cut the
    // sharing short (T1 is clamped to the table), and the two-lookup mode is the better choice then
    return cols >= 16 + (size_t)max_hap / 2 + 4 ? (uint32_t)cols : 0u;
}

// Kernel choice per work list (one list per read-length shape, already in d_work): LUT / shared-prefix (duo) /
// pair-table eligibility is a property of how many loci a workgroup of consecutive list entries spans.
int make_buckets(vtx_ctx* c, const uint32_t* shape_cnt, uint32_t max_hap, uint32_t* d_lut_flag) {
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemsetAsync(d_lut_flag, 0, 48 * sizeof(uint32_t), s));
    c->buckets.clear();
    uint32_t off = 0;
    for (int sh = 0; sh < kNumShapes; ++sh) {
        if (!shape_cnt[sh]) continue;
        const bool lut = kShapes[sh][1] == 16 && (size_t)kLutLociCap * (max_hap + 36) * 6 * 4 <= 96 * 1024;
        const uint32_t dcap = duo_loci_cap(max_hap);
        const bool duo = kShapes[sh][1] == 16 && dcap >= 2;
        if (lut) HIP_TRY(c, vtxk_prep_lut_check(c->d_work.as<uint32_t>() + off, shape_cnt[sh], c->d_rec_locus.as<uint32_t>(), kLutLociCap, 16,
                                                d_lut_flag + c->buckets.size(), s));
        if (duo) HIP_TRY(c, vtxk_prep_lut_check(c->d_work.as<uint32_t>() + off, shape_cnt[sh], c->d_rec_locus.as<uint32_t>(), dcap, 32,
                                                d_lut_flag + 16 + c->buckets.size(), s));
        const bool pair = duo && duo_pair_cols(max_hap) != 0;
        if (pair) HIP_TRY(c, vtxk_prep_lut_check(c->d_work.as<uint32_t>() + off, shape_cnt[sh], c->d_rec_locus.as<uint32_t>(), kPairLociCap, 32,
                                                 d_lut_flag + 32 + c->buckets.size(), s));
        Bucket bk{kShapes[sh][0], kShapes[sh][1], off, shape_cnt[sh], lut};
        bk.duo = duo; bk.pair = pair;
        c->buckets.push_back(bk);
        off += shape_cnt[sh];
    }
    c->slow_off = off; c->slow_cnt = shape_cnt[kNumShapes];          // the slow list sorts last (shape index kNumShapes)
    uint32_t lut_flag[48] = {0};
    HIP_TRY(c, hipMemcpyAsync(lut_flag, d_lut_flag, sizeof lut_flag, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    for (size_t i = 0; i < c->buckets.size(); ++i) {
        if (lut_flag[i]) c->buckets[i].lut = false;
        if (lut_flag[16 + i]) c->buckets[i].duo = false;
        if (lut_flag[16 + i] || lut_flag[32 + i]) c->buckets[i].pair = false;
    }
    return VTX_OK;
}

using vtxp::bits_for;   // bits needed to represent values 0..max_value (vtx_prep_core.h)

}  // namespace

extern "C" {

void vtx_config_default(vtx_config* cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->abi_version = VTX_ABI_VERSION;
    cfg->device = 0;
    cfg->aligner = VTX_ALIGNER_BANDED;
    cfg->scoring_mode = VTX_MODE_CONSENSUS;
    cfg->use_umi = 0;
    cfg->match_score = 1;
    cfg->mismatch_score = -5;
    cfg->gap_open = -5;
    cfg->gap_extend = -1;
    cfg->min_score = 25;
    cfg->kmer_k = 6;
    cfg->band_w = 20;
}

int vtx_abi_sizes(uint32_t* out, uint32_t n) {
    const uint32_t s[17] = {(uint32_t)sizeof(vtx_config), (uint32_t)sizeof(vtx_locus), (uint32_t)sizeof(vtx_record),
                            (uint32_t)sizeof(vtx_batch), (uint32_t)sizeof(vtx_coo), (uint32_t)sizeof(vtx_timing),
                            (uint32_t)sizeof(vtx_raw_record), (uint32_t)sizeof(vtx_raw_batch), (uint32_t)sizeof(vtx_raw_stats),
                            (uint32_t)sizeof(vtx_bgzf_block), (uint32_t)sizeof(vtx_bam_interval), (uint32_t)sizeof(vtx_bam_ingest),
                            (uint32_t)sizeof(vtx_ingest_stats), (uint32_t)sizeof(vtx_bam_segment), (uint32_t)sizeof(vtx_bam_segments),
                            (uint32_t)sizeof(struct vtx_mtx_part), (uint32_t)sizeof(vtx_csr)};
    for (uint32_t i = 0; i < n && i < 17; ++i) out[i] = s[i];
    return VTX_ABI_VERSION;
}

uint32_t vtx_sizeof_csr_stats(void) { return (uint32_t)sizeof(vtx_csr_stats); }
uint32_t vtx_sizeof_geno_tally(void) { return (uint32_t)sizeof(vtx_geno_tally); }
uint32_t vtx_sizeof_geno_pair_tally(void) { return (uint32_t)sizeof(vtx_geno_pair_tally); }

const char* vtx_status_name(int status) {
    switch (status) {
    case VTX_OK: return "VTX_OK";
    case VTX_E_INVAL: return "VTX_E_INVAL";
    case VTX_E_NODEVICE: return "VTX_E_NODEVICE";
    case VTX_E_HIP: return "VTX_E_HIP";
    case VTX_E_NOMEM: return "VTX_E_NOMEM";
    case VTX_E_UNSUPPORTED: return "VTX_E_UNSUPPORTED";
    case VTX_E_STATE: return "VTX_E_STATE";
    case VTX_E_PEER: return "VTX_E_PEER";
    default: return "VTX_E_?";
    }
}

const char* vtx_strerror(const vtx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int vtx_create(const vtx_config* cfg, vtx_ctx** out) {
    if (!cfg || !out) return fail(nullptr, VTX_E_INVAL, "vtx_create: null argument");
    *out = nullptr;
    if (cfg->abi_version != VTX_ABI_VERSION)
        return fail(nullptr, VTX_E_INVAL, "vtx_create: abi_version %d != %d", cfg->abi_version, VTX_ABI_VERSION);
    if (cfg->aligner != VTX_ALIGNER_BANDED && cfg->aligner != VTX_ALIGNER_FULL)
        return fail(nullptr, VTX_E_INVAL, "vtx_create: unknown aligner %d", cfg->aligner);
    if (cfg->scoring_mode < VTX_MODE_CONSENSUS || cfg->scoring_mode > VTX_MODE_COVERAGE)
        return fail(nullptr, VTX_E_INVAL, "vtx_create: unknown scoring_mode %d", cfg->scoring_mode);
    // The kernels bake the reference's scoring constants (src/main.rs:33-38) in as immediates.
    if (cfg->match_score != VTX_REF_MATCH || cfg->mismatch_score != VTX_REF_MISMATCH || cfg->gap_open != VTX_REF_GAP_OPEN ||
        cfg->gap_extend != VTX_REF_GAP_EXTEND)
        return fail(nullptr, VTX_E_UNSUPPORTED,
                    "vtx_create: only the reference scoring (+1/-5, gap -5/-1; src/main.rs:35-38) is built");
    if (cfg->kmer_k != VTX_REF_K || cfg->band_w != VTX_REF_W)
        return fail(nullptr, VTX_E_UNSUPPORTED, "vtx_create: only K=6, W=20 (src/main.rs:33-34) is built");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, VTX_E_NODEVICE, "vtx_create: no HIP device (%s); this library has no CPU path",
                    e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, VTX_E_INVAL, "vtx_create: device %d out of range (%d devices)", cfg->device, ndev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess)
        return fail(nullptr, VTX_E_HIP, "vtx_create: hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, VTX_E_NODEVICE, "vtx_create: device %d is %s; kernels are built for gfx950 only",
                    cfg->device, prop.gcnArchName);
    vtx_ctx* c = new (std::nothrow) vtx_ctx();
    if (!c) return fail(nullptr, VTX_E_NOMEM, "vtx_create: out of host memory");
    c->cfg = *cfg;
    if (hipSetDevice(cfg->device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return fail(nullptr, VTX_E_HIP, "vtx_create: stream creation failed");
    }
    for (auto& ev : c->ev)
        if (hipEventCreate(&ev) != hipSuccess) { vtx_destroy(c); return fail(nullptr, VTX_E_HIP, "vtx_create: event creation failed"); }
    for (auto& ev : c->ev_crc)
        if (hipEventCreate(&ev) != hipSuccess) { vtx_destroy(c); return fail(nullptr, VTX_E_HIP, "vtx_create: event creation failed"); }
    *out = c;
    return VTX_OK;
}

void vtx_destroy(vtx_ctx* c) {
    if (!c) return;
    prefetch_settle(c, Prefetch::Keep);
    if (c->pf_map) { munmap(c->pf_map, c->pf_map_bytes); c->pf_map = nullptr; }
    (void)hipSetDevice(c->cfg.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    DevBuf* bufs[] = {&c->d_loci, &c->d_records, &c->d_rec_locus, &c->d_hap, &c->d_read, &c->d_work, &c->d_ref,
                      &c->d_alt, &c->d_head_cell, &c->d_head_umi, &c->d_cell_scan, &c->d_umi_scan, &c->d_grp_row,
                      &c->d_grp_col, &c->d_umi_cellgrp, &c->d_grp_start, &c->d_cell_cnt, &c->d_umi_cnt, &c->d_keep, &c->d_keep_scan,
                      &c->d_scan_tmp, &c->d_o_row, &c->d_o_col, &c->d_o_alt, &c->d_o_ref, &c->d_o_unk, &c->d_o_val,
                      &c->d_o_refval, &c->d_band_ws, &c->d_band_ws2, &c->d_band, &c->d_poly, &c->d_gtables, &c->d_hard, &c->d_over, &c->d_over2, &c->d_pend, &c->d_pend_buf, &c->d_band2, &c->d_hard2,
                      &c->d_cnt, &c->d_redo, &c->d_redo_cnt, &c->d_bc_slots, &c->d_bc_hash, &c->d_bc_off, &c->d_bc_bytes,
                      &c->d_raw, &c->d_tags, &c->d_raw_locus, &c->d_key_lc, &c->d_key_lc2, &c->d_key_umi, &c->d_key_umi2,
                      &c->d_idx, &c->d_idx2, &c->d_shape, &c->d_shape2, &c->d_seq, &c->d_locus_cnt, &c->d_locus_scan,
                      &c->d_prep_cnt, &c->d_sort_tmp, &c->d_fail, &c->d_fail_tmp, &c->d_refine, &c->d_tail, &c->d_recheck, &c->d_tight, &c->d_tight_pack, &c->d_dband, &c->d_dband_pack, &c->d_dense, &c->d_stage, &c->d_sweep_log, &c->d_tight2, &c->d_tight2_pack, &c->d_recheck2, &c->d_recheck2_pack};
    for (DevBuf* b : bufs) b->release();
    c->d_slow_ws.release(); c->d_slow_retry.release(); c->d_read_packed.release();
    c->csr.release();
    DevBuf* ib[] = {&c->d_bam_comp, &c->d_bam_data, &c->d_bam_blocks, &c->d_bam_seeds, &c->d_bam_seed_cnt, &c->d_bam_seed_scan, &c->d_bam_iv, &c->d_bam_cnt,
                    &c->d_bam_rec, &c->d_bam_nhit, &c->d_bam_rsz, &c->d_bam_tsz, &c->d_bam_hscan, &c->d_bam_rscan, &c->d_bam_tscan, &c->d_bam_info, &c->d_bam_segs};
    for (DevBuf* b : ib) b->release();
    DevBuf* gb[] = {&c->d_g_cnt, &c->d_g_row, &c->d_g_col, &c->d_g_alt, &c->d_g_ref, &c->d_g_unk, &c->d_g_val, &c->d_g_refval};
    for (DevBuf* b : gb) b->release();
    comm_release(c);
    upload_release(c);
    for (auto& ev : c->ev) if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : c->ev_crc) if (ev) (void)hipEventDestroy(ev);
    c->csr.destroy_events();
    if (c->h_pin) (void)hipHostFree(c->h_pin);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->ev2) (void)hipEventDestroy(c->ev2);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// Which loci of the batch have a haplotype above 255 bases (and within the fast kernels' limit)?  One of them used to put the WHOLE batch
// on round 3's path (four-byte match entries, no sweep, no second stage); vtx_run now scores them in a pass of their own (round 6).
static void note_long_loci(vtx_ctx* c, const vtx_locus* loci, uint32_t nl) {
    c->hap_short_max = c->n_long_loci = c->long_first = c->long_last = 0;
    for (uint32_t l = 0; l < nl; ++l) {
        const uint32_t hl = std::max(loci[l].ref_len, loci[l].alt_len);
        if (hl <= 255) c->hap_short_max = std::max(c->hap_short_max, hl);
        else if (hl <= kFastHapLen) {
            if (!c->n_long_loci++) c->long_first = l;
            c->long_last = l;
        }
    }
}

// ---- buffers of the banded stage -------------------------------------------------------------------------------
// One launch covers every task unless a test hook asks for chunks.  The scratch of band_run_kernel belongs to its
// RESIDENT lanes (persistent workgroups).  Hard tasks leave band_run_kernel / band_pending_kernel as compact staircase
// records (192 B); the masked DP expands them into band slots (2 x band_stride u16) one slice of `slots` tasks at a
// time.  A quarter of the tasks may be hard (noisy reads: 11 % at 3 % substitution errors) before anything spills to
// the general kernel's list.  gt_bytes: the k-mer tables of every locus in global memory (0: tables in LDS).
// records band_diag_kernel may leave for band_refine_kernel per chunk of tasks (a quarter of the tasks: 22 % are listed at 8 %
// substitution errors; what does not fit goes to band_run_kernel as before)
// (round 6: with a tight list EVERY task that leaves band_diag_kernel with a certificate leaves a record, for band_corridor_kernel: 24 - 30 %
// of the tasks at 8 % errors (39 % measured: 19.1 M of 48.6 M) — half; a task that does not fit takes the masked DP over its band, as all of them did before)
static uint32_t band_refine_cap(uint32_t chunk) { return std::max(65536u, chunk / 2); }
// records band_diag_kernel may leave for band_tail_kernel per chunk (tasks whose generic set grows: 8 % of a clean workload's tasks; a
// task that does not fit finishes in its wavefront).  128 bytes each; no room for them (the buffer is optional): every task stays.
static uint32_t band_tail_cap(uint32_t chunk) { return std::max(65536u, chunk / 4); }
// records band_diag_kernel may leave for the recheck per chunk (tasks that fail its coarse harmless test; the tail's record, 128 bytes).
// Measured on the host mirror (profiles/r16_recheck_census.txt): 0.08 % of the headline's tasks, 0.6 % at 3 % substitution errors,
// 2.1 % at 8 % — one task in 32 (3.1 %) is one and a half times the noisiest of them: 190 MB on the headline's 48.6 M tasks.  A task that finds no slot
// leaves as before (W_NOT_HARMLESS: the sweep), and so does every task when the buffer cannot be had.
static uint32_t band_recheck_cap(uint32_t chunk) { return std::max(16384u, chunk / 32); }
struct BandPlan {
    uint64_t n_tasks = 0;
    uint32_t chunk = 0, band_stride = 0, hard_cap = 0, pend_cap = 0, slots = 0, poly_stride = 0, tasks_per_locus = 0;
    size_t gt_bytes = 0;
    uint32_t gt_loci = 0;      // loci the table buffer holds (< n_loci: the stage runs in chunks of tasks whose loci fit)
};
static BandPlan band_plan(uint32_t nr, uint32_t n_loci, uint32_t max_hap_len) {
    BandPlan p;
    p.n_tasks = 2ull * nr;
    uint64_t chunk_cap = 1u << 31;
    if (VTX_DEV_ENV("VTX_BAND_CHUNK")) chunk_cap = std::max<uint64_t>(256, strtoull(VTX_DEV_ENV("VTX_BAND_CHUNK"), nullptr, 10));   // test hook
    p.chunk = (uint32_t)std::min<uint64_t>(p.n_tasks, chunk_cap);
    p.band_stride = (max_hap_len + 2 + 7) & ~7u;
    p.hard_cap = (uint32_t)std::min<uint64_t>(p.chunk, p.chunk / 4 + (1u << 20));
    p.pend_cap = (uint32_t)std::min<uint64_t>(p.chunk, p.chunk / 8 + (1u << 20));
    p.slots = (uint32_t)std::min<uint64_t>(p.chunk, p.chunk / 16 + (1u << 20));
    if (VTX_DEV_ENV("VTX_BAND_HARD_CAP")) p.hard_cap = p.pend_cap = p.slots = std::max(1u, (uint32_t)atoi(VTX_DEV_ENV("VTX_BAND_HARD_CAP")));   // test hook
    if (VTX_DEV_ENV("VTX_BAND_SLOTS")) p.slots = std::max(1u, (uint32_t)atoi(VTX_DEV_ENV("VTX_BAND_SLOTS")));                                  // test hook
    p.poly_stride = vtxk_band_poly_stride();
    p.tasks_per_locus = (uint32_t)(p.n_tasks / std::max(n_loci, 1u));
    p.gt_bytes = vtxk_band_gtables_bytes(n_loci, max_hap_len, p.tasks_per_locus, &p.gt_loci);
    if (p.gt_bytes && p.gt_loci < n_loci) {
        // chunks of tasks spanning about half the loci the buffer holds (loci differ in depth; a chunk whose loci do not
        // fit after all takes the LDS-table kernel)
        const uint64_t t = std::max<uint64_t>(4096, (uint64_t)p.gt_loci * std::max(p.tasks_per_locus, 1u) / 2);
        p.chunk = (uint32_t)std::min<uint64_t>(p.chunk, t & ~63ull);
        p.hard_cap = std::min(p.hard_cap, p.chunk); p.pend_cap = std::min(p.pend_cap, p.chunk); p.slots = std::min(p.slots, p.chunk);
    }
    return p;
}
// (hipMalloc of these GBs costs ~0.1 s the first time a context runs.  Doing it on a helper thread during the upload of
// vtx_submit was tried: hipMalloc stalls the copy workers, the submit got slower by more than the run got faster.)
static int band_reserve(vtx_ctx* c, BandPlan& p, bool quiet) {
#define RES(buf, bytes)                                                                             \
    do {                                                                                            \
        const hipError_t e_ = c->buf.reserve(bytes);                                                \
        if (e_ != hipSuccess) {                                                                     \
            if (quiet) { (void)hipGetLastError(); return VTX_E_HIP; }                               \
            return fail(c, e_ == hipErrorOutOfMemory ? VTX_E_NOMEM : VTX_E_HIP, "banded stage buffers: %s", hipGetErrorString(e_)); \
        }                                                                                           \
    } while (0)
    RES(d_band_ws, (size_t)vtxk_band_run_lanes() * vtxk_band_task_words() * sizeof(uint32_t));       // per resident lane
    if (p.gt_bytes && c->d_gtables.reserve(p.gt_bytes) != hipSuccess) {     // no room for them: the LDS-table kernels need none
        (void)hipGetLastError();
        p.gt_bytes = 0;
    }
    RES(d_pend, (size_t)p.pend_cap * sizeof(uint32_t));
    RES(d_pend_buf, (size_t)p.pend_cap * vtxk_band_pend_words() * sizeof(uint32_t));
    RES(d_poly, ((size_t)p.hard_cap + p.pend_cap) * p.poly_stride * sizeof(uint16_t));
    RES(d_band, (size_t)p.slots * 2 * p.band_stride * sizeof(uint16_t));
    RES(d_hard, ((size_t)p.hard_cap + p.pend_cap) * sizeof(uint32_t));
    RES(d_over, 4 * (size_t)p.n_tasks * sizeof(uint32_t));   // [0, 2n): band_run_kernel's overflows and their second-chance appends; [2n, 4n): what band_sweep_kernel declines (its own region: the appends of an overflowing chunk cannot reach it)
    RES(d_cnt, sizeof(vtx_band_counters));
    if (p.gt_bytes) RES(d_fail, 2 * (size_t)p.chunk * sizeof(uint32_t));  // tasks band_diag_kernel leaves to band_run_kernel (as listed, then sorted)
    if (p.gt_bytes) RES(d_refine, (size_t)band_refine_cap(p.chunk) * vtxk_band_refine_words() * sizeof(uint32_t));   // records for band_refine_kernel
    if (p.gt_bytes && c->d_tail.reserve((size_t)band_tail_cap(p.chunk) * vtxk_band_tail_words() * sizeof(uint32_t)) != hipSuccess) {
        (void)hipGetLastError();                                                                          // records for band_tail_kernel
        c->d_tail.release();
    }
    if (p.gt_bytes && c->d_recheck.reserve((size_t)band_recheck_cap(p.chunk) * vtxk_band_tail_words() * sizeof(uint32_t)) != hipSuccess) {
        (void)hipGetLastError();                                                                          // records for the recheck
        c->d_recheck.release();
    }
    if (p.gt_bytes) RES(d_tight, (size_t)p.chunk * sizeof(uint32_t));       // tasks with a certificate but no verdict ...
    if (p.gt_bytes) RES(d_tight_pack, (size_t)p.chunk * sizeof(uint32_t));  // ... and their bands (one diagonal stretch each: one word)
    if (p.gt_bytes) RES(d_dense, 2 * (size_t)p.chunk * sizeof(uint32_t));   // tasks for band_sweep_kernel (repeats: as listed, then sorted)
    if (p.gt_bytes) RES(d_sweep_log, vtxk_band_sweep_log_bytes());
    if (p.gt_bytes) RES(d_tight2, (size_t)p.chunk * sizeof(uint32_t));      // second stage: one-diagonal bands ...
    if (p.gt_bytes) RES(d_tight2_pack, (size_t)p.chunk * sizeof(uint32_t)); // ... one word each
    if (p.gt_bytes) RES(d_recheck2, (size_t)p.chunk * sizeof(uint32_t));
    if (p.gt_bytes) RES(d_recheck2_pack, (size_t)p.chunk * sizeof(uint32_t));
#undef RES
    return VTX_OK;
}

int vtx_submit(vtx_ctx* c, const vtx_batch* b) {
    if (!c) return VTX_E_INVAL;
    prefetch_settle(c, Prefetch::Keep);                   // (upload() below; d_bam_comp is not touched: the bytes stay good for a later vtx_submit_bam)
    if (!b) return fail(c, VTX_E_INVAL, "vtx_submit: null batch");
    c->submitted = false; c->ran = false;
    const uint32_t nl = b->n_loci, nr = b->n_records;
    if ((nl && !b->loci) || (nr && !b->records) || (b->hap_bytes && !b->hap_arena) || (b->read_bytes && !b->read_arena))
        return fail(c, VTX_E_INVAL, "vtx_submit: null array with non-zero count");
    if (b->hap_bytes > 0xffffffffull || b->read_bytes > 0xffffffffull)
        return fail(c, VTX_E_UNSUPPORTED, "vtx_submit: arenas above 4 GiB need more than one batch");

    // ---- loci: validated on the host (O(loci)); everything per record happens on the device ----
    uint32_t next_rec = 0, max_hap = 0, max_hap_all = 0;
    for (uint32_t l = 0; l < nl; ++l) {
        const vtx_locus& L = b->loci[l];
        if (L.rec_begin != next_rec) return fail(c, VTX_E_INVAL, "vtx_submit: locus %u: records not contiguous (rec_begin %u, expected %u)", l, L.rec_begin, next_rec);
        if ((uint64_t)L.rec_begin + L.rec_count > nr) return fail(c, VTX_E_INVAL, "vtx_submit: locus %u: record range exceeds n_records", l);
        if ((uint64_t)L.ref_off + L.ref_len > b->hap_bytes || (uint64_t)L.alt_off + L.alt_len > b->hap_bytes)
            return fail(c, VTX_E_INVAL, "vtx_submit: locus %u: haplotype outside hap_arena", l);
        if (L.ref_len > kMaxHapLen || L.alt_len > kMaxHapLen)
            return fail(c, VTX_E_UNSUPPORTED, "vtx_submit: locus %u: haplotype longer than %u", l, kMaxHapLen);
        const uint32_t hl = std::max(L.ref_len, L.alt_len);
        max_hap_all = std::max(max_hap_all, hl);
        if (hl <= kFastHapLen) max_hap = std::max(max_hap, hl);      // LDS tables are sized for the loci the fast kernels take
        next_rec = L.rec_begin + L.rec_count;
    }
    if (next_rec != nr) return fail(c, VTX_E_INVAL, "vtx_submit: %u records not covered by any locus", nr - next_rec);
    note_long_loci(c, b->loci, nl);

    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t u32 = sizeof(uint32_t), u64 = sizeof(uint64_t);
    HIP_TRY(c, c->d_loci.reserve((size_t)nl * sizeof(vtx_locus)));
    HIP_TRY(c, c->d_hap.reserve(b->hap_bytes + 16));
    HIP_TRY(c, c->d_read.reserve(b->read_bytes + 16));
    const bool nibbles = c->read_format == VTX_READS_NIBBLES;
    if (nibbles && (b->read_bytes & 1)) return fail(c, VTX_E_INVAL, "vtx_submit: VTX_READS_NIBBLES needs an even read_bytes");
    if (nibbles) HIP_TRY(c, c->d_read_packed.reserve(b->read_bytes / 2 + 16));
    if (int rc = reserve_record_buffers(c, nr)) return rc;
    HIP_TRY(c, c->d_seq.reserve(nr * u32));
    HIP_TRY(c, c->d_shape.reserve(nr + 16));
    HIP_TRY(c, c->d_shape2.reserve(nr + 16));
    HIP_TRY(c, c->d_prep_cnt.reserve(8 * u64 + 64 * u32));
    const size_t sort_tmp = vtxk_prep_sort_temp_bytes(nr);
    HIP_TRY(c, c->d_sort_tmp.reserve(std::max(sort_tmp, vtxk_scan_temp_bytes(std::max(nr, nl)))));
    unsigned long long* d_counters = c->d_prep_cnt.as<unsigned long long>();
    uint32_t* d_shape_cnt = (uint32_t*)(d_counters + 8);
    uint32_t caps[kNumShapes];
    for (int i = 0; i < kNumShapes; ++i) caps[i] = (uint32_t)(kShapes[i][0] * kShapes[i][1]);
    HIP_TRY(c, vtxk_prep_set_shapes(caps, kNumShapes, kFastReadLen, kFastHapLen));

    // ---- feed: descriptors first, then the record checks run on the device while the read bases still stream in ----
    hipStream_t s = c->stream;
    if (int rc = upload(c, {{c->d_loci.p, b->loci, (size_t)nl * sizeof(vtx_locus)},
                            {c->d_records.p, b->records, (size_t)nr * sizeof(vtx_record)},
                            {c->d_hap.p, b->hap_arena, (size_t)b->hap_bytes}})) return rc;
    unsigned long long cnt[8] = {0};
    uint32_t shape_cnt[16] = {0};
    HIP_TRY(c, hipMemsetAsync(c->d_prep_cnt.p, 0, 8 * u64 + 64 * u32, s));
    HIP_TRY(c, hipMemsetAsync(d_counters + 6, 0xff, u64, s));                       // "no offending record"
    if (nr) {
        HIP_TRY(c, vtxk_prep_rec_locus(c->d_loci.as<vtx_locus>(), nl, c->d_rec_locus.as<uint32_t>(), s));
        HIP_TRY(c, vtxk_prep_check(c->d_records.as<vtx_record>(), nr, c->d_rec_locus.as<uint32_t>(), c->d_loci.as<vtx_locus>(),
                                   b->read_bytes, kMaxReadLen | (nibbles ? 0x80000000u : 0u), c->cfg.n_barcodes, c->cfg.use_umi ? 1 : 0, kNumShapes, c->d_shape.as<uint8_t>(),
                                   c->d_seq.as<uint32_t>(), d_shape_cnt, d_counters, s));
        // work lists per kernel shape: stable sort of the record numbers by shape
        HIP_TRY(c, vtxk_prep_sort_u8(c->d_shape.as<uint8_t>(), c->d_shape2.as<uint8_t>(), c->d_seq.as<uint32_t>(),
                                     c->d_work.as<uint32_t>(), nr, c->d_sort_tmp.p, sort_tmp, s));
    }
    HIP_TRY(c, hipMemcpyAsync(cnt, d_counters, 8 * u64, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(shape_cnt, d_shape_cnt, sizeof shape_cnt, hipMemcpyDeviceToHost, s));
    if (nibbles) {
        if (int rc = upload(c, {{c->d_read_packed.p, b->read_arena, (size_t)(b->read_bytes / 2)}})) return rc;
        HIP_TRY(c, vtxk_unpack_nibbles(c->d_read_packed.as<uint8_t>(), b->read_bytes / 2, c->d_read.as<uint8_t>(), s));
    } else if (int rc = upload(c, {{c->d_read.p, b->read_arena, (size_t)b->read_bytes}})) return rc;     // overlaps with the kernels above
    HIP_TRY(c, hipStreamSynchronize(s));
    if (cnt[6] != ~0ull) {
        const uint32_t r = (uint32_t)(cnt[6] >> 3), code = (uint32_t)(cnt[6] & 7);
        const vtx_record& R = b->records[r];
        if (code == 1) return fail(c, VTX_E_INVAL, "vtx_submit: record %u: read outside read_arena", r);
        if (code == 2) return fail(c, VTX_E_UNSUPPORTED, "vtx_submit: record %u: read length %u above %u", r, R.read_len, kMaxReadLen);
        if (code == 3) return fail(c, VTX_E_INVAL, "vtx_submit: record %u: cell_index %u >= n_barcodes %u", r, R.cell_index, c->cfg.n_barcodes);
        if (code == 5) return fail(c, VTX_E_INVAL, "vtx_submit: record %u: read_off %u is odd (VTX_READS_NIBBLES: every read starts at an even base)", r, R.read_off);
        return fail(c, VTX_E_INVAL, "vtx_submit: record %u: not sorted by %s within its locus", r, c->cfg.use_umi ? "(cell_index, umi_id)" : "cell_index");
    }
    if (int rc = make_buckets(c, shape_cnt, max_hap, d_shape_cnt + 16)) return rc;
    if (int rc = build_groups(c, nr)) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    c->n_loci = nl; c->n_records = nr; c->max_hap_len = max_hap; c->max_read_len = (uint32_t)cnt[5]; c->cells = cnt[3];
    c->max_hap_all = max_hap_all; c->max_read_all = std::max<uint32_t>((uint32_t)cnt[7], std::max<uint32_t>((uint32_t)cnt[5], 1u));
    c->submitted = true;
    // the banded stage's buffers (a few GB for a config-3 batch) now, not inside the first vtx_run of the context: a drop-in CLI
    // calls vtx_run ONCE per batch, and 0.1 s of hipMalloc inside it was two thirds of that call.  Best effort: vtx_run reserves
    // again (a no-op when this succeeded) and reports a failure there.
    if (c->cfg.aligner == VTX_ALIGNER_BANDED && c->n_records) {
        BandPlan bp = band_plan(c->n_records, c->n_loci, c->max_hap_len);
        (void)band_reserve(c, bp, true);
    }
    return VTX_OK;
}

int vtx_set_barcodes(vtx_ctx* c, const uint8_t* bytes, const uint64_t* offsets, uint32_t n) {
    if (!c) return VTX_E_INVAL;
    if (!offsets || (n && !bytes && offsets[n] > offsets[0])) return fail(c, VTX_E_INVAL, "vtx_set_barcodes: null argument");
    if (c->cfg.n_barcodes == 0) c->cfg.n_barcodes = n;          // a context created before the list was read (cfg.n_barcodes 0) takes its width from it
    if (n != c->cfg.n_barcodes) return fail(c, VTX_E_INVAL, "vtx_set_barcodes: %u barcodes, cfg.n_barcodes is %u", n, c->cfg.n_barcodes);
    c->bc_ready = false;
    for (uint32_t j = 0; j < n; ++j) {
        if (offsets[j + 1] < offsets[j]) return fail(c, VTX_E_INVAL, "vtx_set_barcodes: offsets not ascending at %u", j);
        if (offsets[j + 1] - offsets[j] >= VTX_TAG_MISSING) return fail(c, VTX_E_UNSUPPORTED, "vtx_set_barcodes: barcode %u longer than 65534 bytes", j);
    }
    // open addressing, load <= 1/2; slot = index + 1, 0 = empty.  Duplicated byte strings keep the first index (:704-710).
    const uint32_t cap = vtxp::table_capacity(n);
    std::vector<uint32_t> slots(cap, 0);
    std::vector<uint64_t> hashes(std::max(n, 1u));
    vtxp::table_build(bytes, offsets, n, cap, slots.data(), hashes.data());
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const uint64_t nbytes = n ? offsets[n] : 0;
    HIP_TRY(c, c->d_bc_slots.reserve(cap * sizeof(uint32_t)));
    HIP_TRY(c, c->d_bc_hash.reserve(hashes.size() * sizeof(uint64_t)));
    HIP_TRY(c, c->d_bc_off.reserve(((size_t)n + 1) * sizeof(uint64_t)));
    HIP_TRY(c, c->d_bc_bytes.reserve(nbytes + 16));
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemcpyAsync(c->d_bc_slots.p, slots.data(), cap * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->d_bc_hash.p, hashes.data(), hashes.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->d_bc_off.p, offsets, ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    if (nbytes) HIP_TRY(c, hipMemcpyAsync(c->d_bc_bytes.p, bytes, nbytes, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    c->bc_mask = cap - 1;
    c->bc_ready = true;
    return VTX_OK;
}

// ---- raw batches: what vtx_submit_raw and vtx_submit_bam share ----
// device buffers of a raw batch of nr records over nl loci (the arenas: d_read / d_read_packed, d_tags; the records: d_raw, d_raw_locus)
static int raw_reserve(vtx_ctx* c, uint32_t nl, uint32_t nr, uint64_t hap_bytes, uint64_t read_bytes, uint64_t tag_bytes, bool nibbles) {
    const size_t u32 = sizeof(uint32_t), u64 = sizeof(uint64_t);
    HIP_TRY(c, c->d_loci.reserve((size_t)nl * sizeof(vtx_locus)));
    HIP_TRY(c, c->d_hap.reserve(hap_bytes + 16));
    HIP_TRY(c, c->d_read.reserve(read_bytes + 16));
    if (nibbles) HIP_TRY(c, c->d_read_packed.reserve(read_bytes / 2 + 16));
    HIP_TRY(c, c->d_tags.reserve(tag_bytes + 16));
    HIP_TRY(c, c->d_raw.reserve((size_t)nr * sizeof(vtx_raw_record)));
    if (int rc = reserve_record_buffers(c, nr)) return rc;
    DevBuf* k64[] = {&c->d_key_lc, &c->d_key_lc2, &c->d_key_umi, &c->d_key_umi2};
    for (DevBuf* d : k64) HIP_TRY(c, d->reserve(nr * u64));
    DevBuf* k32[] = {&c->d_raw_locus, &c->d_idx, &c->d_idx2, &c->d_seq};
    for (DevBuf* d : k32) HIP_TRY(c, d->reserve(nr * u32));
    HIP_TRY(c, c->d_shape.reserve(nr + 16));
    HIP_TRY(c, c->d_shape2.reserve(nr + 16));
    HIP_TRY(c, c->d_locus_cnt.reserve(((size_t)nl + 1) * u32));
    HIP_TRY(c, c->d_locus_scan.reserve(((size_t)nl + 1) * u32));
    HIP_TRY(c, c->d_prep_cnt.reserve(8 * u64 + 64 * u32));
    const size_t sort_tmp = vtxk_prep_sort_temp_bytes(nr);
    HIP_TRY(c, c->d_sort_tmp.reserve(std::max(sort_tmp, vtxk_scan_temp_bytes(std::max(nr, nl)))));
    uint32_t caps[kNumShapes];
    for (int i = 0; i < kNumShapes; ++i) caps[i] = (uint32_t)(kShapes[i][0] * kShapes[i][1]);
    HIP_TRY(c, vtxk_prep_set_shapes(caps, kNumShapes, kFastReadLen, kFastHapLen));
    return VTX_OK;
}

// Barcode lookup, UB test, UMI grouping and the sort by (locus, cell, UMI) of the nr raw records resident in d_raw / d_tags (their
// bases in d_read), then the work lists and the group structure: the state vtx_submit leaves.  locus_from_loci: d_raw_locus is derived
// from the loci's record ranges (vtx_submit_raw: records grouped by locus); otherwise the caller filled it (vtx_submit_bam: records in
// BAM order, a locus per record — the sort's key does not care).
static int raw_prepare(vtx_ctx* c, uint32_t nl, uint32_t nr, uint64_t read_bytes, uint64_t tag_bytes, bool nibbles, uint32_t max_hap,
                       uint32_t max_hap_all, bool locus_from_loci, vtx_raw_stats* stats) {
    hipStream_t s = c->stream;
    const size_t u32 = sizeof(uint32_t), u64 = sizeof(uint64_t);
    const size_t sort_tmp = vtxk_prep_sort_temp_bytes(nr);
    unsigned long long* d_counters = c->d_prep_cnt.as<unsigned long long>();
    uint32_t* d_shape_cnt = (uint32_t*)(d_counters + 8);
    uint32_t* d_lut_flag = d_shape_cnt + 16;
    HIP_TRY(c, hipEventRecord(c->ev[EV_PREP_START], s));
    const uint32_t cell_bits = vtxp::cell_bits_of(c->cfg.n_barcodes);
    const int end_bit = (int)vtxp::end_bit_of(cell_bits, nl);
    if (end_bit > 64) return fail(c, VTX_E_UNSUPPORTED, "raw batch: loci x barcodes exceed a 64-bit sort key");
    const int use_umi = c->cfg.use_umi ? 1 : 0;
    unsigned long long cnt[8] = {0};
    uint32_t n_kept = 0, rounds = 0;
    // test hook: the first N rounds hash every UMI to 0, so that the collision check and the re-seed are exercised
    const uint32_t weak_rounds = VTX_DEV_ENV("VTX_PREP_WEAK_ROUNDS") ? (uint32_t)atoi(VTX_DEV_ENV("VTX_PREP_WEAK_ROUNDS")) : 0;
    if (nr && locus_from_loci) HIP_TRY(c, vtxk_prep_rec_locus(c->d_loci.as<vtx_locus>(), nl, c->d_raw_locus.as<uint32_t>(), s));
    for (uint64_t seed = vtxp::UMI_SEED0;; seed = vtxp::next_seed(seed)) {
        ++rounds;
        HIP_TRY(c, hipMemsetAsync(c->d_prep_cnt.p, 0, 8 * u64 + 64 * u32, s));
        HIP_TRY(c, hipMemsetAsync(c->d_locus_cnt.p, 0, ((size_t)nl + 1) * u32, s));      // first record of each locus
        HIP_TRY(c, hipMemsetAsync(c->d_locus_scan.p, 0, ((size_t)nl + 1) * u32, s));     // one past its last record
        HIP_TRY(c, vtxk_prep_resolve(c->d_raw.as<vtx_raw_record>(), nr, c->d_raw_locus.as<uint32_t>(), c->d_tags.as<uint8_t>(),
                                     tag_bytes, read_bytes, kMaxReadLen | (nibbles ? 0x80000000u : 0u), c->d_bc_slots.as<uint32_t>(), c->bc_mask,
                                     c->d_bc_hash.as<uint64_t>(), c->d_bc_off.as<uint64_t>(), c->d_bc_bytes.as<uint8_t>(),
                                     use_umi, seed, rounds <= weak_rounds ? 0ull : ~0ull, cell_bits, nl, c->d_key_lc.as<uint64_t>(), c->d_key_umi.as<uint64_t>(),
                                     c->d_idx.as<uint32_t>(), d_counters, s));
        HIP_TRY(c, hipMemcpyAsync(cnt, d_counters, 3 * u64, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        if (cnt[2]) return fail(c, VTX_E_INVAL, "raw batch: a record points outside its arena, is longer than %u bases, or (VTX_READS_NIBBLES) starts at an odd base", kMaxReadLen);
        n_kept = nr - (uint32_t)cnt[0] - (uint32_t)cnt[1];
        // stable LSD order: UMI hash first, then (locus, cell); dropped records carry the largest key and end up last
        const uint32_t* perm = nullptr;
        const uint64_t* key_sorted = nullptr;
        if (use_umi) {
            HIP_TRY(c, vtxk_prep_sort_u64(c->d_key_umi.as<uint64_t>(), c->d_key_umi2.as<uint64_t>(), c->d_idx.as<uint32_t>(),
                                          c->d_idx2.as<uint32_t>(), nr, 64, c->d_sort_tmp.p, sort_tmp, s));
            HIP_TRY(c, vtxk_prep_gather_u64(c->d_key_lc.as<uint64_t>(), c->d_idx2.as<uint32_t>(), nr, c->d_key_lc2.as<uint64_t>(), s));
            HIP_TRY(c, vtxk_prep_sort_u64(c->d_key_lc2.as<uint64_t>(), c->d_key_umi2.as<uint64_t>(), c->d_idx2.as<uint32_t>(),
                                          c->d_idx.as<uint32_t>(), nr, end_bit, c->d_sort_tmp.p, sort_tmp, s));
            perm = c->d_idx.as<uint32_t>(); key_sorted = c->d_key_umi2.as<uint64_t>();
        } else {
            HIP_TRY(c, vtxk_prep_sort_u64(c->d_key_lc.as<uint64_t>(), c->d_key_lc2.as<uint64_t>(), c->d_idx.as<uint32_t>(),
                                          c->d_idx2.as<uint32_t>(), nr, end_bit, c->d_sort_tmp.p, sort_tmp, s));
            perm = c->d_idx2.as<uint32_t>(); key_sorted = c->d_key_lc2.as<uint64_t>();
        }
        HIP_TRY(c, vtxk_prep_finalize(n_kept, perm, key_sorted, c->d_key_umi.as<uint64_t>(), c->d_raw.as<vtx_raw_record>(),
                                      c->d_tags.as<uint8_t>(), c->d_loci.as<vtx_locus>(), cell_bits, use_umi, kNumShapes,
                                      c->d_records.as<vtx_record>(), c->d_rec_locus.as<uint32_t>(), c->d_head_umi.as<uint32_t>(),
                                      c->d_shape.as<uint8_t>(), c->d_seq.as<uint32_t>(), c->d_locus_cnt.as<uint32_t>(),
                                      c->d_locus_scan.as<uint32_t>(), d_shape_cnt, d_counters, s));
        HIP_TRY(c, hipMemcpyAsync(cnt, d_counters, 8 * u64, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        if (!cnt[4]) break;                  // no UMI hash collision inside a (locus, cell) group
        if (rounds == vtxp::UMI_MAX_ROUNDS) return fail(c, VTX_E_STATE, "raw batch: UMI hash collisions with 8 different seeds");
    }
    const size_t scan_tmp = vtxk_scan_temp_bytes(std::max(nr, nl));
    // dense UMI group numbers; per-locus record ranges of the kept, sorted records
    if (n_kept) {
        HIP_TRY(c, vtxk_inclusive_scan_u32(c->d_head_umi.as<uint32_t>(), c->d_umi_scan.as<uint32_t>(), n_kept, c->d_sort_tmp.p, scan_tmp, s));
        HIP_TRY(c, vtxk_prep_umi_ids(c->d_records.as<vtx_record>(), c->d_umi_scan.as<uint32_t>(), n_kept, s));
    }
    if (nl) {
        HIP_TRY(c, vtxk_prep_locus_counts(c->d_locus_cnt.as<uint32_t>(), c->d_locus_scan.as<uint32_t>(), nl, s));
        HIP_TRY(c, vtxk_inclusive_scan_u32(c->d_locus_cnt.as<uint32_t>(), c->d_locus_scan.as<uint32_t>(), nl, c->d_sort_tmp.p, scan_tmp, s));
        HIP_TRY(c, vtxk_prep_locus_ranges(c->d_loci.as<vtx_locus>(), c->d_locus_cnt.as<uint32_t>(), c->d_locus_scan.as<uint32_t>(), nl, s));
    }
    // work lists per kernel shape: stable sort of the record numbers by shape
    HIP_TRY(c, vtxk_prep_sort_u8(c->d_shape.as<uint8_t>(), c->d_shape2.as<uint8_t>(), c->d_seq.as<uint32_t>(), c->d_work.as<uint32_t>(),
                                 n_kept, c->d_sort_tmp.p, sort_tmp, s));
    uint32_t shape_cnt[16] = {0};
    HIP_TRY(c, hipMemcpyAsync(shape_cnt, d_shape_cnt, sizeof shape_cnt, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (int rc = make_buckets(c, shape_cnt, max_hap, d_lut_flag)) return rc;
    if (int rc = build_groups(c, n_kept)) return rc;
    HIP_TRY(c, hipEventRecord(c->ev[EV_PREP_END], s));
    HIP_TRY(c, hipStreamSynchronize(s));
    float ms = 0;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[EV_PREP_START], c->ev[EV_PREP_END]));
    c->n_loci = nl; c->n_records = n_kept; c->max_hap_len = max_hap; c->max_read_len = (uint32_t)cnt[5]; c->cells = cnt[3];
    c->max_hap_all = max_hap_all; c->max_read_all = std::max<uint32_t>((uint32_t)cnt[7], std::max<uint32_t>((uint32_t)cnt[5], 1u));
    c->submitted = true;
    // the banded stage's buffers (a few GB for a config-3 batch) now, not inside the first vtx_run of the context: a drop-in CLI
    // calls vtx_run ONCE per batch, and 0.1 s of hipMalloc inside it was two thirds of that call.  Best effort: vtx_run reserves
    // again (a no-op when this succeeded) and reports a failure there.
    if (c->cfg.aligner == VTX_ALIGNER_BANDED && c->n_records) {
        BandPlan bp = band_plan(c->n_records, c->n_loci, c->max_hap_len);
        (void)band_reserve(c, bp, true);
    }
    if (stats) {
        stats->num_not_cell_bc = cnt[0]; stats->num_non_umi = cnt[1]; stats->kept = n_kept; stats->prep_ms = ms;
        stats->hash_rounds = rounds;
    }
    return VTX_OK;
}

// loci of a raw batch, host side: haplotypes inside the arena and within the limits; *max_hap: the longest one the fast kernels take
static int check_loci_haps(vtx_ctx* c, const char* who, const vtx_locus* loci, uint32_t nl, uint64_t hap_bytes, uint32_t* max_hap, uint32_t* max_hap_all) {
    *max_hap = *max_hap_all = 0;
    for (uint32_t l = 0; l < nl; ++l) {
        const vtx_locus& L = loci[l];
        if ((uint64_t)L.ref_off + L.ref_len > hap_bytes || (uint64_t)L.alt_off + L.alt_len > hap_bytes)
            return fail(c, VTX_E_INVAL, "%s: locus %u: haplotype outside hap_arena", who, l);
        if (L.ref_len > kMaxHapLen || L.alt_len > kMaxHapLen)
            return fail(c, VTX_E_UNSUPPORTED, "%s: locus %u: haplotype longer than %u", who, l, kMaxHapLen);
        const uint32_t hl = std::max(L.ref_len, L.alt_len);
        *max_hap_all = std::max(*max_hap_all, hl);
        if (hl <= kFastHapLen) *max_hap = std::max(*max_hap, hl);
    }
    return VTX_OK;
}

int vtx_submit_raw(vtx_ctx* c, const vtx_raw_batch* b, vtx_raw_stats* stats) {
    if (!c) return VTX_E_INVAL;
    prefetch_settle(c, Prefetch::Keep);                   // (as in vtx_submit)
    if (!b) return fail(c, VTX_E_INVAL, "vtx_submit_raw: null batch");
    c->submitted = false; c->ran = false;
    if (!c->bc_ready) return fail(c, VTX_E_STATE, "vtx_submit_raw: no barcode list (vtx_set_barcodes)");
    const uint32_t nl = b->n_loci, nr = b->n_records;
    if ((nl && !b->loci) || (nr && !b->records) || (b->hap_bytes && !b->hap_arena) || (b->read_bytes && !b->read_arena) ||
        (b->tag_bytes && !b->tag_arena))
        return fail(c, VTX_E_INVAL, "vtx_submit_raw: null array with non-zero count");
    if (b->hap_bytes > 0xffffffffull || b->read_bytes > 0xffffffffull || b->tag_bytes > 0xffffffffull)
        return fail(c, VTX_E_UNSUPPORTED, "vtx_submit_raw: arenas above 4 GiB need more than one batch");
    // loci: host validation is O(loci); everything per record happens on the device
    uint32_t next_rec = 0, max_hap = 0, max_hap_all = 0;
    for (uint32_t l = 0; l < nl; ++l) {
        const vtx_locus& L = b->loci[l];
        if (L.rec_begin != next_rec) return fail(c, VTX_E_INVAL, "vtx_submit_raw: locus %u: records not contiguous (rec_begin %u, expected %u)", l, L.rec_begin, next_rec);
        if ((uint64_t)L.rec_begin + L.rec_count > nr) return fail(c, VTX_E_INVAL, "vtx_submit_raw: locus %u: record range exceeds n_records", l);
        next_rec = L.rec_begin + L.rec_count;
    }
    if (next_rec != nr) return fail(c, VTX_E_INVAL, "vtx_submit_raw: %u records not covered by any locus", nr - next_rec);
    if (int rc = check_loci_haps(c, "vtx_submit_raw", b->loci, nl, b->hap_bytes, &max_hap, &max_hap_all)) return rc;
    note_long_loci(c, b->loci, nl);

    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    const bool nibbles = c->read_format == VTX_READS_NIBBLES;
    if (nibbles && (b->read_bytes & 1)) return fail(c, VTX_E_INVAL, "vtx_submit_raw: VTX_READS_NIBBLES needs an even read_bytes");
    if (int rc = raw_reserve(c, nl, nr, b->hap_bytes, b->read_bytes, b->tag_bytes, nibbles)) return rc;
    if (int rc = upload(c, {{c->d_loci.p, b->loci, (size_t)nl * sizeof(vtx_locus)},
                            {c->d_raw.p, b->records, (size_t)nr * sizeof(vtx_raw_record)},
                            {c->d_hap.p, b->hap_arena, (size_t)b->hap_bytes},
                            {c->d_tags.p, b->tag_arena, (size_t)b->tag_bytes},
                            {nibbles ? c->d_read_packed.p : c->d_read.p, b->read_arena, (size_t)(nibbles ? b->read_bytes / 2 : b->read_bytes)}})) return rc;
    if (nibbles) HIP_TRY(c, vtxk_unpack_nibbles(c->d_read_packed.as<uint8_t>(), b->read_bytes / 2, c->d_read.as<uint8_t>(), s));
    return raw_prepare(c, nl, nr, b->read_bytes, b->tag_bytes, nibbles, max_hap, max_hap_all, true, stats);
}

// ---- vtx_prefetch_file: the BAM's bytes start travelling before anybody knows which of them matter ----
int vtx_prefetch_file(vtx_ctx* c, const char* path, uint64_t file_off, uint64_t n) {
    if (!c) return VTX_E_INVAL;
    if (!path) return fail(c, VTX_E_INVAL, "vtx_prefetch_file: null argument");
    prefetch_settle(c, Prefetch::Drop);
    if (c->pf_map) { munmap(c->pf_map, c->pf_map_bytes); c->pf_map = nullptr; }
    const int fd = open(path, O_RDONLY);
    struct stat st;
    if (fd < 0 || fstat(fd, &st) != 0) { if (fd >= 0) close(fd); return fail(c, VTX_E_INVAL, "vtx_prefetch_file: cannot open %s", path); }
    if (file_off > (uint64_t)st.st_size) file_off = (uint64_t)st.st_size;
    if (n == 0 || file_off + n > (uint64_t)st.st_size) n = (uint64_t)st.st_size - file_off;
    if (!n) { close(fd); return VTX_OK; }
    if (hipSetDevice(c->cfg.device) != hipSuccess || c->d_bam_comp.reserve((size_t)n + kBamPad) != hipSuccess) { close(fd); return fail(c, VTX_E_NOMEM, "vtx_prefetch_file: no device memory for %llu bytes", (unsigned long long)n); }
    // the copy workers read the file through a mapping of their own (measured against pread() into the pinned buffers at config-3 scale:
    // the same 80 - 200 ms beside the host's planning threads, and the mapping showed no multi-second outliers)
    const uint64_t map_off = file_off & ~(uint64_t)4095;
    void* mp = mmap(nullptr, (size_t)(file_off - map_off + n), PROT_READ, MAP_PRIVATE, fd, (off_t)map_off);
    close(fd);
    if (mp == MAP_FAILED) return fail(c, VTX_E_INVAL, "vtx_prefetch_file: cannot map %s", path);
    c->pf_map = mp; c->pf_map_bytes = (size_t)(file_off - map_off + n);
    c->pf_off = file_off; c->pf_n = n; c->pf_rc = VTX_OK; c->pf_valid = true;
    void* dst = c->d_bam_comp.p;
    const uint8_t* src = (const uint8_t*)mp + (file_off - map_off);
    c->pf_thread = std::thread([c, dst, src, n] {
        if (hipSetDevice(c->cfg.device) != hipSuccess) { c->pf_rc = VTX_E_HIP; return; }
        const auto t0 = std::chrono::steady_clock::now();
        c->pf_rc = upload(c, {{dst, src, (size_t)n}}, &c->pf_cancel);
        c->pf_ms = (float)(1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    });
    return VTX_OK;
}

// ---- vtx_submit_bam: the ingest itself on the device (vtx_ingest.hip) ----
// sg == nullptr: one contiguous stretch (vtx_submit_bam).  Else the segmented plan of vtx_submit_bam_segments: g = &sg->base holds the
// segments' blocks and seeds back to back; only the segments' byte ranges travel, and the record chains end per segment.
// The ingest runs as the stages below, in the order ingest_run lists them, over one IngestState.
struct IngestState {
    const vtx_bam_ingest* g = nullptr;
    const vtx_bam_segments* sg = nullptr;
    vtx_ingest_stats* st = nullptr;
    vtxp::Layout L;                                    // the plan in the device's layout (vtx_ingest_plan_core.h)
    uint32_t max_hap = 0, max_hap_all = 0;             // check_loci_haps
    bool prefetched = false;                           // the compressed bytes are a vtx_prefetch_file's, already in d_bam_comp
    float pf_wait_ms = 0, h2d_ms = 0;
    vtxp::IntervalArrays d_iv{};                       // L.iv on the device
    BamCounters d_cnt{};
    const vtxg_segment* d_segs = nullptr;              // segmented: the segment table, then the seeds' segment numbers
    const uint32_t* d_seed_seg = nullptr;
    uint32_t n_rec = 0;                                // BAM records the chains found
    uint32_t err[3] = {0, 0, 0};                       // the err words as last read back
    unsigned long long cnt[VTXG_N_COUNTERS] = {0};     // the counters after the filters' first pass
};

static float ms_since(std::chrono::steady_clock::time_point t) { return (float)(1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count()); }

// the slicing width of bgzf_crc32_kernel (experiment knob: 4 / 8 / 16)
static int crc_width() {
    static const int w = VTX_DEV_ENV("VTX_CRC_WIDTH") ? atoi(VTX_DEV_ENV("VTX_CRC_WIDTH")) : VTXG_CRC_WIDTH;
    return w;
}

// what the err words say, most specific first
static int ingest_error(vtx_ctx* c, const IngestState& is) {
    const uint32_t e0 = is.err[0], e1 = is.err[1];
    if (!(e0 & (0x1ffu | VTXG_ERR_CRC | VTXG_ERR_CHAIN)) && (e0 & VTXG_ERR_SEG_END))
        return fail(c, VTX_E_UNSUPPORTED, "vtx_submit_bam_segments: %u of %u segments cannot prove their end (the record the index names there starts in front of the segment's last locus: a read spliced over four windows): the host packer decides", is.err[2], is.sg ? is.sg->n_segments : 0u);
    if (e0 & 0x1ffu) return fail(c, VTX_E_UNSUPPORTED, "vtx_submit_bam: BGZF block %u does not inflate on the device (status bits 0x%x): the host packer decides", e1, e0 & 0x1ffu);
    if (e0 & VTXG_ERR_CRC) return fail(c, VTX_E_UNSUPPORTED, "vtx_submit_bam: BGZF block %u: the CRC32 of its inflated bytes does not match its trailer: the host packer decides", e1);
    if (e0 & VTXG_ERR_CHAIN) return fail(c, VTX_E_UNSUPPORTED, "vtx_submit_bam: a record chain does not end on the index's next record start (index and file disagree, or a malformed record)");
    return fail(c, VTX_E_UNSUPPORTED, "vtx_submit_bam: malformed BAM record");
}

// The caller's plan: checked, then rewritten into the device's layout.  The order of the checks is the API's: the barcode list, null
// arrays and the hap arena's size (the core), the loci's haplotypes, then everything else about the plan (the core again).
static int ingest_check_layout(vtx_ctx* c, IngestState& is) {
    const vtx_bam_ingest* g = is.g;
    c->submitted = false; c->ran = false;
    if (is.st) memset(is.st, 0, sizeof *is.st);
    if (!c->bc_ready) return fail(c, VTX_E_STATE, "vtx_submit_bam: no barcode list (vtx_set_barcodes)");
    char why[512];
    if (int rc = vtxp::check_arrays(*g, why, sizeof why)) return fail(c, rc, "%s", why);
    if (int rc = check_loci_haps(c, "vtx_submit_bam", g->loci, g->n_loci, g->hap_bytes, &is.max_hap, &is.max_hap_all)) return rc;
    note_long_loci(c, g->loci, g->n_loci);
    if (int rc = vtxp::layout(*g, is.sg, is.L, why, sizeof why)) return fail(c, rc, "%s", why);
    return VTX_OK;
}

// bytes a vtx_prefetch_file already brought (or is still bringing) to the device?
// (Tried in round 6: inflating the blocks of a 128 MB segment as soon as it has landed, on streams of their own.  Every launch of
//  the latency-bound inflate kernel takes its full ~35 ms whatever the block count, and the copies still in flight queued behind
//  the kernels: inflate 94 -> 250 ms, the copy 0.09 -> 1.4 s.  The copy is waited for as a whole.)
static void ingest_settle_prefetch(vtx_ctx* c, IngestState& is) {
    const vtxp::Layout& L = is.L;
    const auto t_pf = std::chrono::steady_clock::now();
    // (a segmented plan has no use for the file as a whole: the prefetch stops at its next chunk and its bytes are dropped)
    prefetch_settle(c, is.sg ? Prefetch::Cancel : Prefetch::Keep);
    is.pf_wait_ms = ms_since(t_pf);
    is.prefetched = !is.sg && c->pf_valid && c->pf_rc == VTX_OK && is.g->n_blocks && c->pf_off <= L.lo && L.hi + vtxp::kTrailer <= c->pf_off + c->pf_n;
    if (is.prefetched) { const uint64_t shift = L.lo - c->pf_off; for (auto& B : is.L.blocks) B.coff += shift; }
    else c->pf_valid = false;                          // (d_bam_comp is about to take this plan's own bytes)
}

// every buffer the stages up to the record count need, and the typed pointers into the shared ones
static int ingest_reserve(vtx_ctx* c, IngestState& is) {
    const vtx_bam_ingest* g = is.g;
    const vtxp::Layout& L = is.L;
    const size_t u32 = sizeof(uint32_t), u64 = sizeof(uint64_t);
    const uint32_t ns = g->n_seeds;
    if (!is.prefetched) HIP_TRY(c, c->d_bam_comp.reserve((size_t)L.comp_bytes + kBamPad));
    if (is.sg) HIP_TRY(c, c->d_bam_segs.reserve(L.segs.size() * sizeof(vtxg_segment) + (size_t)ns * sizeof(uint32_t) + 64));
    HIP_TRY(c, c->d_bam_data.reserve((size_t)L.utotal + kBamPad));
    HIP_TRY(c, c->d_bam_blocks.reserve((size_t)g->n_blocks * sizeof(vtxg_block)));
    HIP_TRY(c, c->d_bam_seeds.reserve((size_t)ns * u64));
    HIP_TRY(c, c->d_bam_seed_cnt.reserve((size_t)ns * u32 + 16));
    HIP_TRY(c, c->d_bam_seed_scan.reserve((size_t)ns * u32 + 16));
    HIP_TRY(c, c->d_bam_iv.reserve(L.iv.size() * u32 + 64));
    if (int rc = reserve_bam_counters(c, &is.d_cnt)) return rc;
    HIP_TRY(c, c->d_scan_tmp.reserve(vtxk_scan_temp_bytes(std::max(ns, 1u))));
    HIP_TRY(c, c->d_hap.reserve(g->hap_bytes + 16));
    HIP_TRY(c, c->d_loci.reserve((size_t)g->n_loci * sizeof(vtx_locus)));
    is.d_iv = vtxp::IntervalArrays{c->d_bam_iv.as<uint32_t>(), g->n_intervals, g->n_ref};
    // segment table, then the seeds' segment numbers (8-byte aligned: the table's entries are 40 bytes)
    is.d_segs = c->d_bam_segs.as<vtxg_segment>();
    is.d_seed_seg = (const uint32_t*)(is.d_segs + L.segs.size());
    return VTX_OK;
}

// the counters and err words zeroed; then the plan and the file's bytes (unless a prefetch brought them) to the device
static int ingest_upload(vtx_ctx* c, IngestState& is) {
    const vtx_bam_ingest* g = is.g;
    const vtxp::Layout& L = is.L;
    hipStream_t s = c->stream;
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(c, hipMemsetAsync(is.d_cnt.counters, 0, BamCounters::kBytes, s));
    HIP_TRY(c, hipMemsetAsync(is.d_cnt.err + 1, 0xff, sizeof(uint32_t), s));
    if (is.sg) {
        if (int rc = upload_gather(c, c->d_bam_comp.p, g->file, L.pieces)) return rc;
        if (int rc = upload(c, {{c->d_bam_segs.p, L.segs.data(), L.segs.size() * sizeof(vtxg_segment)},
                                {(void*)is.d_seed_seg, L.seed_seg.data(), L.seed_seg.size() * sizeof(uint32_t)}})) return rc;
    }
    if (int rc = upload(c, {{c->d_bam_comp.p, g->file + L.lo, is.prefetched || is.sg ? (size_t)0 : (size_t)L.comp_bytes},
                            {c->d_bam_blocks.p, L.blocks.data(), L.blocks.size() * sizeof(vtxg_block)},
                            {c->d_bam_seeds.p, g->seeds, (size_t)g->n_seeds * sizeof(uint64_t)},
                            {c->d_bam_iv.p, L.iv.data(), L.iv.size() * sizeof(uint32_t)},
                            {c->d_loci.p, g->loci, (size_t)g->n_loci * sizeof(vtx_locus)},
                            {c->d_hap.p, g->hap_arena, (size_t)g->hap_bytes}})) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    is.h2d_ms = ms_since(t0);
    return VTX_OK;
}

// ---- inflate; then the CRC32 of every block's inflated bytes against its trailer (htslib's check in bgzf_read_block): in front of
//      the first reader of those bytes, on the same stream, its verdict in the same err words ----
static int ingest_inflate_crc(vtx_ctx* c, IngestState& is) {
    hipStream_t s = c->stream;
    const uint32_t nb = is.g->n_blocks;
    HIP_TRY(c, hipEventRecord(c->ev[EV_INGEST_START], s));
    HIP_TRY(c, vtxg_inflate(c->d_bam_comp.as<uint8_t>(), c->d_bam_blocks.as<vtxg_block>(), nb, c->d_bam_data.as<uint8_t>(), is.d_cnt.err, nullptr, 0, s));
    HIP_TRY(c, hipEventRecord(c->ev[EV_INFLATE_END], s));
    HIP_TRY(c, hipEventRecord(c->ev_crc[0], s));
    HIP_TRY(c, vtxg_crc32(c->d_bam_comp.as<uint8_t>(), c->d_bam_blocks.as<vtxg_block>(), nb, c->d_bam_data.as<uint8_t>(), is.d_cnt.err, nullptr, 0, crc_width(), s));
    HIP_TRY(c, hipEventRecord(c->ev_crc[1], s));
    c->crc_ms = 0;
    return VTX_OK;
}

// One pass of the record chains, a chain per seed.  off == nullptr: the records of every chain are counted into d_bam_seed_cnt; else
// (off = the inclusive scan of those counts) their offsets go to rec_upos.
static int ingest_chain_pass(vtx_ctx* c, const IngestState& is, const uint32_t* off, uint64_t* rec_upos) {
    const uint8_t* data = c->d_bam_data.as<uint8_t>();
    const uint64_t* seeds = c->d_bam_seeds.as<uint64_t>();
    uint32_t* cnt = c->d_bam_seed_cnt.as<uint32_t>();
    const uint32_t ns = is.g->n_seeds;
    if (is.sg) HIP_TRY(c, vtxg_chain_segments(data, seeds, ns, is.d_seed_seg, is.d_segs, cnt, off, rec_upos, is.d_cnt.err, c->stream));
    else HIP_TRY(c, vtxg_chain(data, is.L.utotal, seeds, ns, is.L.end_upos, cnt, off, rec_upos, is.d_cnt.err, c->stream));
    return VTX_OK;
}

// ---- record boundaries: count per seed, scan, (the first verdict on the blocks and the chains,) emit ----
static int ingest_chains(vtx_ctx* c, IngestState& is) {
    hipStream_t s = c->stream;
    const size_t u32 = sizeof(uint32_t);
    const uint32_t ns = is.g->n_seeds;
    if (ns) {
        if (int rc = ingest_chain_pass(c, is, nullptr, nullptr)) return rc;
        HIP_TRY(c, vtxk_inclusive_scan_u32(c->d_bam_seed_cnt.as<uint32_t>(), c->d_bam_seed_scan.as<uint32_t>(), ns, c->d_scan_tmp.p, vtxk_scan_temp_bytes(ns), s));
        HIP_TRY(c, hipMemcpyAsync(&is.n_rec, c->d_bam_seed_scan.as<uint32_t>() + (ns - 1), u32, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipMemcpyAsync(is.err, is.d_cnt.err, 3 * u32, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (is.err[0]) return ingest_error(c, is);
    const uint32_t n_rec = is.n_rec;
    if ((uint64_t)n_rec > 0xfffffff0ull) return fail(c, VTX_E_UNSUPPORTED, "vtx_submit_bam: more than 2^32 BAM records in one ingest");
    HIP_TRY(c, c->d_bam_rec.reserve((size_t)n_rec * sizeof(uint64_t) + 16));
    DevBuf* per_rec[] = {&c->d_bam_nhit, &c->d_bam_rsz, &c->d_bam_tsz, &c->d_bam_hscan, &c->d_bam_rscan, &c->d_bam_tscan};
    for (DevBuf* d : per_rec) HIP_TRY(c, d->reserve((size_t)n_rec * u32 + 16));
    HIP_TRY(c, c->d_bam_info.reserve((size_t)n_rec * sizeof(vtxg_recinfo) + 16));
    HIP_TRY(c, c->d_scan_tmp.reserve(vtxk_scan_temp_bytes(std::max(n_rec, 1u))));
    if (ns) { if (int rc = ingest_chain_pass(c, is, c->d_bam_seed_scan.as<uint32_t>(), c->d_bam_rec.as<uint64_t>())) return rc; }
    HIP_TRY(c, hipEventRecord(c->ev[EV_INDEX_END], s));
    return VTX_OK;
}

// One pass of the fetch + filters per (read, locus) pair.  emit == 0: the counts per record and the counters; emit == 1 (behind the
// scans of the counts): the raw records, their loci, the tag and read arenas.
static int ingest_scan_pass(vtx_ctx* c, const IngestState& is, int emit) {
    const vtx_bam_ingest* g = is.g;
    const vtxg_filter f{g->n_ref, g->min_mapq, g->primary_only ? 1u : 0u, g->no_duplicates ? 1u : 0u, (uint32_t)(uint8_t)g->bam_tag[0] | ((uint32_t)(uint8_t)g->bam_tag[1] << 8)};
    const vtxp::IntervalArrays& iv = is.d_iv;
    HIP_TRY(c, vtxg_scan(emit, c->d_bam_data.as<uint8_t>(), c->d_bam_rec.as<uint64_t>(), is.n_rec, f, iv.start(), iv.end(), iv.locus(), iv.tid_begin(), iv.tid_span(),
                         c->d_bam_nhit.as<uint32_t>(), c->d_bam_rsz.as<uint32_t>(), c->d_bam_tsz.as<uint32_t>(), c->d_bam_info.as<vtxg_recinfo>(),
                         emit ? c->d_bam_hscan.as<uint32_t>() : nullptr, emit ? c->d_bam_rscan.as<uint32_t>() : nullptr, emit ? c->d_bam_tscan.as<uint32_t>() : nullptr,
                         emit ? c->d_raw.as<vtx_raw_record>() : nullptr, emit ? c->d_raw_locus.as<uint32_t>() : nullptr, emit ? c->d_tags.as<uint8_t>() : nullptr,
                         emit ? c->d_read_packed.as<uint8_t>() : nullptr, is.d_cnt.counters, is.d_cnt.err, c->stream));
    return VTX_OK;
}

// ---- fetch + filters per (read, locus) pair: counts, then offsets, then the raw records ----
static int ingest_filter(vtx_ctx* c, IngestState& is) {
    hipStream_t s = c->stream;
    const uint32_t n_rec = is.n_rec;
    if (int rc = ingest_scan_pass(c, is, 0)) return rc;
    HIP_TRY(c, hipMemcpyAsync(is.cnt, is.d_cnt.counters, sizeof is.cnt, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(is.err, is.d_cnt.err, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (is.err[0]) return ingest_error(c, is);
    const uint64_t read_bases = is.cnt[6], tag_bytes = is.cnt[7], n_pairs = is.cnt[8];
    if (read_bases > 0xF0000000ull || tag_bytes > 0xF0000000ull || n_pairs > 0x7fffffffull)
        return fail(c, VTX_E_UNSUPPORTED, "vtx_submit_bam: the reads of this range need more than one batch (%llu bases, %llu tag bytes, %llu pairs): pack ranges of loci",
                    (unsigned long long)read_bases, (unsigned long long)tag_bytes, (unsigned long long)n_pairs);
    if (int rc = raw_reserve(c, is.g->n_loci, (uint32_t)n_pairs, is.g->hap_bytes, read_bases, tag_bytes, true)) return rc;
    if (n_rec) {
        const size_t tb = vtxk_scan_temp_bytes(n_rec);
        HIP_TRY(c, vtxk_inclusive_scan_u32(c->d_bam_nhit.as<uint32_t>(), c->d_bam_hscan.as<uint32_t>(), n_rec, c->d_scan_tmp.p, tb, s));
        HIP_TRY(c, vtxk_inclusive_scan_u32(c->d_bam_rsz.as<uint32_t>(), c->d_bam_rscan.as<uint32_t>(), n_rec, c->d_scan_tmp.p, tb, s));
        HIP_TRY(c, vtxk_inclusive_scan_u32(c->d_bam_tsz.as<uint32_t>(), c->d_bam_tscan.as<uint32_t>(), n_rec, c->d_scan_tmp.p, tb, s));
        if (int rc = ingest_scan_pass(c, is, 1)) return rc;
    }
    HIP_TRY(c, vtxk_unpack_nibbles(c->d_read_packed.as<uint8_t>(), read_bases / 2, c->d_read.as<uint8_t>(), s));
    HIP_TRY(c, hipEventRecord(c->ev[EV_FILTER_END], s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return VTX_OK;
}

// the stages' device times, the preparation every raw batch goes through (raw_prepare), and the statistics
static int ingest_publish(vtx_ctx* c, const IngestState& is) {
    const uint64_t read_bases = is.cnt[6], tag_bytes = is.cnt[7];
    const uint32_t nr = (uint32_t)is.cnt[8];
    float inflate_ms = 0, index_ms = 0, filter_ms = 0;
    HIP_TRY(c, hipEventElapsedTime(&inflate_ms, c->ev[EV_INGEST_START], c->ev[EV_INFLATE_END]));
    HIP_TRY(c, hipEventElapsedTime(&c->crc_ms, c->ev_crc[0], c->ev_crc[1]));
    HIP_TRY(c, hipEventElapsedTime(&index_ms, c->ev_crc[1], c->ev[EV_INDEX_END]));
    HIP_TRY(c, hipEventElapsedTime(&filter_ms, c->ev[EV_INDEX_END], c->ev[EV_FILTER_END]));
    c->bam_n_rec = is.n_rec; c->bam_n_raw = nr; c->bam_utotal = is.L.utotal; c->bam_read_bases = read_bases; c->bam_tag_bytes = tag_bytes;
    vtx_raw_stats rs{};
    if (int rc = raw_prepare(c, is.g->n_loci, nr, read_bases, tag_bytes, true, is.max_hap, is.max_hap_all, false, &rs)) return rc;
    if (vtx_ingest_stats* st = is.st) {
        st->num_reads = is.cnt[0]; st->num_low_mapq = is.cnt[1]; st->num_non_primary = is.cnt[2]; st->num_duplicates = is.cnt[3];
        st->num_not_useful = is.cnt[4]; st->num_no_barcode_tag = is.cnt[5];
        st->bam_records = is.n_rec; st->raw_records = nr; st->inflated_bytes = is.L.utotal; st->compressed_bytes = is.L.comp_bytes;
        st->raw = rs; st->h2d_ms = is.h2d_ms; st->inflate_ms = inflate_ms; st->index_ms = index_ms; st->filter_ms = filter_ms;
        st->prefetch_ms = is.prefetched ? c->pf_ms : 0.f; st->prefetch_wait_ms = is.prefetched ? is.pf_wait_ms : 0.f;
    }
    return VTX_OK;
}

static int ingest_run(vtx_ctx* c, const vtx_bam_ingest* g, const vtx_bam_segments* sg, vtx_ingest_stats* st) {
    IngestState is;
    is.g = g; is.sg = sg; is.st = st;
    if (int rc = ingest_check_layout(c, is)) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    ingest_settle_prefetch(c, is);
    if (int rc = ingest_reserve(c, is)) return rc;
    if (int rc = ingest_upload(c, is)) return rc;
    if (int rc = ingest_inflate_crc(c, is)) return rc;
    if (int rc = ingest_chains(c, is)) return rc;
    if (int rc = ingest_filter(c, is)) return rc;
    return ingest_publish(c, is);
}

int vtx_submit_bam(vtx_ctx* c, const vtx_bam_ingest* g, vtx_ingest_stats* st) {
    if (!c) return VTX_E_INVAL;
    if (!g) return fail(c, VTX_E_INVAL, "vtx_submit_bam: null argument");
    return ingest_run(c, g, nullptr, st);
}

// ---- vtx_submit_bam_segments: the same ingest for a plan of several stretches of the file (sparse loci) ----
int vtx_submit_bam_segments(vtx_ctx* c, const vtx_bam_segments* sg, vtx_ingest_stats* st) {
    if (!c) return VTX_E_INVAL;
    if (!sg) return fail(c, VTX_E_INVAL, "vtx_submit_bam_segments: null argument");
    return ingest_run(c, &sg->base, sg, st);
}

// Test hook: bgzf_inflate_kernel on arbitrary raw-DEFLATE payloads — block i is file[blocks[i].coff .. + clen) and must inflate to
// exactly blocks[i].isize bytes; status[i] = 0 when the device's decoder accepted it (its bytes at out + the sum of the isizes before
// it), else a vtxi::Status.  Blocks need not be ordered or disjoint (the tests feed truncated copies of one stream).
int vtx_debug_inflate(vtx_ctx* c, const uint8_t* file, uint64_t file_bytes, const vtx_bgzf_block* blk, uint32_t n, uint8_t* out, uint64_t out_cap, uint32_t* status) {
    if (!c || (n && (!blk || !status)) || (file_bytes && !file)) return VTX_E_INVAL;
    std::vector<vtxg_block> blocks(n);
    uint64_t utotal = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (blk[i].coff > file_bytes || blk[i].clen > file_bytes - blk[i].coff || blk[i].isize > 65536u) return fail(c, VTX_E_INVAL, "vtx_debug_inflate: block %u outside the input or above 64 KiB", i);
        blocks[i] = vtxg_block{blk[i].coff, utotal, blk[i].clen, blk[i].isize};
        utotal += blk[i].isize;
    }
    if (utotal > out_cap) return fail(c, VTX_E_INVAL, "vtx_debug_inflate: output buffer too small");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    prefetch_settle(c, Prefetch::Drop);
    HIP_TRY(c, c->d_bam_comp.reserve((size_t)file_bytes + kBamPad));
    HIP_TRY(c, c->d_bam_data.reserve((size_t)utotal + kBamPad));
    HIP_TRY(c, c->d_bam_blocks.reserve((size_t)n * sizeof(vtxg_block) + 16));
    BamCounters cnt;
    if (int rc = reserve_bam_counters(c, &cnt)) return rc;
    HIP_TRY(c, c->d_bam_seed_cnt.reserve((size_t)n * sizeof(uint32_t) + 16));
    uint32_t* d_err = cnt.err;
    HIP_TRY(c, hipMemsetAsync(d_err, 0, 4 * sizeof(uint32_t), s));
    HIP_TRY(c, hipMemsetAsync(c->d_bam_data.p, 0xEE, (size_t)utotal + kBamPad, s));
    if (file_bytes) HIP_TRY(c, hipMemcpyAsync(c->d_bam_comp.p, file, (size_t)file_bytes, hipMemcpyHostToDevice, s));
    if (n) HIP_TRY(c, hipMemcpyAsync(c->d_bam_blocks.p, blocks.data(), (size_t)n * sizeof(vtxg_block), hipMemcpyHostToDevice, s));
    HIP_TRY(c, vtxg_inflate(c->d_bam_comp.as<uint8_t>(), c->d_bam_blocks.as<vtxg_block>(), n, c->d_bam_data.as<uint8_t>(), d_err, c->d_bam_seed_cnt.as<uint32_t>(), 0, s));
    if (n) HIP_TRY(c, hipMemcpyAsync(status, c->d_bam_seed_cnt.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (utotal && out) HIP_TRY(c, hipMemcpyAsync(out, c->d_bam_data.p, (size_t)utotal, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return VTX_OK;
}

// Test hook: bgzf_crc32_kernel on arbitrary byte ranges — range i is data[offsets[i] .. offsets[i + 1]), at most 64 KiB each; crc_out[i]
// = its CRC-32 as the device computes it (no trailer to compare with).  vtx_last_crc_ms then gives the kernel's time.
int vtx_debug_crc32(vtx_ctx* c, const uint8_t* data, uint64_t n_bytes, const uint64_t* offsets, uint32_t n, uint32_t* crc_out) {
    if (!c || !offsets || (n && !crc_out) || (n_bytes && !data)) return VTX_E_INVAL;
    std::vector<vtxg_block> blocks(n);
    if (offsets[n] > n_bytes) return fail(c, VTX_E_INVAL, "vtx_debug_crc32: the last offset lies outside the data");
    for (uint32_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 65536u) return fail(c, VTX_E_INVAL, "vtx_debug_crc32: range %u: not ascending or above 64 KiB", i);
        blocks[i] = vtxg_block{0, offsets[i], 0, (uint32_t)(offsets[i + 1] - offsets[i])};
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    prefetch_settle(c, Prefetch::Keep);                   // (upload() below; d_bam_comp is not touched)
    HIP_TRY(c, c->d_bam_data.reserve((size_t)n_bytes + 64));
    HIP_TRY(c, c->d_bam_blocks.reserve((size_t)n * sizeof(vtxg_block) + 16));
    BamCounters cnt;
    if (int rc = reserve_bam_counters(c, &cnt)) return rc;
    HIP_TRY(c, c->d_bam_seed_cnt.reserve((size_t)n * sizeof(uint32_t) + 16));
    uint32_t* d_err = cnt.err;
    HIP_TRY(c, hipMemsetAsync(d_err, 0, 4 * sizeof(uint32_t), s));
    if (int rc = upload(c, {{c->d_bam_data.p, data, (size_t)n_bytes}, {c->d_bam_blocks.p, blocks.data(), (size_t)n * sizeof(vtxg_block)}})) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipEventRecord(c->ev_crc[0], s));
    HIP_TRY(c, vtxg_crc32(nullptr, c->d_bam_blocks.as<vtxg_block>(), n, c->d_bam_data.as<uint8_t>(), d_err, c->d_bam_seed_cnt.as<uint32_t>(), 0, crc_width(), s));
    HIP_TRY(c, hipEventRecord(c->ev_crc[1], s));
    if (n) HIP_TRY(c, hipMemcpyAsync(crc_out, c->d_bam_seed_cnt.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipEventElapsedTime(&c->crc_ms, c->ev_crc[0], c->ev_crc[1]));
    return VTX_OK;
}

// Device time of the last bgzf_crc32_kernel launch of this context (vtx_submit_bam / vtx_submit_bam_segments that got as far as the
// raw records, or vtx_debug_crc32), in milliseconds; 0 before any.
int vtx_last_crc_ms(vtx_ctx* c, float* ms) {
    if (!c || !ms) return VTX_E_INVAL;
    *ms = c->crc_ms;
    return VTX_OK;
}

// Test / audit hook: the ingest's intermediate arrays of the last vtx_submit_bam (what: VTX_INGEST_*).  *bytes = the array's size;
// min(cap, *bytes) bytes are copied to dst.
int vtx_debug_ingest(vtx_ctx* c, int what, void* dst, uint64_t cap, uint64_t* bytes) {
    if (!c || !bytes) return VTX_E_INVAL;
    const void* src = nullptr;
    uint64_t n = 0;
    switch (what) {
    case VTX_INGEST_INFLATED: src = c->d_bam_data.p; n = c->bam_utotal; break;
    case VTX_INGEST_RECORD_OFFSETS: src = c->d_bam_rec.p; n = (uint64_t)c->bam_n_rec * 8; break;
    case VTX_INGEST_RAW_RECORDS: src = c->d_raw.p; n = (uint64_t)c->bam_n_raw * sizeof(vtx_raw_record); break;
    case VTX_INGEST_RAW_LOCUS: src = c->d_raw_locus.p; n = (uint64_t)c->bam_n_raw * 4; break;
    case VTX_INGEST_TAGS: src = c->d_tags.p; n = c->bam_tag_bytes; break;
    case VTX_INGEST_READS_PACKED: src = c->d_read_packed.p; n = c->bam_read_bases / 2; break;
    default: return fail(c, VTX_E_INVAL, "vtx_debug_ingest: unknown array %d", what);
    }
    *bytes = n;
    const uint64_t k = std::min(cap, n);
    if (k && dst) {
        HIP_TRY(c, hipSetDevice(c->cfg.device));
        HIP_TRY(c, hipMemcpy(dst, src, (size_t)k, hipMemcpyDeviceToHost));
    }
    return VTX_OK;
}

int vtx_fetch_records(vtx_ctx* c, vtx_record* records, uint32_t* rec_begin, uint32_t* rec_count) {
    if (!c) return VTX_E_INVAL;
    if (!c->submitted) return fail(c, VTX_E_STATE, "vtx_fetch_records: no batch submitted");
    if ((c->n_records && !records) || (c->n_loci && (!rec_begin || !rec_count))) return fail(c, VTX_E_INVAL, "vtx_fetch_records: null output");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (c->n_records) HIP_TRY(c, hipMemcpy(records, c->d_records.p, (size_t)c->n_records * sizeof(vtx_record), hipMemcpyDeviceToHost));
    if (c->n_loci) {
        std::vector<vtx_locus> loci(c->n_loci);
        HIP_TRY(c, hipMemcpy(loci.data(), c->d_loci.p, (size_t)c->n_loci * sizeof(vtx_locus), hipMemcpyDeviceToHost));
        for (uint32_t l = 0; l < c->n_loci; ++l) { rec_begin[l] = loci[l].rec_begin; rec_count[l] = loci[l].rec_count; }
    }
    return VTX_OK;
}

}  // extern "C": the run path's helpers are C++

namespace {

// ---- vtx_run: the hooks, the state its stages share -------------------------------------------------------------------------
// The developer hooks of vtx_run that hold for the life of the process (libvtx_dev.so; in libvtx.so every VTX_DEV_ENV is the constant
// nullptr and the members are their defaults), and whether VTX_DEBUG asked for the kernels' statistics.  Read once, by band_knobs().
inline bool env_is(const char* v, const char* what) { return v && !strcmp(v, what); }
inline uint32_t env_u32(const char* v, int base, uint32_t dflt) { return v ? (uint32_t)strtoul(v, nullptr, base) : dflt; }
struct BandKnobs {
    bool no_duo = env_is(VTX_DEV_ENV("VTX_DP_KERNEL"), "lut"), no_pair = env_is(VTX_DEV_ENV("VTX_DP_KERNEL"), "duo2");   // (duo2: two-lookup prefix phase)
    bool no_coop = VTX_DEV_ENV("VTX_BAND_NO_COOP") != nullptr;                  // experiment / test hook
    uint32_t diag2_min = env_u32(VTX_DEV_ENV("VTX_BAND_DIAG2_MIN"), 10, 700000u);   // the shortest list the second stage takes (see second_stage_on)
    bool no_stream = VTX_DEV_ENV("VTX_BAND_NO_STREAM") != nullptr;              // what exceeds the second stage's list goes to the sweep
    bool no_diag = VTX_DEV_ENV("VTX_BAND_NO_DIAG") != nullptr;                  // experiment / test hook: stage 1 off
    bool legacy = VTX_DEV_ENV("VTX_BAND_LEGACY") != nullptr;                    // round 3's band_run_kernel / pending / general path (kept for A/B tests)
    bool no_tight = VTX_DEV_ENV("VTX_BAND_NO_TIGHT") != nullptr;                // test hook: tasks with a certificate go to the sweep like the others
    bool use_check = VTX_DEV_ENV("VTX_BAND_CHECK") != nullptr;                  // experiment hook: full-matrix check in front of their DP
    uint32_t dense_mask = env_u32(VTX_DEV_ENV("VTX_BAND_DENSE_MASK"), 0, 1u << 4);   // experiment knob (0x3be: everything but shape; 0: nothing — band_run_kernel sees every task first)
    bool no_refine = VTX_DEV_ENV("VTX_BAND_NO_REFINE") != nullptr;              // experiment / test hook
    bool no_fork = VTX_DEV_ENV("VTX_BAND_NO_FORK") != nullptr;                  // experiment / test hook
    bool tail_inline = VTX_DEV_ENV("VTX_BAND_TAIL_INLINE") != nullptr;          // A/B hook: band_tail_kernel behind band_diag_kernel on the main stream in fork mode too
    bool no_corridor = VTX_DEV_ENV("VTX_BAND_NO_CORRIDOR") != nullptr;          // round 3's band_refine_kernel instead of band_corridor_kernel
    uint32_t run_min = env_u32(VTX_DEV_ENV("VTX_BAND_RUN_MIN"), 10, 65536u);    // the shortest list worth band_run_kernel's launch (see repeats)
    bool no_split = VTX_DEV_ENV("VTX_BAND_NO_SPLIT") != nullptr;                // test hook: the single pass of rounds 3 - 5
    bool debug = getenv("VTX_DEBUG") != nullptr;                                // the [vtx] lines on stderr
    bool sweep_stats = debug;                                                   // band_sweep_kernel counts its reasons
    int diag_stats = debug ? 1 : 0;                                             // band_diag_kernel and its followers count theirs
};
const BandKnobs& band_knobs() { static const BandKnobs k; return k; }
// What the stages of one vtx_run share.  a: the batch's arrays, filled once per run from the context; stage: one byte per task saying which stage decided it (vtx_fetch_stage), or nullptr
struct RunState { vtx_task_arrays a{}; uint8_t* stage = nullptr; uint32_t launches = 0, hard_total = 0; float band_run_ms = 0; };

// A member of the banded stage's counter block (vtx_band_counters, device memory) zeroed, and copied to the host: to the member of the same type in PinnedCounters (does not
// block), or to pageable memory (blocks until the stream reaches the copy).  The size is the member's.
template <class T> hipError_t zero(T& member, hipStream_t st) { return hipMemsetAsync(&member, 0, sizeof(T), st); }
template <class T> hipError_t read_back(T& host, const T& member, hipStream_t st) { return hipMemcpyAsync(&host, &member, sizeof(T), hipMemcpyDeviceToHost, st); }

// ---- vtx_run: one pass of the banded stages ---------------------------------------------------------------------------------------
// Tasks [t_begin, t_end) whose locus has its longer haplotype in (mh_min, mh] (the others are left alone); chunk_tables: the tables are built per chunk for the loci the chunk spans, whatever the
// buffer would hold. Per chunk of tasks (task = 2*record + hap), round 4 (the stages are described in vtx_band.hip's header): tables -> band_diag_kernel (+ band_refine_kernel): scores of the
// certified tasks, and three lists — tasks whose band is one diagonal stretch (masked DP straight from one word), repeats (band_sweep_kernel + masked DP), the others (band_run_kernel: seeds,
// chain, general certificate; its hard list -> expand -> masked DP).  What overflows band_run_kernel's lists joins the repeats after the last chunk; what band_sweep_kernel declines takes
// the general band kernel (side stream). The counters are vtx_band_counters (vtx_device.h), what is read back through pinned memory PinnedCounters, the events EvSlot.
struct BandPass {
    vtx_ctx* const c;
    RunState& rs;
    const uint32_t mh, mh_min;
    const uint64_t t_begin, t_end;
    const bool chunk_tables;
    const BandKnobs& kn = band_knobs();
    const vtx_task_arrays& a = rs.a;
    hipStream_t s = c->stream, s2 = nullptr;
    BandPlan bp;
    bool gt_chunked = false, sweep_path = false;
    vtx_band_counters* d_cnt = nullptr;
    const int* shape = kShapes[0];              // the masked DP's (rows per lane, lanes per record) for the batch's longest read
    uint32_t *tight_list = nullptr, *tight_pack = nullptr, *dense_list = nullptr, *refine_list = nullptr, refine_cap = 0;   // band_diag_kernel's other outputs
    // The launchers' bundles that hold for the whole pass, built once in run(): the pass's shape; the lists of band_diag_kernel and the kernels over its records; band_run_kernel's outputs
    vtx_band_shape sh{};
    vtx_diag_routes routes{};
    vtx_band_out run_out{};
    vtx_band_counters::run_t cnt{};             // host copy of band_run_kernel's counters
    uint32_t pending_total = 0, over_before = 0;
    uint64_t diag_total = 0, diag_left = 0, refined_total = 0, checked_total = 0, swept_total = 0, diag2_total = 0, diag2_scored = 0, tight2_total = 0, stream_total = 0;
    float diag_ms = 0, check_ms = 0, sweep_ms = 0;
    bool sweep_used = false;                    // some chunk took the round-4 path
    // a swept chunk whose events (and, forked, final counts) collect_sweep_times has not read yet: whether it ran its two branches side by side, with band_tail_kernel on the side one; its tasks
    struct OpenSweep { bool open = false, forked = false, tail_side = false; uint32_t nt = 0; } open_sweep;
    // one chunk of tasks [base, base + nt): the loci whose tables are resident, and what band_diag_kernel left for band_run_kernel
    struct Chunk { uint64_t base; uint32_t nt; bool last; vtx_band_tables tb{}; bool diag = false, swept = false; uint32_t n_fail = 0; const uint32_t* fail_list = nullptr;
                   vtx_rec_buf tail{}; bool tail_side = false;          // band_tail_kernel's record buffer; whether diag_sweep_path launches that kernel on the side stream
                   vtx_rec_buf recheck{}; };                            // the recheck's record buffer (cap 0: no recheck for this chunk)
    BandPass(vtx_ctx* c_, RunState& rs_, uint32_t mh_, uint32_t mh_min_, uint64_t t_begin_, uint64_t t_end_, bool chunk_tables_) : c(c_), rs(rs_), mh(mh_), mh_min(mh_min_), t_begin(t_begin_), t_end(t_end_),
             chunk_tables(chunk_tables_) {}
    int run() {
        bp = band_plan(c->n_records, c->n_loci, mh);
        if (int rc = band_reserve(c, bp, false)) return rc;
        gt_chunked = bp.gt_bytes && (bp.gt_loci < c->n_loci || chunk_tables);
        d_cnt = c->d_cnt.as<vtx_band_counters>();
        int k = 0;
        while ((uint32_t)(kShapes[k][0] * kShapes[k][1]) < c->max_read_len) ++k;
        shape = kShapes[k];
        if (!c->stream2) {
            HIP_TRY(c, hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
            HIP_TRY(c, hipEventCreateWithFlags(&c->ev2, hipEventDisableTiming));
            HIP_TRY(c, hipHostMalloc((void**)&c->h_pin, sizeof(PinnedCounters), hipHostMallocDefault));
        }
        s2 = c->stream2;
        // Round 4's path (sweep + masked DP for what the certificate stages leave), or round 3's (VTX_BAND_LEGACY=1; a haplotype above 255 bases)
        sweep_path = !kn.legacy && mh <= vtxk_band_sweep_max_len() && mh > 0;
        tight_list = (sweep_path && !kn.no_tight) ? c->d_tight.as<uint32_t>() : nullptr;
        tight_pack = tight_list ? c->d_tight_pack.as<uint32_t>() : nullptr;
        // dense list: the tasks whose vtxf::Why is in kn.dense_mask (default W_MATCHES: repeats) skip band_run_kernel and take band_sweep_kernel at once
        dense_list = sweep_path ? c->d_dense.as<uint32_t>() : nullptr;
        refine_cap = std::min(band_refine_cap(bp.chunk), env_u32(VTX_DEV_ENV("VTX_DIAG_REFINE_CAP"), 10, 0xffffffffu));   // (test hook: a small record buffer, read per run)
        refine_list = kn.no_refine ? nullptr : c->d_refine.as<uint32_t>();
        sh = vtx_band_shape{mh, mh_min, c->max_read_len, bp.tasks_per_locus};
        routes = vtx_diag_routes{c->d_fail.as<uint32_t>(), refine_list, refine_cap, d_cnt, kn.diag_stats, tight_list, tight_pack, rs.stage, dense_list, kn.dense_mask};
        run_out = vtx_band_out{c->d_poly.as<uint16_t>(), bp.poly_stride / 2, c->d_hard.as<uint32_t>(), c->d_over.as<uint32_t>(), nullptr, d_cnt};
        HIP_TRY(c, zero(*d_cnt, s));
        for (uint64_t base = t_begin; base < t_end; base += bp.chunk) {
            Chunk ch{base, (uint32_t)std::min<uint64_t>(bp.chunk, t_end - base), base + bp.chunk >= t_end};
            ch.fail_list = c->d_fail.as<uint32_t>();
            if (int rc = resident_tables(ch)) return rc;
            if (ch.tb.n_loci && !kn.no_diag) { if (int rc = diag_stage(ch)) return rc; }
            if (int rc = run_stage(ch)) return rc;
            if (sweep_used && ch.last) { if (int rc = last_chunk()) return rc; }
        }
        return publish();
    }
    // src == nullptr: the band slots already hold arrays (or the full-matrix marker), one slot per task
    int masked_dp(uint32_t n_hard, uint32_t* hard, const uint16_t* src, uint16_t* band, uint32_t n_slots, hipStream_t st, uint8_t code) {
        if (rs.stage) HIP_TRY(c, vtxk_mark_stage(hard, n_hard, nullptr, code, rs.stage, st));
        for (uint32_t off = 0; off < n_hard; off += n_slots) {
            const uint32_t cnt_s = std::min(n_slots, n_hard - off);
            HIP_TRY(c, vtxk_launch_band_expand(a, hard + off, cnt_s, src ? src + (size_t)off * bp.poly_stride : band, src ? bp.poly_stride : 2 * bp.band_stride, band, bp.band_stride, st));
            HIP_TRY(c, vtxk_launch_sw_banded(a, shape[0], shape[1], cnt_s, hard + off, band, bp.band_stride, mh, st));
            rs.launches += 2;
        }
        return VTX_OK;
    }
    // The general band kernel (tasks band_run_kernel could not hold) is a handful of serial lanes: ~4.5 ms of latency for 0.1 % of config 3.  It runs on a side
    // stream, with its own hard list; started once the overflow list is complete, finished (slabs grow until every task fits) after the main path's launches are queued.
    struct GeneralFallback {
        BandPass& pass;                         // (its masked DP and its counter block)
        vtx_ctx* const c = pass.c; const BandKnobs& kn = pass.kn; const vtx_task_arrays& a = pass.a; const vtx_band_shape& sh = pass.sh; const BandPlan& bp = pass.bp; RunState& rs = pass.rs;
        const hipStream_t& s2 = pass.s2;        // (the side stream: set in BandPass::run)
        uint32_t n_over = 0, cap2 = 0, todo = 0, off = 0, total = 0; const uint32_t* tasks = nullptr; bool active = false; uint32_t n_hard = 0, n_again = 0;
        explicit GeneralFallback(BandPass& p) : pass(p) {}
        // the half of d_over2 the general kernel's current list is not in: where it writes the tasks that need a larger slab
        uint32_t* other() const { return c->d_over2.as<uint32_t>() + ((tasks == c->d_over2.as<uint32_t>()) ? n_over : 0); }
        int launch() {
            // A few overflow tasks (shallow data: some hundreds per run) first try the in-LDS variant of the general kernel
            // with a slab for kLdsMatches k-mer matches: their ~2 ms of serial HBM latency were a third of a shallow step.
            const uint32_t kLdsMatches = 512, kLdsTasks = 4096, mh = sh.max_hap;       // (kLdsTasks: the longest list the in-LDS variant takes)
            const uint64_t worst = (uint64_t)c->max_read_len * mh;
            if (cap2 >= worst && cap2 >= 512) return fail(c, VTX_E_STATE, "vtx_run: band kernel overflow with a worst-case slab");
            // first three rounds: the cooperative kernel, everything in LDS (band_coop_kernel: a wavefront per task, up to 512 matches,
            // then 1024, then 4096; reads up to 256 bases); what that cannot hold takes the serial kernel below
            const int tier = cap2 < 512 ? 0 : (cap2 == 512 ? 1 : (cap2 == 1024 ? 2 : -1));
            const uint32_t tier_cap = tier == 0 ? 512u : (tier == 1 ? 1024u : 4096u);
            // (haplotypes up to 1000 bases: the kernel walks its Fenwick tree in ten unrolled steps, tn = n + 8 < 1024)
            const bool coop = tier >= 0 && !kn.no_coop && c->max_read_len <= 256 && mh <= 1000 && vtxk_band_coop_lds(mh, tier_cap) <= 64u * 1024;
            // (its own band slots and hard list; the tasks that need a larger slab go to the other half of d_over2)
            vtx_cnt_pair& cnt = pass.d_cnt->general;
            const vtx_band_out out{c->d_band2.as<uint16_t>(), bp.band_stride, c->d_hard2.as<uint32_t>(), other(), &cnt};
            if (coop) {
                cap2 = tier_cap;
                HIP_TRY(c, zero(cnt.overflow, s2));
                HIP_TRY(c, vtxk_launch_band_coop(a, tier, tasks, todo, sh, out, s2));
            } else {
                const bool in_lds = cap2 < 512 && todo <= kLdsTasks && vtxk_band_lds_stride(kLdsMatches, mh, c->max_read_len) <= 160 * 1024 - 512;
                cap2 = in_lds ? kLdsMatches : (uint32_t)std::max<uint64_t>(std::min<uint64_t>((uint64_t)cap2 * 16, worst), 512);
                const size_t stride2 = vtxk_band_ws_stride(cap2, mh);
                if (!in_lds) {                                                  // whole wavefronts: the 64 slabs are interleaved, vtxk_band_lanes() of them in use
                    const size_t lanes = vtxk_band_lanes(todo);
                    HIP_TRY(c, c->d_band_ws2.reserve(lanes < 64 ? (size_t)todo * stride2 : ((size_t)todo + 63) / 64 * 64 * stride2));   // (sparse lanes: a contiguous slab per task)
                }
                HIP_TRY(c, zero(cnt.overflow, s2));
                HIP_TRY(c, vtxk_launch_band(a, tasks, todo, 0, c->d_band_ws2.as<uint8_t>(), stride2, cap2, sh, out, in_lds ? 1 : 0, s2));
            }
            HIP_TRY(c, read_back(c->h_pin->general, cnt, s2));   // pinned: does not block
            ++rs.launches;
            return VTX_OK;
        }
        int start(uint32_t off_, uint32_t total_) {   // the overflow list d_over[0, total) is complete and visible
            n_over = std::min(std::max(bp.slots, 1024u), total_ - off_);   // slices (bounds d_band2)
            off = off_; total = total_; todo = n_over; cap2 = 512 / 16; tasks = c->d_over.as<uint32_t>() + off; active = true;
            HIP_TRY(c, c->d_over2.reserve(2 * (size_t)n_over * sizeof(uint32_t)));
            HIP_TRY(c, c->d_hard2.reserve((size_t)n_over * sizeof(uint32_t)));
            HIP_TRY(c, c->d_band2.reserve((size_t)n_over * 2 * bp.band_stride * sizeof(uint16_t)));
            HIP_TRY(c, zero(pass.d_cnt->general, s2));
            return launch();
        }
        int finish() {
            if (!active) return VTX_OK;
            for (;;) {
                for (;;) {
                    HIP_TRY(c, hipStreamSynchronize(s2));
                    n_hard = c->h_pin->general.hard; n_again = c->h_pin->general.overflow;
                    // tasks that still do not fit were written to the other half of d_over2: rerun them with a larger slab
                    tasks = other();
                    todo = n_again;
                    if (!todo) break;
                    if (int rc = launch()) return rc;
                }
                if (int rc = pass.masked_dp(n_hard, c->d_hard2.as<uint32_t>(), nullptr, c->d_band2.as<uint16_t>(), std::max(n_hard, 1u), s2, VTX_STAGE_GENERAL_DP)) return rc;
                rs.hard_total += n_hard;
                if (off + n_over >= total) break;
                if (int rc = start(off + n_over, total)) return rc;      // next slice (same stream: in order)
            }
            HIP_TRY(c, hipEventRecord(c->ev2, s2));
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev2, 0));         // the reduction kernels read every score
            return VTX_OK;
        }
    } fb{*this};
    // the band of every listed task (band_sweep_kernel), one slice of band slots at a time, then the masked DP over the slice (its length — the tasks the sweep did not decline — is read on the
    // device: counters[0]; declined: counters[1])
    int sweep_slices(const uint32_t* list, uint32_t n, uint32_t* over_out, vtx_cnt_pair* counters) {
        uint32_t* why = kn.sweep_stats ? d_cnt->sweep_why : nullptr;
        HIP_TRY(c, c->d_sweep_log.reserve(vtxk_band_sweep_log_bytes()));
        const vtx_band_out out{c->d_band.as<uint16_t>(), bp.band_stride, c->d_hard.as<uint32_t>(), over_out, counters};
        for (uint32_t off = 0; off < n; off += bp.slots) {
            const uint32_t cnt_s = std::min(bp.slots, n - off);
            HIP_TRY(c, zero(counters->hard, s));
            HIP_TRY(c, vtxk_launch_band_sweep(a, list + off, cnt_s, nullptr, out, why, rs.stage, nullptr, c->d_sweep_log.as<uint32_t>(), s));
            HIP_TRY(c, vtxk_launch_sw_banded_dev(a, shape[0], shape[1], cnt_s, out.hard_list, &counters->hard, out.band, out.band_stride, mh, s));
            rs.launches += 2;
        }
        return VTX_OK;
    }
    // Second stage (round 5; DESIGN.md 4.3.3b, where its threshold of 700 k tasks is measured): band_diag2_kernel, band_stream_kernel for what exceeds its list, the full-matrix check + masked DP
    // over the one-diagonal bands they prove; what they leave — out[0, *n_out) — takes the sweep.  One host round trip for the counts. The tables of the tasks' loci have to be resident (tb:
    // the table buffer as the stage that built them was handed it).
    bool second_stage_on(uint32_t n) const { return n >= kn.diag2_min && mh <= 255; }
    int second_stage(const uint32_t* list, uint32_t n, const vtx_band_tables& tb, uint32_t* out, uint32_t* n_out) {
        HIP_TRY(c, zero(d_cnt->diag2, s));
        HIP_TRY(c, zero(d_cnt->streamed, s));
        HIP_TRY(c, vtxk_launch_band_diag2(a, list, n, sh, tb, out, c->d_tight2.as<uint32_t>(), c->d_tight2_pack.as<uint32_t>(), &d_cnt->diag2.left,
                kn.no_stream ? nullptr : c->d_recheck2.as<uint32_t>(), c->d_recheck2_pack.as<uint32_t>(), &d_cnt->streamed, rs.stage, s));
        HIP_TRY(c, read_back(c->h_pin->diag2, d_cnt->diag2, s));
        HIP_TRY(c, read_back(c->h_pin->streamed, d_cnt->streamed, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        stream_total += std::min(c->h_pin->streamed, n);
        const uint32_t n_sweep = std::min(c->h_pin->diag2.left, n);
        const uint32_t n_tight2 = std::min(c->h_pin->diag2.tight, n - n_sweep);
        ++rs.launches;
        diag2_total += n; diag2_scored += n - n_sweep - n_tight2;
        if (n_tight2) {
            // certificate == full-matrix score decides practically all of them (cert <= banded <= full); the masked DP for the rest (count on the device)
            HIP_TRY(c, zero(d_cnt->check2, s));
            HIP_TRY(c, vtxk_launch_sw_check(a, shape[0], shape[1], n_tight2, c->d_tight2.as<uint32_t>(), c->d_tight2_pack.as<uint32_t>(), nullptr, mh, c->d_recheck2.as<uint32_t>(), c->d_recheck2_pack.as<uint32_t>(),
                                            &d_cnt->check2, rs.stage, s));
            HIP_TRY(c, vtxk_launch_sw_diag_band(a, shape[0], shape[1], n_tight2, c->d_recheck2.as<uint32_t>(), c->d_recheck2_pack.as<uint32_t>(), &d_cnt->check2, mh, rs.stage, s));
            // (its grid is sized for n_tight2 although a few hundred tasks remain: the workgroups past the device count leave at once)
            rs.launches += 2;
            tight2_total += n_tight2;
        }
        *n_out = n_sweep; return 0;
    }
    int collect_sweep_times() {
        const OpenSweep sw = open_sweep;
        open_sweep = OpenSweep{};
        if (!sw.open) return VTX_OK;
        HIP_TRY(c, hipEventSynchronize(c->ev[EV_SWEEP_END]));
        float ms = 0;
        // BRANCH_START .. BRANCH_END: band_tail_kernel (when it runs on the side stream) + band_refine_kernel (forked only) + the one-diagonal bands' masked DP; then band_sweep_kernel + its
        // masked DP (the chunk's repeats) — forked: FORK_START .. SWEEP_END on the main stream, BESIDE the first interval, not after it
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[EV_BRANCH_START], c->ev[EV_BRANCH_END])); check_ms += ms;
        HIP_TRY(c, hipEventElapsedTime(&ms, sw.forked ? c->ev[EV_FORK_START] : c->ev[EV_BRANCH_END], c->ev[EV_SWEEP_END])); sweep_ms += ms;
        if (sw.forked) checked_total += std::min(c->h_pin->fork_tight, sw.nt);                // (copied before BRANCH_END, which SWEEP_END waited for)
        if (sw.tail_side) refined_total += std::min(c->h_pin->fork_refine, refine_cap);       // (likewise; band_tail_kernel's records included)
        return VTX_OK;
    }
    // Sorts list[0, n) by task into `sorted` when it has more than 64 entries and the temporary buffer can be had; *at = where the list then is.  (Lists come out in the order the wavefronts
    // finished: eight XCD ranges interleaved.  Sorted, neighbours share their loci's tables, haplotypes and reads again — 12.7 -> GB of L2 misses for 2 % of the tasks otherwise — and the hard
    // list comes out in a fixed order.)
    int sort_by_task(uint32_t* list, uint32_t* sorted, uint32_t n, const uint32_t** at) {
        *at = list;
        if (n <= 64) return VTX_OK;
        const size_t tb = vtxk_sort_keys_u32_temp_bytes(n);
        if (c->d_fail_tmp.reserve(tb) != hipSuccess) { (void)hipGetLastError(); return VTX_OK; }
        HIP_TRY(c, vtxk_sort_keys_u32(list, sorted, n, c->d_fail_tmp.p, tb, s));
        *at = sorted;
        return VTX_OK;
    }
    // the chunk's counters, and the loci of this range of tasks (tables in global memory are built per range)
    int resident_tables(Chunk& ch) {
        if (int rc = collect_sweep_times()) return rc;                              // (a chunk re-records the events)
        HIP_TRY(c, zero(d_cnt->run.hard, s));
        HIP_TRY(c, zero(d_cnt->run.pending, s));
        uint32_t gt_l0 = 0, gt_n = bp.gt_bytes ? c->n_loci : 0;
        if (gt_chunked) {
            uint32_t ends[2];
            HIP_TRY(c, hipMemcpyAsync(&ends[0], a.rec_locus + ch.base / 2, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipMemcpyAsync(&ends[1], a.rec_locus + (ch.base + ch.nt - 1) / 2, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            gt_l0 = ends[0]; gt_n = ends[1] - ends[0] + 1;
            if (gt_n > bp.gt_loci) gt_n = 0;                    // does not fit after all: tables in LDS for this chunk
        }
        ch.tb = vtx_band_tables{gt_n ? c->d_gtables.as<uint8_t>() : nullptr, bp.gt_bytes, gt_l0, gt_n};      // (no table buffer for band_run_kernel: it builds them in LDS)
        c->gt_used = (gt_n && bp.gt_loci) ? (uint64_t)gt_n * (bp.gt_bytes / bp.gt_loci) : 0;     // (gt_bytes = gt_loci x bytes per locus)
        HIP_TRY(c, hipEventRecord(c->ev[EV_CHUNK_START], s));
        return VTX_OK;
    }
    // Stage 1 (tables in global memory): band_diag_kernel decides the tasks whose alignment lives on one diagonal
    // (vtx_fast_core.h) and lists the others; band_run_kernel then takes that LIST instead of the whole range.
    int diag_stage(Chunk& ch) {
        HIP_TRY(c, zero(d_cnt->lists, s));
        const uint32_t tail_cap = (uint32_t)std::min<size_t>(band_tail_cap(bp.chunk), c->d_tail.cap / (vtxk_band_tail_words() * sizeof(uint32_t)));
        const uint32_t tail_cap_hook = VTX_DEV_ENV("VTX_DIAG_TAIL_CAP") ? (uint32_t)atoi(VTX_DEV_ENV("VTX_DIAG_TAIL_CAP")) : 0xffffffffu;   // test hook: a small buffer (read per run)
        ch.tail = vtx_rec_buf{c->d_tail.as<uint32_t>(), std::min(tail_cap, tail_cap_hook)};
        // The sweep path with its two branches: band_tail_kernel goes to the side one (diag_sweep_path).  Every other path keeps it behind band_diag_kernel on this stream.
        ch.tail_side = sweep_path && fork_on() && !kn.tail_inline && vtxk_band_tail_on(ch.tail);
        // The recheck of the tasks that fail band_diag_kernel's harmless test (diag_sweep_path launches it): on the path with the two branches only, where a task it clears has a tight
        // list to go to and band_corridor_kernel behind it.  Every other path (no fork, no tight list, round 3's, four-byte entries: vtxk_band_recheck_on) hands the kernel no buffer.
        const uint32_t recheck_cap = (uint32_t)std::min<size_t>(band_recheck_cap(bp.chunk), c->d_recheck.cap / (vtxk_band_tail_words() * sizeof(uint32_t)));
        const uint32_t recheck_cap_hook = VTX_DEV_ENV("VTX_DIAG_RECHECK_CAP") ? (uint32_t)atoi(VTX_DEV_ENV("VTX_DIAG_RECHECK_CAP")) : 0xffffffffu;   // test hook: a small buffer (read per run)
        ch.recheck = vtx_rec_buf{c->d_recheck.as<uint32_t>(), std::min(recheck_cap, recheck_cap_hook)};
        if (!(sweep_path && fork_on() && refine_list && !kn.no_corridor && vtxk_band_recheck_on(ch.recheck, mh))) ch.recheck = vtx_rec_buf{nullptr, 0};
        const hipError_t e = vtxk_launch_band_diag(a, ch.nt, (uint32_t)ch.base, sh, ch.tb, routes, ch.tail, !ch.tail_side, ch.recheck, s);
        if (e != hipSuccess) {
            // (the tables do not fit the buffer for this chunk: band_run_kernel alone, tables in LDS)
            if (kn.debug) fprintf(stderr, "[vtx] band_diag_kernel not launched for tasks [%llu, +%u): %s\n", (unsigned long long)ch.base, ch.nt, hipGetErrorString(e));
            (void)hipGetLastError(); return VTX_OK;
        }
        return sweep_path ? diag_sweep_path(ch) : diag_round3_path(ch);
    }
    // the records band_diag_kernel left: with a tight list (round 6) every task that holds a certificate and a one-diagonal
    // band, for band_corridor_kernel; else (VTX_BAND_NO_TIGHT, libvtx_dev.so's VTX_BAND_NO_CORRIDOR) round 3's, for band_refine_kernel
    hipError_t second_look(const Chunk& ch, uint32_t n_rec, hipStream_t st) {
        if (tight_list && !kn.no_corridor) return vtxk_launch_band_corridor(a, refine_list, n_rec, routes, &d_cnt->lists.refine, st);
        return vtxk_launch_band_refine(a, refine_list, n_rec, sh, ch.tb, routes, &d_cnt->lists.refine, st);
    }
    // What the stage left, in two branches over disjoint tasks: side stream — band_tail_kernel (tail_on_side), band_refine_kernel / band_corridor_kernel over its records, then the masked DP over the
    // one-diagonal bands; this stream — band_sweep_kernel + masked DP over the repeats and the short fail list.  One host round trip, right after band_diag_kernel.  (VTX_BAND_NO_TIGHT: the
    // refinement's leftovers go to the fail list, so everything stays in order on this stream.)
    // (the two branches: a tight list to feed the side one, and no VTX_BAND_NO_FORK)
    bool fork_on() const { return tight_list != nullptr && !kn.no_fork; }
    // band_tail_kernel on the side stream, behind band_diag_kernel (EV_DIAG_END) and beside everything the main stream does from there on.  A task deferred to it passed back_harmless,
    // so with a tight list it ends decided, as a refine / corridor record or as a tight entry (vtx_band.hip: band_tail_kernel): lists.run_left and lists.dense, which the main branch
    // starts from, are final when band_diag_kernel ends, and the side branch reads its own two counts on the device.  The kernel gets no fail_list and no dense_list: those are the main
    // branch's.  d_tail is free again at EV_BRANCH_END, which the main stream joins before the next chunk.
    // (It does not wait for the recheck on the main stream either.  Measured: started behind that kernel instead of beside it, the recheck takes what it takes beside the tail,
    // 0.19 ms — it is a few hundred wavefronts of dependent LDS round trips, not a matter of room — and the step loses 0.17 ms: DESIGN.md 4.3.7.)
    int tail_on_side(const Chunk& ch) {
        HIP_TRY(c, hipStreamWaitEvent(s2, c->ev[EV_DIAG_END], 0));
        HIP_TRY(c, hipEventRecord(c->ev[EV_BRANCH_START], s2));
        vtx_diag_routes side = routes;
        side.fail_list = nullptr; side.dense_list = nullptr;
        HIP_TRY(c, vtxk_launch_band_tail(a, sh, side, ch.tail, 1, s2));
        return VTX_OK;
    }
    int diag_sweep_path(Chunk& ch) {
        ch.diag = true; ch.swept = true; sweep_used = true;
        HIP_TRY(c, hipEventRecord(c->ev[EV_DIAG_END], s));
        const bool fork = fork_on();
        hipStream_t sb = fork ? s2 : s;                                             // the refine / one-diagonal branch
        if (ch.tail_side) { if (int rc = tail_on_side(ch)) return rc; }             // (before the host waits: it starts while band_diag_kernel drains)
        if (!fork && refine_list) HIP_TRY(c, second_look(ch, std::min(refine_cap, ch.nt), s));
        // The recheck, on THIS stream, in front of the counter copy: it appends to the fail (or dense) list what it does not clear and to the refine / tight lists what it does — beside
        // band_tail_kernel on the side stream, through the same atomics — so the four counts below include everything it listed: run_left and dense are final, refine and tight are
        // the bounds they were.  Its grid comes from the buffer's capacity and it reads its record count on the device: no round trip of its own.
        if (ch.recheck.cap) {
            HIP_TRY(c, vtxk_launch_band_recheck(a, sh, routes, ch.recheck, s));
            ++rs.launches;
        }
        vtx_band_counters::lists_t& pin = c->h_pin->lists;
        HIP_TRY(c, read_back(pin, d_cnt->lists, s));
        if (ch.tail_side) HIP_TRY(c, read_back(c->h_pin->tail, d_cnt->tail, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        // band_tail_kernel on the side stream: refine and tight are what that kernel had appended when the copy ran, and every one of its n_tail records may still become a record for the
        // second look or, that buffer full, a tight entry.  These two are BOUNDS for the grids; the kernels read the final counts on the device, the figures of vtx_timing arrive with the events.
        const uint32_t n_tail = ch.tail_side ? std::min(c->h_pin->tail, ch.tail.cap) : 0u;
        const uint32_t n_refine = (uint32_t)std::min<uint64_t>((uint64_t)pin.refine + n_tail, refine_cap);
        // (forked: the tight list still grows by what the refinement leaves — at most its records)
        const uint32_t n_tight = (uint32_t)std::min<uint64_t>((uint64_t)pin.tight + (fork && refine_list ? n_refine : 0u) + n_tail, ch.nt);
        if (!ch.tail_side) refined_total += n_refine;                               // (else: collect_sweep_times)
        rs.launches += 2;
        if (fork && !ch.tail_side) HIP_TRY(c, hipStreamWaitEvent(s2, c->ev[EV_DIAG_END], 0));
        if (!ch.tail_side) HIP_TRY(c, hipEventRecord(c->ev[EV_BRANCH_START], sb));
        if (fork && refine_list && n_refine) HIP_TRY(c, second_look(ch, n_refine, sb));
        if (n_tight) { if (int rc = one_diagonal_dp(n_tight, fork, sb)) return rc; }
        if (fork) HIP_TRY(c, read_back(c->h_pin->fork_tight, d_cnt->lists.tight, sb));   // the list's final length (read in collect_sweep_times)
        if (ch.tail_side) HIP_TRY(c, read_back(c->h_pin->fork_refine, d_cnt->lists.refine, sb));   // ... and the records' final count
        HIP_TRY(c, hipEventRecord(c->ev[EV_BRANCH_END], sb));
        if (fork) HIP_TRY(c, hipEventRecord(c->ev[EV_FORK_START], s));                          // (this stream's branch starts here)
        ch.n_fail = pin.run_left;
        const uint32_t n_dense = std::min(pin.dense, ch.nt);
        if (!fork) checked_total += n_tight;                                    // (forked: the exact count arrives with the events)
        diag_total += ch.nt; diag_left += (uint64_t)ch.n_fail + n_dense;
        if (int rc = repeats(ch, n_dense)) return rc;
        // the others: band_run_kernel (task-list mode) in run_stage — seeds, chain and the general certificate (a read against the
        // other allele of an indel lies on TWO diagonals: cert == ub decides nearly all of those without a DP cell)
        if (int rc = sort_by_task(c->d_fail.as<uint32_t>(), c->d_fail.as<uint32_t>() + ch.nt, ch.n_fail, &ch.fail_list)) return rc;
        if (fork) HIP_TRY(c, hipStreamWaitEvent(s, c->ev[EV_BRANCH_END], 0));                    // join: what follows reads every score
        HIP_TRY(c, hipEventRecord(c->ev[EV_SWEEP_END], s));
        open_sweep = OpenSweep{true, fork, ch.tail_side, ch.nt};
        return VTX_OK;
    }
    // tasks with a certificate but no verdict: their band is one diagonal stretch (tight_pack): the masked DP expands it itself.  (VTX_BAND_CHECK=1: the full-matrix check first — full == cert
    // decides a task, cert <= banded <= full; measured: 5.6 ns per task against 10 for the DP it saves on 20 - 30 % of noisy reads.)
    int one_diagonal_dp(uint32_t n_tight, bool fork, hipStream_t sb) {
        const uint32_t *dp_list = tight_list, *dp_pack = tight_pack, *dp_cnt = fork ? &d_cnt->lists.tight : nullptr;
        if (kn.use_check) {
            HIP_TRY(c, c->d_dband.reserve((size_t)bp.chunk * sizeof(uint32_t)));
            HIP_TRY(c, c->d_dband_pack.reserve((size_t)bp.chunk * sizeof(uint32_t)));
            HIP_TRY(c, zero(d_cnt->check, sb));
            HIP_TRY(c, vtxk_launch_sw_check(a, shape[0], shape[1], n_tight, tight_list, tight_pack, dp_cnt, mh, c->d_dband.as<uint32_t>(), c->d_dband_pack.as<uint32_t>(), &d_cnt->check, rs.stage, sb));
            dp_list = c->d_dband.as<uint32_t>(); dp_pack = c->d_dband_pack.as<uint32_t>(); dp_cnt = &d_cnt->check;
            ++rs.launches;
        }
        HIP_TRY(c, vtxk_launch_sw_diag_band(a, shape[0], shape[1], n_tight, dp_list, dp_pack, dp_cnt, mh, rs.stage, sb));
        ++rs.launches;
        return VTX_OK;
    }
    // repeats: band_sweep_kernel (the band of ANY task) + masked DP, sorted by task; what it declines waits in d_over[2 n_tasks ..) for the general band kernel after the last chunk (a short list of the
    // other tasks is not worth band_run_kernel's launch — a persistent grid: ~1 ms whatever the count — and the two host round trips behind it: it joins the repeats, ~25 ns per task)
    int repeats(Chunk& ch, uint32_t n_dense) {
        if (ch.n_fail && ch.n_fail < kn.run_min && (uint64_t)n_dense + ch.n_fail <= ch.nt) {
            HIP_TRY(c, hipMemcpyAsync(dense_list + n_dense, c->d_fail.as<uint32_t>(), (size_t)ch.n_fail * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
            n_dense += ch.n_fail;
            ch.n_fail = 0;
        }
        if (!n_dense) return VTX_OK;
        const uint32_t* dl = nullptr;
        if (int rc = sort_by_task(dense_list, dense_list + ch.nt, n_dense, &dl)) return rc;
        // Second stage (round 5): band_diag2_kernel + band_stream_kernel + the full-matrix check
        const uint32_t* sl = dl;
        uint32_t n_sweep = n_dense;
        if (second_stage_on(n_dense)) {
            uint32_t* sweep2 = (dl == dense_list) ? dense_list + ch.nt : dense_list;          // (the half of d_dense the list is not in)
            if (int rc = second_stage(dl, n_dense, ch.tb, sweep2, &n_sweep)) return rc;
            sl = sweep2;
        }
        if (n_sweep) { if (int rc = sweep_slices(sl, n_sweep, c->d_over.as<uint32_t>() + 2 * bp.n_tasks, &d_cnt->sweep)) return rc; }
        swept_total += n_sweep;
        return VTX_OK;
    }
    // round 3's path (VTX_BAND_LEGACY, or a haplotype above band_sweep_kernel's 255 bases): band_refine_kernel, then band_run_kernel over the fail list
    int diag_round3_path(Chunk& ch) {
        ch.diag = true;
        vtx_band_counters::lists_t& pin = c->h_pin->lists;              // (this path has a fail list and records, no dense or tight list: it copies and reads those two words)
        HIP_TRY(c, read_back(pin.run_left, d_cnt->lists.run_left, s));
        HIP_TRY(c, read_back(pin.refine, d_cnt->lists.refine, s));
        HIP_TRY(c, hipEventRecord(c->ev[EV_DIAG_END], s));
        HIP_TRY(c, hipStreamSynchronize(s));
        ch.n_fail = pin.run_left;
        const uint32_t n_refine = std::min(pin.refine, refine_cap);
        if (n_refine) {
            HIP_TRY(c, vtxk_launch_band_refine(a, refine_list, n_refine, sh, ch.tb, routes, nullptr, s));          // (this path has no tight list: routes.tight_list == nullptr)
            HIP_TRY(c, read_back(pin.run_left, d_cnt->lists.run_left, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            ch.n_fail = pin.run_left;
            refined_total += n_refine;
            ++rs.launches;
        }
        diag_total += ch.nt; diag_left += ch.n_fail;
        ++rs.launches;
        return sort_by_task(c->d_fail.as<uint32_t>(), c->d_fail.as<uint32_t>() + ch.nt, ch.n_fail, &ch.fail_list);
    }
    // band_run_kernel over what is left (the whole range when band_diag_kernel did not run), its second chance and pending records,
    // the masked DP over its hard list; after the last chunk of a pass without a sweep, the general kernel's start
    int run_stage(Chunk& ch) {
        HIP_TRY(c, hipEventRecord(c->ev[EV_BAND_RUN_START], s));
        if (!ch.diag || ch.n_fail) HIP_TRY(c, zero(d_cnt->block, s));      // (here, not per chunk: band_diag_kernel's claim loop, where libvtx_dev.so runs it, has counted in them since)
        if (!ch.diag || ch.n_fail) HIP_TRY(c, vtxk_launch_band_run(a, ch.diag ? ch.n_fail : ch.nt, ch.diag ? 0u : (uint32_t)ch.base, sh, ch.tb, run_out, c->d_band_ws.as<uint32_t>(), c->d_pend.as<uint32_t>(),
            c->d_pend_buf.as<uint32_t>(), bp.hard_cap, bp.pend_cap, ch.diag ? ch.fail_list : nullptr, c->band_long_lists ? 1 : 0, s));
        HIP_TRY(c, hipEventRecord(c->ev[EV_BAND_RUN_END], s));                  // (complete once the read-back below is: no synchronisation of its own)
        const bool run_skipped = ch.swept && ch.n_fail == 0;             // nothing went to band_run_kernel: its counters are what they were
        if (run_skipped) {
            cnt.hard = 0; cnt.pending = 0; cnt.overflow = over_before;
        } else {
            HIP_TRY(c, read_back(cnt, d_cnt->run, s));
            HIP_TRY(c, hipStreamSynchronize(s));
        }
        if (int rc = second_chance(ch)) return rc;
        over_before = cnt.overflow;
        float ms = 0;
        if (!run_skipped) {
            HIP_TRY(c, hipEventElapsedTime(&ms, ch.swept ? c->ev[EV_BAND_RUN_START] : c->ev[EV_CHUNK_START], c->ev[EV_BAND_RUN_END]));
            rs.band_run_ms += ms;
            if (int rc = collect_sweep_times()) return rc;
        }
        if (ch.diag) { HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[EV_CHUNK_START], c->ev[EV_DIAG_END])); diag_ms += ms; }
        if (!sweep_used && ch.last && cnt.overflow)      // last chunk: the overflow list is complete
            if (int rc = fb.start(0, cnt.overflow)) return rc;
        if (cnt.hard > bp.hard_cap) {               // the excess went to the general kernel's list: slots in use = hard_cap
            cnt.hard = bp.hard_cap;
            HIP_TRY(c, hipMemcpyAsync(&d_cnt->run.hard, &cnt.hard, sizeof cnt.hard, hipMemcpyHostToDevice, s));
        }
        cnt.pending = std::min(cnt.pending, bp.pend_cap);
        if (cnt.pending) {
            // tasks whose piece list overflowed its LDS slots: the same certificate, from their pending records
            HIP_TRY(c, vtxk_launch_band_pending(a, c->d_pend.as<uint32_t>(), cnt.pending, c->d_pend_buf.as<uint32_t>(), run_out, s));
            HIP_TRY(c, read_back(cnt.hard, d_cnt->run.hard, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            pending_total += cnt.pending;
            ++rs.launches;
        }
        if (int rc = masked_dp(cnt.hard, c->d_hard.as<uint32_t>(), c->d_poly.as<uint16_t>(), c->d_band.as<uint16_t>(), bp.slots, s, VTX_STAGE_RUN_DP)) return rc;
        rs.hard_total += cnt.hard;
        ++rs.launches;
        return VTX_OK;
    }
    // The six-wavefront variant of band_run_kernel keeps 12-entry lists: the tasks that overflowed them ([a0, a1) of the overflow list) get a second chance in the 15-entry variant before the
    // general kernel — what overflows again is appended behind a1 and then moved down to a0. (task-list mode runs the 15-entry variant: nothing to give a second chance to)
    int second_chance(const Chunk& ch) {
        const bool short_lists = !ch.diag && ch.tb.n_loci && vtxk_band_second_chance(bp.tasks_per_locus, c->band_long_lists ? 1 : 0);
        if (short_lists && ch.nt >= (1u << 20)) {
            // feedback for the next run of this context: many overflows of the 12-entry lists (noisy reads: 3.3 % of the
            // tasks at 3 % substitution errors, 0.2 % at 0.5 %) make the 15-entry variant the better first pass
            if ((uint64_t)(cnt.overflow - over_before) * 50 > ch.nt) c->band_long_lists = true;
        }
        if (!short_lists || cnt.overflow <= over_before) return VTX_OK;
        const uint32_t a0 = over_before, a1 = cnt.overflow;
        uint32_t* over = c->d_over.as<uint32_t>();
        HIP_TRY(c, zero(d_cnt->block, s));
        HIP_TRY(c, vtxk_launch_band_run(a, a1 - a0, 0, sh, ch.tb, run_out, c->d_band_ws.as<uint32_t>(), c->d_pend.as<uint32_t>(), c->d_pend_buf.as<uint32_t>(), bp.hard_cap, bp.pend_cap, over + a0, 0, s));
        HIP_TRY(c, hipEventRecord(c->ev[EV_BAND_RUN_END], s));
        HIP_TRY(c, read_back(cnt, d_cnt->run, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        const uint32_t again = cnt.overflow - a1;          // <= a1 - a0: source and destination do not overlap
        if (again) HIP_TRY(c, hipMemcpyAsync(over + a0, over + a1, (size_t)again * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        cnt.overflow = a0 + again;
        HIP_TRY(c, hipMemcpyAsync(&d_cnt->run.overflow, &cnt.overflow, sizeof cnt.overflow, hipMemcpyHostToDevice, s));
        ++rs.launches;
        return VTX_OK;
    }
    // After the last chunk of a pass with a sweep.  What overflowed band_run_kernel's lists (d_over[0, nA)) takes band_sweep_kernel too; then everything the sweep declined — here and in the
    // chunks' own sweeps: d_over[2 n_tasks, + nB), counted on the device — takes the general band kernel.
    int last_chunk() {
        uint32_t *over = c->d_over.as<uint32_t>(), *declined = over + 2 * bp.n_tasks;
        const uint32_t nA = cnt.overflow;
        if (nA) {
            // (these tasks left band_diag_kernel for another reason than their number of matches, and then overflowed band_run_kernel's piece lists: repeats as well — on real-sequence loci 0.9 M
            // tasks.  The second stage first, when the tables of every locus are still resident.)
            const uint32_t* sl = over;
            uint32_t n_sweep = nA;
            if (second_stage_on(nA) && bp.gt_bytes && !gt_chunked && nA <= bp.chunk && c->d_dense.cap >= (size_t)nA * sizeof(uint32_t)) {
                const vtx_band_tables every_locus{c->d_gtables.as<uint8_t>(), bp.gt_bytes, 0, c->n_loci};
                if (int rc = second_stage(over, nA, every_locus, c->d_dense.as<uint32_t>(), &n_sweep)) return rc;
                sl = c->d_dense.as<uint32_t>();
            }
            if (n_sweep) { if (int rc = sweep_slices(sl, n_sweep, declined, &d_cnt->sweep)) return rc; }
            swept_total += n_sweep;
        }
        uint32_t nB = 0;                            // what band_sweep_kernel declines (bytes outside ACGTN, > 255 bases, > 1 024 sections, a full stash bucket)
        HIP_TRY(c, read_back(nB, d_cnt->sweep.overflow, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        if (int rc = collect_sweep_times()) return rc;
        cnt.overflow = nB;
        if (nB) { if (int rc = fb.start((uint32_t)(2 * bp.n_tasks), (uint32_t)(2 * bp.n_tasks) + nB)) return rc; }
        return VTX_OK;
    }
    // the general kernel's end; the pass's times and task counts ADDED to the run's; the VTX_DEBUG lines
    int publish() {
        const uint32_t fast_overflow = cnt.overflow;
        if (kn.debug) {
            vtx_band_counters::run_t run;
            HIP_TRY(c, hipMemcpy(&run, &d_cnt->run, sizeof run, hipMemcpyDeviceToHost));
            const uint32_t* run_why = run.why;
            fprintf(stderr, "[vtx] band_run_kernel: %u tasks hard only because pieces were dropped from a full list\n", run.dropped);
            fprintf(stderr, "[vtx] band_run_kernel overflow reasons: bound=%u parked-full=%u log-full=%u other=%u traceback=%u\n", run_why[1], run_why[2], run_why[3], run_why[4], run_why[5]);
        }
        if (int rc = fb.finish()) return rc;
        c->fast_overflow += fast_overflow;
        c->timing.diag_ms += diag_ms; c->timing.diag_left += (uint32_t)std::min<uint64_t>(diag_left, 0xffffffffull);
        c->timing.check_ms += check_ms; c->timing.sweep_ms += sweep_ms;
        c->timing.swept_tasks += (uint32_t)std::min<uint64_t>(swept_total, 0xffffffffull);
        c->timing.diag2_tasks += (uint32_t)std::min<uint64_t>(diag2_total, 0xffffffffull);
        c->timing.diag2_scored += (uint32_t)std::min<uint64_t>(diag2_scored, 0xffffffffull);
        c->timing.diag2_streamed += (uint32_t)std::min<uint64_t>(stream_total, 0xffffffffull);
        checked_total += tight2_total;                     // (one-diagonal bands of the second stage: the same masked DP)
        c->timing.checked_tasks += (uint32_t)std::min<uint64_t>(checked_total, 0xffffffffull);
        if (swept_total) rs.hard_total += (uint32_t)std::min<uint64_t>(swept_total - std::min<uint64_t>(swept_total, fast_overflow), 0xffffffffull);
        rs.hard_total += (uint32_t)std::min<uint64_t>(checked_total, 0xffffffffull);      // (tasks with a certificate: masked DP over their diagonal band; with VTX_BAND_CHECK an upper bound)
        if (kn.debug && diag_total) {
            vtx_band_counters all;
            HIP_TRY(c, hipMemcpy(&all, d_cnt, sizeof all, hipMemcpyDeviceToHost));
            const uint32_t* why = all.diag_why;
            fprintf(stderr, "[vtx] band_refine_kernel: %llu tasks listed\n", (unsigned long long)refined_total);
            fprintf(stderr, "[vtx] band_diag_kernel: %llu of %llu tasks left to band_run_kernel (%.2f %%), %.2f ms: shape=%u no-diagonal=%u pieces=%u matches=%u not-harmless=%u generic=%u not-tight=%u no-main=%u\n",
                    (unsigned long long)diag_left, (unsigned long long)diag_total, 100.0 * (double)diag_left / (double)diag_total, (double)diag_ms, why[1], why[2], why[3], why[4], why[5], why[7], why[8], why[9]);
            fprintf(stderr, "[vtx] band_tail_kernel, recheck: %u tasks that failed band_diag_kernel's harmless test rechecked, %u cleared\n", all.recheck_total, all.recheck_cleared);
            if (VTX_DEVTOOLS_ON) fprintf(stderr, "[vtx] band_tail_kernel: %u records routed towards the dense or fail list beside a tight list\n", all.tail_stray);
        }
        if (kn.debug && diag2_total) fprintf(stderr, "[vtx] band_diag2_kernel: %llu tasks looked at, %llu scored, %llu left with a one-diagonal band, %llu to band_sweep_kernel (%llu through band_stream_kernel)\n",
            (unsigned long long)diag2_total, (unsigned long long)diag2_scored, (unsigned long long)tight2_total, (unsigned long long)(diag2_total - diag2_scored - tight2_total), (unsigned long long)stream_total);
        if (kn.debug) fprintf(stderr, "[vtx] banded: %llu tasks, %u overflowed band_run_kernel, %u bounded by the pending kernel, %u hard\n", (unsigned long long)bp.n_tasks, fast_overflow, pending_total, rs.hard_total);
        return VTX_OK;
    }
};

// ---- vtx_run: its stages ----------------------------------------------------------------------------------------------------------
// The banded stages ADD their times and task counts per pass (BandPass::publish): zeroed here, for every run — a run that does not enter them (an empty batch, a batch of slow records only) must
// not report the previous batch's.  Then the test / audit hooks (vtx_set_debug): poison the score arrays so that a stage that fails to write a task's score cannot hide behind the previous run's
// value; one byte per task saying which stage decided it (vtx_fetch_stage).
int run_prologue(vtx_ctx* c, RunState& rs) {
    hipStream_t s = c->stream;
    const uint32_t nr = c->n_records;
    c->ran = false;
    c->fast_overflow = 0;
    c->timing.diag_ms = c->timing.check_ms = c->timing.sweep_ms = 0;
    c->timing.diag_left = c->timing.checked_tasks = c->timing.swept_tasks = 0;     // (resweep_tasks: never set, see vtx.h)
    c->timing.diag2_tasks = c->timing.diag2_scored = c->timing.diag2_streamed = 0;
    rs.a = vtx_task_arrays{c->d_records.as<vtx_record>(), c->d_rec_locus.as<uint32_t>(), c->d_loci.as<vtx_locus>(), c->d_read.as<uint8_t>(), c->d_hap.as<uint8_t>(), c->d_ref.as<int32_t>(), c->d_alt.as<int32_t>()};
    if (c->stage_trace && nr) {
        HIP_TRY(c, c->d_stage.reserve(2 * (size_t)nr));
        rs.stage = c->d_stage.as<uint8_t>();
        HIP_TRY(c, hipMemsetAsync(rs.stage, c->cfg.aligner == VTX_ALIGNER_BANDED ? VTX_STAGE_UNKNOWN : VTX_STAGE_FULL_DP, 2 * (size_t)nr, s));
    }
    if (c->poison && nr) {
        HIP_TRY(c, vtxk_fill_i32(rs.a.ref, nr, c->poison_value, s));
        HIP_TRY(c, vtxk_fill_i32(rs.a.alt, nr, c->poison_value, s));
    }
    HIP_TRY(c, hipEventRecord(c->ev[EV_START], s));
    return VTX_OK;
}
// The full-matrix DP, one launch per bucket of records (the banded flavour never runs it), and the generic (byte-equality) kernel
// again over the records with bytes outside ACGTN that the table kernels listed.
int run_full_dp(vtx_ctx* c, RunState& rs) {
    hipStream_t s = c->stream;
    const BandKnobs& kn = band_knobs();
    const vtx_task_arrays& a = rs.a;
    const uint32_t mh = c->max_hap_len;
    uint32_t *work = c->d_work.as<uint32_t>(), *d_redo = c->d_redo.as<uint32_t>();
    bool any_lut = false; const bool full_dp = c->cfg.aligner != VTX_ALIGNER_BANDED;
    for (const Bucket& bk : c->buckets) any_lut |= bk.lut || bk.duo;
    any_lut &= full_dp;
    if (any_lut) HIP_TRY(c, hipMemsetAsync(c->d_redo_cnt.p, 0, 16 * sizeof(uint32_t), s));
    for (size_t b = 0; full_dp && b < c->buckets.size(); ++b) {
        const Bucket& bk = c->buckets[b];
        const bool use_pair = bk.pair && !kn.no_pair;
        uint32_t* redo_cnt = c->d_redo_cnt.as<uint32_t>() + b;
        if (bk.duo && !kn.no_duo) HIP_TRY(c, vtxk_launch_sw_full_duo(a, bk.R, bk.count, work + bk.offset, mh, use_pair ? kPairLociCap : duo_loci_cap(mh), d_redo + bk.offset, redo_cnt, use_pair ? duo_pair_cols(mh) : 0u, s));
        else if (bk.lut) HIP_TRY(c, vtxk_launch_sw_full_lut(a, bk.R, bk.count, work + bk.offset, mh, kLutLociCap, d_redo + bk.offset, redo_cnt, s));
        else HIP_TRY(c, vtxk_launch_sw_full(a, bk.R, bk.GL, bk.count, work + bk.offset, mh, s));
        ++rs.launches;
    }
    if (any_lut) {
        uint32_t redo[16] = {0};
        HIP_TRY(c, hipMemcpyAsync(redo, c->d_redo_cnt.p, sizeof redo, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        for (size_t b = 0; b < c->buckets.size(); ++b) {
            const Bucket& bk = c->buckets[b];
            if (!(bk.lut || bk.duo) || !redo[b]) continue;
            HIP_TRY(c, vtxk_launch_sw_full(a, bk.R, bk.GL, redo[b], d_redo + bk.offset, mh, s));
            ++rs.launches;
        }
    }
    HIP_TRY(c, hipEventRecord(c->ev[EV_FULL_END], s));
    return VTX_OK;
}
// One pass, or two when a few loci have haplotypes above 255 bases (the shape per task of round 6: DESIGN.md 4.3.1, "Host orchestration"): every locus up
// to 255 bases as if the others were not there, then the stretch of tasks from the first to the last long locus with round 3's kernels.
int run_banded(vtx_ctx* c, RunState& rs) {
    hipStream_t s = c->stream; const uint32_t nr = c->n_records;
    const bool split = !band_knobs().no_split && c->max_hap_len > 255 && c->hap_short_max > 0 && c->n_long_loci > 0 && (uint64_t)c->n_long_loci * 8 <= c->n_loci;
    if (!split) return BandPass(c, rs, c->max_hap_len, 0, 0, 2ull * nr, false).run();
    if (int rc = BandPass(c, rs, c->hap_short_max, 0, 0, 2ull * nr, false).run()) return rc;
    vtx_locus ends[2];
    HIP_TRY(c, hipMemcpyAsync(&ends[0], rs.a.loci + c->long_first, sizeof(vtx_locus), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&ends[1], rs.a.loci + c->long_last, sizeof(vtx_locus), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const uint64_t t0 = 2ull * std::min(ends[0].rec_begin, nr), t1 = 2ull * std::min<uint64_t>((uint64_t)ends[1].rec_begin + ends[1].rec_count, nr);
    if (t1 > t0) return BandPass(c, rs, c->max_hap_len, 255, t0, t1, true).run();
    return VTX_OK;
}
// records beyond the fast kernels' limits: exact slow path, both flavours (slabs grow until every chain fits)
int run_slow(vtx_ctx* c, RunState& rs) {
    hipStream_t s = c->stream;
    const uint32_t n_slow = 2 * c->slow_cnt;
    const int banded = c->cfg.aligner == VTX_ALIGNER_BANDED;
    if (rs.stage) HIP_TRY(c, vtxk_mark_stage_records(c->d_work.as<uint32_t>() + c->slow_off, c->slow_cnt, VTX_STAGE_SLOW, rs.stage, s));
    HIP_TRY(c, c->d_cnt.reserve(sizeof(vtx_band_counters)));
    uint32_t* d_scnt = &c->d_cnt.as<vtx_band_counters>()->slow;
    HIP_TRY(c, c->d_slow_retry.reserve(2 * (size_t)n_slow * sizeof(uint32_t)));
    const uint32_t* tasks = nullptr; uint32_t todo = n_slow, cap = 1024;
    const uint32_t mh = std::max(c->max_hap_all, 1u);
    for (;;) {
        const uint64_t worst = (uint64_t)c->max_read_all * mh;
        const size_t stride = vtxk_slow_ws_stride(cap, mh, c->max_read_all);
        HIP_TRY(c, c->d_slow_ws.reserve((size_t)todo * stride));
        HIP_TRY(c, hipMemsetAsync(d_scnt, 0, sizeof *d_scnt, s));
        uint32_t* retry = c->d_slow_retry.as<uint32_t>() + ((tasks == c->d_slow_retry.as<uint32_t>()) ? n_slow : 0);
        HIP_TRY(c, vtxk_launch_slow_align(rs.a, c->d_work.as<uint32_t>() + c->slow_off, tasks, todo, banded, c->d_slow_ws.as<uint8_t>(), stride, cap, mh, c->max_read_all, retry, d_scnt, s));
        uint32_t left = 0;
        HIP_TRY(c, hipMemcpyAsync(&left, d_scnt, sizeof left, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        ++rs.launches;
        if (!left) return VTX_OK;
        if (cap >= worst) return fail(c, VTX_E_STATE, "vtx_run: slow path overflow with a worst-case slab");
        cap = (uint32_t)std::min<uint64_t>((uint64_t)cap * 16, std::max<uint64_t>(worst, 1024));
        tasks = retry; todo = left;
    }
}
// The call reduction: scores -> triplets; *nnz32 arrives with the stream's next synchronisation. Short groups (the mean at most kReduceMeanGroupMax records): one thread per group counts its
// records in registers, twice — once for the kept groups per block, once to emit behind the scanned block counts (d_keep / d_keep_scan hold one word per block of groups then).  Deep groups: a
// histogram with atomics, one thread per record.
int run_reduce(vtx_ctx* c, const RunState& rs, uint32_t* nnz32) {
    hipStream_t s = c->stream;
    const uint32_t nr = c->n_records, ng = c->n_cell_groups, nu = c->n_umi_groups;
    const int32_t *ref = rs.a.ref, *alt = rs.a.alt;
    uint32_t mean_max = kReduceMeanGroupMax;
    if (VTX_DEV_ENV("VTX_REDUCE_THRESHOLD")) mean_max = (uint32_t)strtoul(VTX_DEV_ENV("VTX_REDUCE_THRESHOLD"), nullptr, 10);   // test hook (read per run)
    const bool legacy = VTX_DEV_ENV("VTX_REDUCE_LEGACY") && atoi(VTX_DEV_ENV("VTX_REDUCE_LEGACY"));                            // A/B and test hook (read per run)
    const bool onepass = !legacy && (uint64_t)nr <= (uint64_t)mean_max * ng;
    c->reduce_path = nr ? (onepass ? 2 : 1) : 0;
    uint32_t *keep = c->d_keep.as<uint32_t>(), *keep_scan = c->d_keep_scan.as<uint32_t>();
    if (nr && onepass) {
        const uint32_t nb = vtxk_reduce_blocks(ng);
        HIP_TRY(c, vtxk_reduce_count(ref, alt, c->d_head_umi.as<uint32_t>(), c->d_grp_start.as<uint32_t>(), ng, c->cfg.min_score, c->cfg.use_umi, c->cfg.scoring_mode, keep, s));
        HIP_TRY(c, vtxk_inclusive_scan_u32(keep, keep_scan, nb, c->d_scan_tmp.p, vtxk_scan_temp_bytes(nr), s));
        HIP_TRY(c, vtxk_reduce_emit(ref, alt, c->d_head_umi.as<uint32_t>(), c->d_grp_start.as<uint32_t>(), ng, c->cfg.min_score, c->cfg.use_umi, c->cfg.scoring_mode, keep_scan, c->d_grp_row.as<uint32_t>(), c->d_grp_col.as<uint32_t>(),
                c->d_o_row.as<uint32_t>(), c->d_o_col.as<uint32_t>(), c->d_o_alt.as<uint32_t>(), c->d_o_ref.as<uint32_t>(), c->d_o_unk.as<uint32_t>(), c->d_o_val.as<double>(), c->d_o_refval.as<double>(), s));
        if (nb) HIP_TRY(c, hipMemcpyAsync(nnz32, keep_scan + (nb - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    } else if (nr) {
        const size_t tmp_bytes = vtxk_scan_temp_bytes(nr);
        uint32_t* cell_cnt = c->d_cell_cnt.as<uint32_t>();
        HIP_TRY(c, hipMemsetAsync(cell_cnt, 0, 3 * (size_t)ng * sizeof(uint32_t), s));
        if (c->cfg.use_umi) {
            HIP_TRY(c, hipMemsetAsync(c->d_umi_cnt.p, 0, 3 * (size_t)nu * sizeof(uint32_t), s));
            HIP_TRY(c, vtxk_count_calls(ref, alt, nr, c->cfg.min_score, c->d_umi_scan.as<uint32_t>(), c->d_umi_cnt.as<uint32_t>(), s));
            HIP_TRY(c, vtxk_umi_collapse(c->d_umi_cnt.as<uint32_t>(), nu, c->d_umi_cellgrp.as<uint32_t>(), cell_cnt, s));
        } else {
            HIP_TRY(c, vtxk_count_calls(ref, alt, nr, c->cfg.min_score, c->d_cell_scan.as<uint32_t>(), cell_cnt, s));
        }
        HIP_TRY(c, vtxk_keep_flags(cell_cnt, ng, c->cfg.scoring_mode, keep, s));
        HIP_TRY(c, vtxk_inclusive_scan_u32(keep, keep_scan, ng, c->d_scan_tmp.p, tmp_bytes, s));
        HIP_TRY(c, vtxk_emit_coo(cell_cnt, ng, c->cfg.scoring_mode, keep, keep_scan, c->d_grp_row.as<uint32_t>(), c->d_grp_col.as<uint32_t>(), c->d_o_row.as<uint32_t>(), c->d_o_col.as<uint32_t>(), c->d_o_alt.as<uint32_t>(),
                c->d_o_ref.as<uint32_t>(), c->d_o_unk.as<uint32_t>(), c->d_o_val.as<double>(), c->d_o_refval.as<double>(), s));
        if (ng) HIP_TRY(c, hipMemcpyAsync(nnz32, keep_scan + (ng - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipEventRecord(c->ev[EV_REDUCE_END], s));
    return VTX_OK;
}

int run_epilogue(vtx_ctx* c, const RunState& rs) {
    float t01 = 0, t12 = 0, t03 = 0;
    HIP_TRY(c, hipEventElapsedTime(&t03, c->ev[EV_START], c->ev[EV_FULL_END])); c->timing.full_ms = t03;
    HIP_TRY(c, hipEventElapsedTime(&t01, c->ev[EV_START], c->ev[EV_DP_END])); c->timing.band_ms = t01 - t03;
    HIP_TRY(c, hipEventElapsedTime(&t12, c->ev[EV_DP_END], c->ev[EV_REDUCE_END]));
    c->timing.sw_ms = t01; c->timing.reduce_ms = t12; c->timing.total_ms = t01 + t12;
    c->timing.sw_launches = rs.launches; c->timing.hard_tasks = rs.hard_total;
    c->timing.band_run_ms = rs.band_run_ms; c->timing.overflow_tasks = c->fast_overflow;
    return VTX_OK;
}

}  // namespace

extern "C" {

int vtx_run(vtx_ctx* c) {
    if (!c) return VTX_E_INVAL;
    if (!c->submitted) return fail(c, VTX_E_STATE, "vtx_run: no batch submitted");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    RunState rs;
    if (int rc = run_prologue(c, rs)) return rc;
    if (int rc = run_full_dp(c, rs)) return rc;
    if (c->cfg.aligner == VTX_ALIGNER_BANDED && c->n_records) { if (int rc = run_banded(c, rs)) return rc; }
    if (c->slow_cnt) { if (int rc = run_slow(c, rs)) return rc; }
    HIP_TRY(c, hipEventRecord(c->ev[EV_DP_END], c->stream));
    uint32_t nnz32 = 0;
    if (int rc = run_reduce(c, rs, &nnz32)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->nnz = nnz32;
    if (int rc = run_epilogue(c, rs)) return rc;
    c->ran = true;
    return VTX_OK;
}

int vtx_fetch_scores(vtx_ctx* c, int32_t* ref_score, int32_t* alt_score) {
    if (!c) return VTX_E_INVAL;
    if (!c->ran) return fail(c, VTX_E_STATE, "vtx_fetch_scores: no completed vtx_run");
    if (c->n_records && (!ref_score || !alt_score)) return fail(c, VTX_E_INVAL, "vtx_fetch_scores: null output");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (c->n_records) {
        HIP_TRY(c, hipMemcpy(ref_score, c->d_ref.p, (size_t)c->n_records * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(alt_score, c->d_alt.p, (size_t)c->n_records * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return VTX_OK;
}

#ifdef VTX_DEVTOOLS
// developer library only (not part of include/vtx.h): which call reduction the last vtx_run took — 0 none (no records),
// 1 the histogram kernels, 2 one pass per group
extern "C" int vtx_dev_reduce_path(vtx_ctx* c) { return c ? c->reduce_path : -1; }
#endif

int vtx_set_debug(vtx_ctx* c, int key, int64_t value) {
    if (!c) return VTX_E_INVAL;
    switch (key) {
        case VTX_DEBUG_STAGE_TRACE: c->stage_trace = value != 0; return VTX_OK;
        case VTX_DEBUG_POISON_SCORES: c->poison = value != 0; return VTX_OK;
        case VTX_DEBUG_POISON_VALUE: c->poison_value = (int32_t)value; return VTX_OK;
        default: return fail(c, VTX_E_INVAL, "vtx_set_debug: unknown key %d", key);
    }
}

int vtx_fetch_stage(vtx_ctx* c, uint8_t* stage) {
    if (!c) return VTX_E_INVAL;
    if (!c->ran) return fail(c, VTX_E_STATE, "vtx_fetch_stage: no completed vtx_run");
    if (!c->stage_trace || (c->n_records && c->d_stage.cap < 2 * (size_t)c->n_records))
        return fail(c, VTX_E_STATE, "vtx_fetch_stage: the last vtx_run was not traced (vtx_set_debug(ctx, VTX_DEBUG_STAGE_TRACE, 1) before it)");
    if (c->n_records && !stage) return fail(c, VTX_E_INVAL, "vtx_fetch_stage: null output");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (c->n_records) HIP_TRY(c, hipMemcpy(stage, c->d_stage.p, 2 * (size_t)c->n_records, hipMemcpyDeviceToHost));
    return VTX_OK;
}

int vtx_set_read_format(vtx_ctx* c, int format) {
    if (!c) return VTX_E_INVAL;
    if (format != VTX_READS_BYTES && format != VTX_READS_NIBBLES) return fail(c, VTX_E_INVAL, "vtx_set_read_format: unknown format %d", format);
    c->read_format = format;
    return VTX_OK;
}

int vtx_debug_tables(vtx_ctx* c, void* dst, uint64_t cap, uint64_t* bytes) {
    if (!c || !bytes) return VTX_E_INVAL;
    *bytes = 0;
    if (!c->submitted) return fail(c, VTX_E_STATE, "vtx_debug_tables: no batch submitted");
    if (cap && !dst) return fail(c, VTX_E_INVAL, "vtx_debug_tables: null destination");
    *bytes = c->gt_used;
    const size_t n = (size_t)std::min<uint64_t>(cap, c->gt_used);
    if (!n) return VTX_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(dst, c->d_gtables.p, n, hipMemcpyDeviceToHost));
    return VTX_OK;
}

int vtx_debug_bands(vtx_ctx* c, const uint32_t* tasks, uint32_t n_tasks, uint32_t stride, uint16_t* lo, uint16_t* hi, uint8_t* status) {
    if (!c) return VTX_E_INVAL;
    if (!c->submitted) return fail(c, VTX_E_STATE, "vtx_debug_bands: no batch submitted");
    if (!n_tasks) return VTX_OK;
    if (!tasks || !lo || !hi || !status) return fail(c, VTX_E_INVAL, "vtx_debug_bands: null array");
    if (stride < c->max_hap_all + 1) return fail(c, VTX_E_INVAL, "vtx_debug_bands: stride %u < longest haplotype + 1 (%u)", stride, c->max_hap_all + 1);
    for (uint32_t i = 0; i < n_tasks; ++i)
        if (tasks[i] >= 2ull * c->n_records) return fail(c, VTX_E_INVAL, "vtx_debug_bands: task %u out of range", tasks[i]);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    // scratch of its own (one task per launch slot; a debug call may be slow): tasks, hard list, overflow list, counters, bands
    DevBuf d_t, d_h, d_o, d_c, d_b, d_d;
    const uint32_t bs = (stride + 7u) & ~7u;
    auto done = [&](int rc) { d_t.release(); d_h.release(); d_o.release(); d_c.release(); d_b.release(); d_d.release(); return rc; };
#define DBG_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return done(fail(c, VTX_E_HIP, "%s: %s", #expr, hipGetErrorString(e_))); } while (0)
    DBG_TRY(d_t.reserve((size_t)n_tasks * 4)); DBG_TRY(d_h.reserve((size_t)n_tasks * 4)); DBG_TRY(d_o.reserve((size_t)n_tasks * 4));
    DBG_TRY(d_c.reserve(sizeof(vtx_cnt_pair))); DBG_TRY(d_b.reserve((size_t)n_tasks * 2 * bs * sizeof(uint16_t)));
    const bool dbg_on = VTX_DEV_ENV("VTX_SWEEP_DBG") != nullptr;        // developer aid: the kernel's per-task intermediate state on stderr
    if (dbg_on) DBG_TRY(d_d.reserve((size_t)n_tasks * 64 * 4));
    DBG_TRY(hipMemcpyAsync(d_t.p, tasks, (size_t)n_tasks * 4, hipMemcpyHostToDevice, s));
    DBG_TRY(hipMemsetAsync(d_c.p, 0, sizeof(vtx_cnt_pair), s));
    DBG_TRY(c->d_sweep_log.reserve(vtxk_band_sweep_log_bytes()));
    const vtx_task_arrays a{c->d_records.as<vtx_record>(), c->d_rec_locus.as<uint32_t>(), c->d_loci.as<vtx_locus>(), c->d_read.as<uint8_t>(), c->d_hap.as<uint8_t>(), nullptr, nullptr};
    const vtx_band_out out{d_b.as<uint16_t>(), bs, d_h.as<uint32_t>(), d_o.as<uint32_t>(), d_c.as<vtx_cnt_pair>()};
    uint32_t* dbg = dbg_on ? d_d.as<uint32_t>() : nullptr;
    DBG_TRY(vtxk_launch_band_sweep(a, d_t.as<uint32_t>(), n_tasks, nullptr, out, nullptr, nullptr, dbg, c->d_sweep_log.as<uint32_t>(), s));
    vtx_cnt_pair swept{};                    // band_sweep_kernel's two counters: band slots, declined tasks
    DBG_TRY(hipMemcpyAsync(&swept, d_c.p, sizeof swept, hipMemcpyDeviceToHost, s));
    DBG_TRY(hipStreamSynchronize(s));
    std::vector<uint32_t> hard(swept.hard);
    std::vector<uint16_t> bands((size_t)swept.hard * 2 * bs);
    if (swept.hard) {
        DBG_TRY(hipMemcpy(hard.data(), d_h.p, (size_t)swept.hard * 4, hipMemcpyDeviceToHost));
        DBG_TRY(hipMemcpy(bands.data(), d_b.p, bands.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
    }
    if (dbg_on) {
        std::vector<uint32_t> dd((size_t)n_tasks * 64);
        DBG_TRY(hipMemcpy(dd.data(), d_d.p, dd.size() * 4, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n_tasks; ++i) {
            const uint32_t* o = dd.data() + (size_t)i * 64;
            fprintf(stderr, "[sweep dbg] task %u: best dp %u x %u y %u, log %u, sections %u, cA %d cB %d, decline %u, m %u n %u\n  sections:", tasks[i],
                    o[0] >> 16, (o[0] >> 8) & 0xff, o[0] & 0xff, o[1], o[2], (int)o[3], (int)o[4], o[5], o[6], o[7]);
            for (uint32_t k = 0; k < o[2] && k < 12; ++k) fprintf(stderr, " (%u,%u,%u)", o[8 + k] >> 16, (o[8 + k] >> 8) & 0xff, o[8 + k] & 0xff);
            fprintf(stderr, "\n  log:");
            for (uint32_t k = 0; k < o[1] && k < 24; ++k) fprintf(stderr, " (%u,%u<-%04x)", o[20 + k] >> 24, (o[20 + k] >> 16) & 0xff, o[20 + k] & 0xffff);
            fprintf(stderr, "\n  rmin:");
            for (int k = 0; k < 10; ++k) fprintf(stderr, " %d", (int)o[44 + k]);
            fprintf(stderr, "  rmax:");
            for (int k = 0; k < 10; ++k) fprintf(stderr, " %d", (int)o[54 + k]);
            fprintf(stderr, "\n");
        }
    }
#undef DBG_TRY
    // slots come out in any order, and a task may be listed more than once: every occurrence of a task gets the band of one of its slots
    std::vector<std::pair<uint32_t, uint32_t>> by_task(swept.hard);
    for (uint32_t h = 0; h < swept.hard; ++h) by_task[h] = {hard[h], h};
    std::sort(by_task.begin(), by_task.end());
    for (uint32_t i = 0; i < n_tasks; ++i) {
        auto it = std::lower_bound(by_task.begin(), by_task.end(), std::make_pair(tasks[i], 0u));
        if (it == by_task.end() || it->first != tasks[i]) { status[i] = 1; continue; }
        status[i] = 0;
        const uint16_t* src = bands.data() + (size_t)it->second * 2 * bs;
        memcpy(lo + (size_t)i * stride, src, (size_t)stride * sizeof(uint16_t));
        memcpy(hi + (size_t)i * stride, src + bs, (size_t)stride * sizeof(uint16_t));
    }
    return done(VTX_OK);
}

int vtx_device_scores(vtx_ctx* c, const int32_t** d_ref, const int32_t** d_alt) {
    if (!c) return VTX_E_INVAL;
    if (!c->ran) return fail(c, VTX_E_STATE, "vtx_device_scores: no completed vtx_run");
    if (d_ref) *d_ref = c->d_ref.as<int32_t>();
    if (d_alt) *d_alt = c->d_alt.as<int32_t>();
    return VTX_OK;
}

int vtx_fetch_coo(vtx_ctx* c, vtx_coo* out) {
    if (!c) return VTX_E_INVAL;
    if (!out) return fail(c, VTX_E_INVAL, "vtx_fetch_coo: null output");
    if (!c->ran) return fail(c, VTX_E_STATE, "vtx_fetch_coo: no completed vtx_run");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return fetch_arrays(c, c->nnz, c->d_o_row.p, c->d_o_col.p, c->d_o_alt.p, c->d_o_ref.p, c->d_o_unk.p, c->d_o_val.p, c->d_o_refval.p, out);
}

// sprs::io::write_matrix_market of the last vtx_run's triplets (src/main.rs:381-389: three header lines, then "row+1 col+1 value"
// in insertion order), formatted ON THE DEVICE and streamed into the file by the copy workers: the triplets never become host arrays.
// which: 0 = `value` (the matrix), 1 = `ref_value` (coverage mode's ref matrix).
// vtx_write_mtx: only for integral values — consensus 1 / 2 / 3, coverage counts — whose Rust `{}` text is their digits; alt_frac's
// fractions / NaN: VTX_E_UNSUPPORTED, nothing is left at `path`.
// vtx_write_mtx_f64 (real): those too — shortest round-trip digits per lane (vtx_f64_text.h); VTX_E_UNSUPPORTED only for a value outside
// that formatter's domain (nothing vtx_run produces), and then the caller formats on the host (vtx_fetch_coo + vtxh_write_mtx).
// *sum (optional) = the sum of the values (the reference's "matrix has a sum of 0" warning, :410-415), added up in no fixed order; NaN
// when a value is NaN, as the host's `sum += v` gives.
// vtx_write_mtx_gz (gz): the same text, header lines included, as a BGZF file — per pass the text is cut into chunks of vtxd::CHUNK bytes
// (the chunking restarts with every pass; a pass's last chunk may be short), mtx_deflate_kernel makes a gzip member of each, the members
// are compacted and only they are downloaded; the 28-byte empty member ends the file.  real = the values' formatter as above, and the
// same decline rule.  *text_bytes (optional) = the uncompressed size.
// The slab loop is ONE engine with two sinks: a file (vtx_write_mtx*: the copy workers pwrite their pinned buffers) or a host buffer
// (vtx_mtx_part: the same bytes through download(), without header lines and without the end-of-file member).
struct MtxSink {
    int fd = -1;                 // >= 0: the file, written at file_off
    uint64_t file_off = 0;
    uint8_t* buf = nullptr;      // fd < 0: malloc'ed, `len` bytes used of `cap`
    uint64_t len = 0, cap = 0;
};

static int mtx_sink_put(vtx_ctx* c, const char* fn, MtxSink& k, const void* d_src, size_t bytes) {
    if (k.fd >= 0) {
        if (int rc = download_to_fd(c, k.fd, k.file_off, d_src, bytes)) return rc;
        k.file_off += bytes;
        return VTX_OK;
    }
    if (!bytes) return VTX_OK;
    if (k.len + bytes > k.cap) {                          // one pass is the rule: the first allocation is exact
        const uint64_t cap = std::max<uint64_t>(k.len + bytes, k.cap + k.cap / 2);
        uint8_t* p = (uint8_t*)realloc(k.buf, (size_t)cap);
        if (!p) return fail(c, VTX_E_NOMEM, "%s: out of host memory for %llu bytes", fn, (unsigned long long)cap);
        k.buf = p; k.cap = cap;
    }
    if (int rc = download(c, {{k.buf + k.len, d_src, bytes}})) return rc;
    k.len += bytes;
    return VTX_OK;
}

// The lines of the last vtx_run's triplets into `sink`, pass by pass.  head / hl: text that lies in front of the first pass's lines and
// goes through the encoder with them (gz files: the header lines; such a call has a pass even without a triplet); hl = 0: the lines
// alone.  *text_total = the bytes of text that went to the sink, *sum as documented above.  On an error the sink is the caller's to undo.
static int mtx_text_engine(vtx_ctx* c, const char* fn, bool real, bool gz, int which, const char* head, uint32_t hl, MtxSink& sink,
                           uint64_t* text_total, double* sum) {
    hipStream_t s = c->stream;
    const uint64_t nnz = c->nnz;
    const uint32_t* d_row = c->d_o_row.as<uint32_t>();
    const uint32_t* d_col = c->d_o_col.as<uint32_t>();
    const double* d_val = which ? c->d_o_refval.as<double>() : c->d_o_val.as<double>();
    uint32_t kSlab = 48u << 20;                           // lines per pass: <= 33 bytes each (real: <= 54), 32-bit text offsets
    static_assert((uint64_t)(48u << 20) * VTXG_MTX_LINE_MAX < (1ull << 32), "a pass's text has 32-bit offsets");
    if (VTX_DEV_ENV("VTX_MTX_SLAB")) kSlab = std::min(kSlab, (uint32_t)std::max(1, atoi(VTX_DEV_ENV("VTX_MTX_SLAB"))));   // test hook: several passes
    BamCounters cnt;                                      // (here: the sum in the first counter's eight bytes, the flag in the first of the four words)
    if (int rc = reserve_bam_counters(c, &cnt)) return rc;
    double* d_sum = (double*)cnt.counters;
    uint32_t* d_flag = cnt.err;
    HIP_TRY(c, hipMemsetAsync(cnt.counters, 0, BamCounters::kBytes, s));
    *text_total = 0;
    bool first = true;
    for (uint64_t base = 0; base < nnz || (hl && first); base += kSlab) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(kSlab, nnz - base);
        const uint32_t pre = first ? hl : 0u;                      // gz: the header lines lie in front of the first pass's text — every byte of the file goes through the encoder
        first = false;
        if (hipError_t e = c->d_bam_nhit.reserve((size_t)n * sizeof(uint32_t) + 16)) return fail(c, VTX_E_NOMEM, "%s: %s", fn, hipGetErrorString(e));
        if (hipError_t e = c->d_bam_hscan.reserve((size_t)n * sizeof(uint32_t) + 16)) return fail(c, VTX_E_NOMEM, "%s: %s", fn, hipGetErrorString(e));
        if (hipError_t e = c->d_scan_tmp.reserve(vtxk_scan_temp_bytes(n))) return fail(c, VTX_E_NOMEM, "%s: %s", fn, hipGetErrorString(e));
        uint32_t* d_len = c->d_bam_nhit.as<uint32_t>();
        uint32_t* d_end = c->d_bam_hscan.as<uint32_t>();
        hipError_t e = vtxg_mtx_len(d_row + base, d_col + base, d_val + base, n, d_len, d_sum, d_flag, real ? 1 : 0, s);
        if (e == hipSuccess) e = vtxk_inclusive_scan_u32(d_len, d_end, n, c->d_scan_tmp.p, vtxk_scan_temp_bytes(n), s);
        uint32_t total = 0, flag = 0;
        if (e == hipSuccess && n) e = hipMemcpyAsync(&total, d_end + (n - 1), sizeof total, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(c, VTX_E_HIP, "%s: %s", fn, hipGetErrorString(e));
        const char* host_fn = sink.fd < 0 ? "vtxh_mtx_part" : gz ? "vtxh_write_mtx_gz" : "vtxh_write_mtx";
        if (flag)
            return real ? fail(c, VTX_E_UNSUPPORTED, "%s: a value outside the device formatter's domain (infinite, subnormal, |v| >= 2^53 or 0 < |v| < 2^-40): format on the host (vtx_fetch_coo + %s)", fn, host_fn)
                        : fail(c, VTX_E_UNSUPPORTED, "%s: a value that is not a non-negative integer (alt_frac): format on the host (vtx_fetch_coo + %s)", fn, host_fn);
        if ((e = c->d_bam_data.reserve((size_t)pre + total + 64)) != hipSuccess) return fail(c, VTX_E_NOMEM, "%s: %s", fn, hipGetErrorString(e));
        if (pre) e = hipMemcpyAsync(c->d_bam_data.p, head, pre, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = vtxg_mtx_text(d_row + base, d_col + base, d_val + base, n, d_end, c->d_bam_data.as<uint8_t>() + pre, real ? 1 : 0, s);
        *text_total += (uint64_t)pre + total;
        if (!gz) {
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return fail(c, VTX_E_HIP, "%s: %s", fn, hipGetErrorString(e));
            if (int rc = mtx_sink_put(c, fn, sink, c->d_bam_data.p, total)) return rc;
            continue;
        }
        const uint64_t t_bytes = (uint64_t)pre + total;             // > 0: a pass has the header lines or at least one line
        const uint32_t n_chunks = (uint32_t)((t_bytes + vtxd::CHUNK - 1) / vtxd::CHUNK);
        // d_bam_comp is where vtx_prefetch_file's thread copies a BAM: like every other user of it, wait for that thread and drop the
        // prefetch before the encoder's slots take the buffer (a later vtx_submit_bam uploads its bytes again)
        prefetch_settle(c, Prefetch::Drop);
        DevBuf &slots = c->d_bam_comp, &packed = c->d_bam_rec, &sizes = c->d_bam_rsz, &ends = c->d_bam_rscan, &tok = c->d_bam_info;
        if (e == hipSuccess) e = slots.reserve((size_t)n_chunks * vtxd::SLOT);
        if (e == hipSuccess) e = packed.reserve((size_t)n_chunks * vtxd::SLOT);
        if (e == hipSuccess) e = sizes.reserve((size_t)n_chunks * sizeof(uint32_t));
        if (e == hipSuccess) e = ends.reserve((size_t)n_chunks * sizeof(uint32_t));
        if (e == hipSuccess) e = tok.reserve((size_t)vtxg_deflate_grid(n_chunks) * vtxd::CHUNK * sizeof(uint32_t));
        if (e == hipSuccess) e = c->d_scan_tmp.reserve(vtxk_scan_temp_bytes(std::max(n, n_chunks)));
        if (e != hipSuccess) return fail(c, VTX_E_NOMEM, "%s: %s", fn, hipGetErrorString(e));
        e = vtxg_mtx_deflate(c->d_bam_data.as<uint8_t>(), t_bytes, n_chunks, slots.as<uint8_t>(), sizes.as<uint32_t>(), tok.as<uint32_t>(), s);
        if (e == hipSuccess) e = vtxk_inclusive_scan_u32(sizes.as<uint32_t>(), ends.as<uint32_t>(), n_chunks, c->d_scan_tmp.p, vtxk_scan_temp_bytes(n_chunks), s);
        if (e == hipSuccess) e = vtxg_mtx_gz_compact(slots.as<uint8_t>(), sizes.as<uint32_t>(), ends.as<uint32_t>(), n_chunks, packed.as<uint8_t>(), s);
        uint32_t gz_bytes = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&gz_bytes, ends.as<uint32_t>() + (n_chunks - 1), sizeof gz_bytes, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(c, VTX_E_HIP, "%s: %s", fn, hipGetErrorString(e));
        if (gz_bytes > (uint64_t)n_chunks * vtxd::SLOT) return fail(c, VTX_E_HIP, "%s: the encoder's sizes do not fit its slots", fn);
        if (int rc = mtx_sink_put(c, fn, sink, packed.p, gz_bytes)) return rc;
    }
    if (sum) {
        *sum = 0.0;
        if (nnz)
            if (hipError_t e = hipMemcpy(sum, d_sum, sizeof(double), hipMemcpyDeviceToHost)) return fail(c, VTX_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    }
    return VTX_OK;
}

static int write_mtx_text(vtx_ctx* c, const char* fn, bool real, bool gz, const char* path, uint32_t n_rows, uint32_t n_cols, int which, double* sum,
                          uint64_t* text_bytes) {
    if (!c) return VTX_E_INVAL;
    if (!path || (which != 0 && which != 1)) return fail(c, VTX_E_INVAL, "%s: bad argument", fn);
    if (!c->ran) return fail(c, VTX_E_STATE, "%s: no completed vtx_run", fn);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    char head[160];
    const int hl = vtxj::header(head, sizeof head, n_rows, n_cols, c->nnz);
    MtxSink sink;
    sink.fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (sink.fd < 0) return fail(c, VTX_E_INVAL, "cannot open %s for writing", path);
    auto bail = [&](int rc) { close(sink.fd); unlink(path); return rc; };
    if (!gz) {                                            // plain: the header lines straight into the file, the passes behind them
        if (pwrite(sink.fd, head, (size_t)hl, 0) != hl) return bail(fail(c, VTX_E_INVAL, "error writing %s", path));
        sink.file_off = (uint64_t)hl;
    }
    uint64_t text_total = 0;
    if (int rc = mtx_text_engine(c, fn, real, gz, which, head, gz ? (uint32_t)hl : 0u, sink, &text_total, sum)) return bail(rc);
    if (gz && pwrite(sink.fd, vtxd::EOF_BLOCK, sizeof vtxd::EOF_BLOCK, (off_t)sink.file_off) != (ssize_t)sizeof vtxd::EOF_BLOCK)
        return bail(fail(c, VTX_E_INVAL, "error writing %s", path));
    if (text_bytes) *text_bytes = text_total + (gz ? 0u : (uint64_t)hl);
    if (close(sink.fd) != 0) { unlink(path); return fail(c, VTX_E_INVAL, "error writing %s", path); }
    return VTX_OK;
}

int vtx_write_mtx(vtx_ctx* c, const char* path, uint32_t n_rows, uint32_t n_cols, int which, double* sum) {
    return write_mtx_text(c, "vtx_write_mtx", false, false, path, n_rows, n_cols, which, sum, nullptr);
}

int vtx_write_mtx_f64(vtx_ctx* c, const char* path, uint32_t n_rows, uint32_t n_cols, int which, double* sum) {
    return write_mtx_text(c, "vtx_write_mtx_f64", true, false, path, n_rows, n_cols, which, sum, nullptr);
}

int vtx_write_mtx_gz(vtx_ctx* c, const char* path, uint32_t n_rows, uint32_t n_cols, int which, int real, double* sum, uint64_t* text_bytes) {
    return write_mtx_text(c, "vtx_write_mtx_gz", real != 0, true, path, n_rows, n_cols, which, sum, text_bytes);
}

// ---- the matrix in parts (include/vtx.h): one part per vtx_run, joined behind a header at the end; no device state between the runs ----
int vtx_mtx_part(vtx_ctx* c, int which, int real, int gz, struct vtx_mtx_part* out) {
    if (!c) return VTX_E_INVAL;
    if (out) memset(out, 0, sizeof *out);                 // before any return: vtx_mtx_part_free on it is always safe
    if (!out || (which != 0 && which != 1)) return fail(c, VTX_E_INVAL, "vtx_mtx_part: bad argument");
    if (!c->ran) return fail(c, VTX_E_STATE, "vtx_mtx_part: no completed vtx_run");
    if (const char* k = VTX_DEV_ENV("VTX_MTX_PART_DECLINE")) {     // test hook: the k-th call of the process declines, as a value outside the formatter's domain would
        static std::atomic<int> calls{0};
        if (++calls == atoi(k)) return fail(c, VTX_E_UNSUPPORTED, "vtx_mtx_part: declined by the developer hook: format on the host (vtx_fetch_coo + vtxh_mtx_part)");
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    // the part comes back through download(): the copy workers' pinned buffers and streams, which a vtx_prefetch_file in flight is using
    // for its upload — wait for it (plain parts too; a gz part drops the prefetched bytes as well, in the engine)
    prefetch_settle(c, Prefetch::Keep);
    MtxSink sink;
    uint64_t text_total = 0;
    double sum = 0.0;
    if (int rc = mtx_text_engine(c, "vtx_mtx_part", real != 0, gz != 0, which, nullptr, 0, sink, &text_total, &sum)) { free(sink.buf); return rc; }
    out->bytes = sink.buf; out->n_bytes = sink.len; out->text_bytes = text_total; out->nnz = c->nnz; out->sum = sum; out->gz = gz ? 1u : 0u;
    return VTX_OK;
}

void vtx_mtx_part_free(struct vtx_mtx_part* part) {
    if (!part) return;
    free(part->bytes);
    memset(part, 0, sizeof *part);
}

int vtx_mtx_join(const char* path, uint32_t n_rows, uint32_t n_cols, int gz, const struct vtx_mtx_part* parts, uint32_t n_parts, uint64_t* text_bytes) {
    char why[512];
    const int rc = vtxj::join(path, n_rows, n_cols, gz, parts, n_parts, text_bytes, why, sizeof why);      // host code only (vtx_mtx_join.h)
    return rc ? fail(nullptr, rc, "%s", why) : VTX_OK;
}

int vtx_device_coo(vtx_ctx* c, vtx_coo* out) {
    if (!c) return VTX_E_INVAL;
    if (!out) return fail(c, VTX_E_INVAL, "vtx_device_coo: null output");
    if (!c->ran) return fail(c, VTX_E_STATE, "vtx_device_coo: no completed vtx_run");
    out->row = c->d_o_row.as<uint32_t>(); out->col = c->d_o_col.as<uint32_t>(); out->alt = c->d_o_alt.as<uint32_t>();
    out->ref = c->d_o_ref.as<uint32_t>(); out->unk = c->d_o_unk.as<uint32_t>(); out->value = c->d_o_val.as<double>();
    out->ref_value = c->d_o_refval.as<double>();
    out->nnz = c->nnz;
    return VTX_OK;
}

// ---- the matrices as CSR on the device (include/vtx.h, vtx_csr.hip) ----
static const char* csr_bad_reason(uint32_t flag) {
    if (flag & vtxr::BAD_FIRST) return "indptr[0] != 0";
    if (flag & vtxr::BAD_ORDER) return "indptr decreases";
    if (flag & vtxr::BAD_LAST) return "indptr[n_major] != nnz";
    if (flag & vtxr::BAD_INDEX) return "an index >= n_minor";
    return "a triplet's row outside [row_begin, row_end)";
}

static int csr_events(vtx_ctx* c) {
    for (auto& ev : c->csr.ev) if (!ev) HIP_TRY(c, hipEventCreate(&ev));
    return VTX_OK;
}
static int csr_times(vtx_ctx* c, bool checked, bool sorted, bool placed, bool offsets = true) {        // after the stream is synchronised
    const int pair[4][2] = {{EV_CSR_CHECK0, EV_CSR_CHECK1}, {EV_CSR_SORT0, EV_CSR_SORT1}, {EV_CSR_SORT1, EV_CSR_OFFSETS1}, {EV_CSR_OFFSETS1, EV_CSR_PLACE1}};
    const bool on[4] = {checked, sorted, offsets, placed};
    for (int i = 0; i < 4; ++i) {
        c->csr.ms[i] = 0.f;
        if (on[i]) HIP_TRY(c, hipEventElapsedTime(&c->csr.ms[i], c->csr.ev[pair[i][0]], c->csr.ev[pair[i][1]]));
    }
    return VTX_OK;
}

int vtx_last_csr_ms(vtx_ctx* c, float* ms, uint32_t n) {
    if (!c) return VTX_E_INVAL;
    if (!ms) return fail(c, VTX_E_INVAL, "vtx_last_csr_ms: null output");
    for (uint32_t i = 0; i < n && i < 4; ++i) ms[i] = c->csr.ms[i];
    return VTX_OK;
}

// The preamble of every call that takes arrays from outside: they are read, and judged, before a single byte is written through them.
// The verdict words are set on the stream, `launch(s)` issues the call's check kernels between the events of the check phase, and the
// words come back to `verdict` with the stream synchronised.  Every call sets all the words: none survives into the next call.
static const uint64_t kCsrVerdictInit[V_COUNT] = {0ull, ~0ull, ~0ull, ~0ull};      // (static: the copy is asynchronous)
extern "C++" {      // (templates over the callables: this part of the file has C linkage)
template <class Launch> static int csr_judged(vtx_ctx* c, uint64_t verdict[V_COUNT], Launch launch) {
    hipStream_t s = c->stream;
    if (int rc = csr_events(c)) return rc;
    HIP_TRY(c, c->csr.d_verdict.reserve(sizeof kCsrVerdictInit));
    HIP_TRY(c, hipMemcpyAsync(c->csr.d_verdict.p, kCsrVerdictInit, sizeof kCsrVerdictInit, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_CHECK0], s));
    if (int rc = launch(s)) return rc;
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_CHECK1], s));
    HIP_TRY(c, hipMemcpyAsync(verdict, c->csr.d_verdict.p, sizeof kCsrVerdictInit, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return VTX_OK;
}

// ... of a caller's CSR: vtxr_check and the call's own checks (`extra(s)`; each reads its own array only, whatever the others hold).  A
// bad CSR is refused here, first; the caller judges the words of its own checks in `verdict` next.
template <class Extra> static int csr_checked(vtx_ctx* c, const char* who, uint32_t n_major, uint32_t n_minor, uint64_t nnz, const uint64_t* d_indptr,
                                              const uint32_t* d_indices, uint64_t verdict[V_COUNT], Extra extra) {
    if (int rc = csr_judged(c, verdict, [&](hipStream_t s) -> int {
            HIP_TRY(c, vtxr_check(d_indptr, n_major, nnz, d_indices, n_minor, c->csr.verdict<uint32_t>(V_CSR_BAD), s));
            return extra(s);
        })) return rc;
    if (const uint32_t flag = (uint32_t)verdict[V_CSR_BAD]) return fail(c, VTX_E_INVAL, "%s: %s", who, csr_bad_reason(flag));
    return VTX_OK;
}
}
static int csr_checked(vtx_ctx* c, const char* who, uint32_t n_major, uint32_t n_minor, uint64_t nnz, const uint64_t* d_indptr,
                       const uint32_t* d_indices) {
    uint64_t verdict[V_COUNT];
    return csr_checked(c, who, n_major, n_minor, nnz, d_indptr, d_indices, verdict, [](hipStream_t) { return (int)VTX_OK; });
}

// what the calls refuse on the host, before the device is touched
static int csr_positions_fit(vtx_ctx* c, const char* who, uint64_t nnz) {
    if (nnz >= (1ull << 32)) return fail(c, VTX_E_UNSUPPORTED, "%s: %llu entries: positions are 32-bit", who, (unsigned long long)nnz);
    return VTX_OK;
}
// the arrays that move with the entries; need_in / need_out: the input / output side has elements, so that its arrays must exist
static int csr_payload_args(vtx_ctx* c, const char* who, const void* const* d_payload_in, void* const* d_payload_out, const uint32_t* payload_elem_bytes,
                            uint32_t n_payload, bool need_in, bool need_out) {
    if (n_payload && (!d_payload_in || !d_payload_out || !payload_elem_bytes)) return fail(c, VTX_E_INVAL, "%s: null payload list", who);
    for (uint32_t a = 0; a < n_payload; ++a) {
        if (payload_elem_bytes[a] != 4 && payload_elem_bytes[a] != 8)
            return fail(c, VTX_E_INVAL, "%s: payload %u has elements of %u bytes (4 or 8)", who, a, payload_elem_bytes[a]);
        if ((need_in && !d_payload_in[a]) || (need_out && !d_payload_out[a])) return fail(c, VTX_E_INVAL, "%s: payload %u is null", who, a);
    }
    return VTX_OK;
}

int vtx_device_csr(vtx_ctx* c, uint32_t row_begin, uint32_t row_end, vtx_csr* out) {
    if (!c) return VTX_E_INVAL;
    if (!out) return fail(c, VTX_E_INVAL, "vtx_device_csr: null output");
    memset(out, 0, sizeof *out);
    if (!c->ran) return fail(c, VTX_E_STATE, "vtx_device_csr: no completed vtx_run");
    if (row_begin > row_end) return fail(c, VTX_E_INVAL, "vtx_device_csr: row_begin %u > row_end %u", row_begin, row_end);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    const uint64_t nnz = c->nnz;
    const uint32_t* d_row = c->d_o_row.as<uint32_t>();
    if (int rc = csr_events(c)) return rc;
    if (nnz) {
        uint64_t verdict[V_COUNT];
        if (int rc = csr_judged(c, verdict, [&](hipStream_t st) -> int {
                HIP_TRY(c, vtxr_window_check(d_row, nnz, row_begin, row_end, c->csr.verdict<uint32_t>(V_CSR_BAD), st));
                return VTX_OK;
            })) return rc;
        if (const uint32_t flag = (uint32_t)verdict[V_CSR_BAD]) return fail(c, VTX_E_INVAL, "vtx_device_csr: %s [%u, %u)", csr_bad_reason(flag), row_begin, row_end);
    }
    HIP_TRY(c, c->csr.d_indptr.reserve(((size_t)(row_end - row_begin) + 1) * sizeof(uint64_t)));
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_SORT1], s));
    HIP_TRY(c, vtxr_offsets(d_row, nnz, row_begin, row_end, c->csr.d_indptr.as<uint64_t>(), s));
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_OFFSETS1], s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (int rc = csr_times(c, nnz != 0, false, false)) return rc;
    out->indptr = c->csr.d_indptr.as<uint64_t>();
    out->indices = c->d_o_col.as<uint32_t>();
    out->alt = c->d_o_alt.as<uint32_t>(); out->ref = c->d_o_ref.as<uint32_t>(); out->unk = c->d_o_unk.as<uint32_t>();
    out->value = c->d_o_val.as<double>(); out->ref_value = c->d_o_refval.as<double>();
    out->nnz = nnz;
    out->row_begin = row_begin; out->row_end = row_end; out->n_cols = c->cfg.n_barcodes;
    return VTX_OK;
}

int vtx_csr_transpose(vtx_ctx* c, uint32_t n_major, uint32_t n_minor, uint64_t nnz, const uint64_t* d_indptr, const uint32_t* d_indices,
                      uint64_t* d_indptr_t, uint32_t* d_indices_t, uint32_t* d_perm, const void* const* d_payload_in, void* const* d_payload_out,
                      const uint32_t* payload_elem_bytes, uint32_t n_payload) {
    const char* who = "vtx_csr_transpose";
    if (!c) return VTX_E_INVAL;
    if (int rc = csr_positions_fit(c, who, nnz)) return rc;
    if (!d_indptr || !d_indptr_t || (nnz && (!d_indices || !d_indices_t))) return fail(c, VTX_E_INVAL, "%s: null array", who);
    if (int rc = csr_payload_args(c, who, d_payload_in, d_payload_out, payload_elem_bytes, n_payload, nnz != 0, nnz != 0)) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    if (int rc = csr_checked(c, who, n_major, n_minor, nnz, d_indptr, d_indices)) return rc;
    uint32_t* perm = d_perm;
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_SORT0], s));
    if (nnz) {
        const int end_bit = (int)bits_for(n_minor - 1);
        const size_t tmp = vtxr_sort_temp_bytes(nnz, end_bit);
        HIP_TRY(c, c->csr.d_keys.reserve((size_t)nnz * sizeof(uint32_t)));
        HIP_TRY(c, c->csr.d_iota.reserve((size_t)nnz * sizeof(uint32_t)));
        HIP_TRY(c, c->csr.d_tmp.reserve(tmp));
        if (!perm) { HIP_TRY(c, c->csr.d_perm.reserve((size_t)nnz * sizeof(uint32_t))); perm = c->csr.d_perm.as<uint32_t>(); }
        HIP_TRY(c, vtxr_sort_positions(d_indices, c->csr.d_keys.as<uint32_t>(), c->csr.d_iota.as<uint32_t>(), perm, nnz, end_bit, c->csr.d_tmp.p, tmp, s));
    }
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_SORT1], s));
    HIP_TRY(c, vtxr_offsets(c->csr.d_keys.as<uint32_t>(), nnz, 0, n_minor, d_indptr_t, s));
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_OFFSETS1], s));
    HIP_TRY(c, vtxr_place(d_indptr, n_major, perm, nnz, d_indices_t, d_payload_in, d_payload_out, payload_elem_bytes, n_payload, s));
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_PLACE1], s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (int rc = csr_times(c, true, true, true)) return rc;
    return VTX_OK;
}

// ---- summaries and selections of a caller's CSR (include/vtx.h, vtx_csr_ops.hip) ----
int vtx_csr_row_stats(vtx_ctx* c, uint32_t n_major, uint32_t n_minor, uint64_t nnz, const uint64_t* d_indptr, const uint32_t* d_indices,
                      const uint32_t* d_alt, const uint32_t* d_ref, const uint32_t* d_unk, const vtx_csr_stats* out) {
    if (!c) return VTX_E_INVAL;
    if (int rc = csr_positions_fit(c, "vtx_csr_row_stats", nnz)) return rc;
    if (!out || !d_indptr || (nnz && (!d_indices || !d_alt || !d_ref || !d_unk))) return fail(c, VTX_E_INVAL, "vtx_csr_row_stats: null array");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    if (int rc = csr_checked(c, "vtx_csr_row_stats", n_major, n_minor, nnz, d_indptr, d_indices)) return rc;
    uint32_t G = vtxr::group_lanes(nnz, n_major);
    if (const char* e = VTX_DEV_ENV("VTX_CSR_STATS_G")) G = (uint32_t)atoi(e);    // developer library: the sweep behind the rule (tools/csr_profile.py)
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_OFFSETS1], s));
    HIP_TRY(c, vtxr_row_stats(d_indptr, n_major, d_alt, d_ref, d_unk, out, G, s));
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_PLACE1], s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (int rc = csr_times(c, true, false, true, false)) return rc;      // no sort, no offsets here
    return VTX_OK;
}

// The scans of a selection; the three sizes come back to the host.  Writes into the context's work space only.
static int csr_select_scans(vtx_ctx* c, const char* who, uint32_t n_major, uint32_t n_minor, uint64_t nnz, const uint64_t* d_indptr,
                            const uint32_t* d_indices, const uint8_t* d_keep_major, const uint8_t* d_keep_minor, uint32_t sizes[3]) {
    hipStream_t s = c->stream;
    if (int rc = csr_checked(c, who, n_major, n_minor, nnz, d_indptr, d_indices)) return rc;
    const size_t tmp = std::max(vtxr_scan_temp_bytes(nnz + 1), std::max(vtxr_scan_temp_bytes((uint64_t)n_major + 1), vtxr_scan_temp_bytes((uint64_t)n_minor + 1)));
    HIP_TRY(c, c->csr.d_sel_pos.reserve(((size_t)nnz + 1) * sizeof(uint32_t)));
    HIP_TRY(c, c->csr.d_sel_major.reserve(((size_t)n_major + 1) * sizeof(uint32_t)));
    HIP_TRY(c, c->csr.d_sel_minor.reserve(((size_t)n_minor + 1) * sizeof(uint32_t)));
    HIP_TRY(c, c->csr.d_sel_tmp.reserve(std::max<size_t>(tmp, 1)));      // never a null work space: with one the scan only reports its size
    uint32_t *pos = c->csr.d_sel_pos.as<uint32_t>(), *major_map = c->csr.d_sel_major.as<uint32_t>(), *minor_map = c->csr.d_sel_minor.as<uint32_t>();
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_SORT0], s));
    HIP_TRY(c, vtxr_mask_map(d_keep_minor, n_minor, minor_map, c->csr.d_sel_tmp.p, tmp, s));
    HIP_TRY(c, vtxr_keep_positions(d_indptr, n_major, d_indices, nnz, d_keep_major, d_keep_minor, pos, c->csr.d_sel_tmp.p, tmp, s));
    HIP_TRY(c, vtxr_mask_map(d_keep_major, n_major, major_map, c->csr.d_sel_tmp.p, tmp, s));
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_SORT1], s));
    HIP_TRY(c, hipMemcpyAsync(&sizes[0], major_map + n_major, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&sizes[1], minor_map + n_minor, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&sizes[2], pos + nnz, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return VTX_OK;
}

int vtx_csr_select_plan(vtx_ctx* c, uint32_t n_major, uint32_t n_minor, uint64_t nnz, const uint64_t* d_indptr, const uint32_t* d_indices,
                        const uint8_t* d_keep_major, const uint8_t* d_keep_minor, uint32_t* n_major_out, uint32_t* n_minor_out,
                        uint64_t* nnz_out) {
    if (!c) return VTX_E_INVAL;
    if (int rc = csr_positions_fit(c, "vtx_csr_select_plan", nnz)) return rc;
    if (!d_indptr || (nnz && !d_indices) || !n_major_out || !n_minor_out || !nnz_out) return fail(c, VTX_E_INVAL, "vtx_csr_select_plan: null array");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    uint32_t sizes[3] = {0, 0, 0};
    if (int rc = csr_select_scans(c, "vtx_csr_select_plan", n_major, n_minor, nnz, d_indptr, d_indices, d_keep_major, d_keep_minor, sizes)) return rc;
    if (int rc = csr_times(c, true, true, false, false)) return rc;
    *n_major_out = sizes[0]; *n_minor_out = sizes[1]; *nnz_out = sizes[2];
    return VTX_OK;
}

int vtx_csr_select(vtx_ctx* c, uint32_t n_major, uint32_t n_minor, uint64_t nnz, const uint64_t* d_indptr, const uint32_t* d_indices,
                   const uint8_t* d_keep_major, const uint8_t* d_keep_minor, uint32_t n_major_out, uint32_t n_minor_out, uint64_t nnz_out,
                   uint64_t* d_indptr_out, uint32_t* d_indices_out, uint32_t* d_major_ids, uint32_t* d_minor_ids,
                   const void* const* d_payload_in, void* const* d_payload_out, const uint32_t* payload_elem_bytes, uint32_t n_payload) {
    if (!c) return VTX_E_INVAL;
    if (int rc = csr_positions_fit(c, "vtx_csr_select", nnz)) return rc;
    if (!d_indptr || !d_indptr_out || (nnz && !d_indices) || (nnz_out && !d_indices_out)) return fail(c, VTX_E_INVAL, "vtx_csr_select: null array");
    if (int rc = csr_payload_args(c, "vtx_csr_select", d_payload_in, d_payload_out, payload_elem_bytes, n_payload, nnz != 0, nnz_out != 0)) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    uint32_t sizes[3] = {0, 0, 0};
    if (int rc = csr_select_scans(c, "vtx_csr_select", n_major, n_minor, nnz, d_indptr, d_indices, d_keep_major, d_keep_minor, sizes)) return rc;
    // stateless: the sizes are this call's own; a caller whose arrays were made for other ones is refused before a byte is written
    if (sizes[0] != n_major_out || sizes[1] != n_minor_out || sizes[2] != nnz_out)
        return fail(c, VTX_E_INVAL, "vtx_csr_select: the selection has %u rows, %u columns and %u entries, the caller said %u, %u and %llu (vtx_csr_select_plan)",
                    sizes[0], sizes[1], sizes[2], n_major_out, n_minor_out, (unsigned long long)nnz_out);
    const uint32_t *pos = c->csr.d_sel_pos.as<uint32_t>(), *major_map = c->csr.d_sel_major.as<uint32_t>(), *minor_map = c->csr.d_sel_minor.as<uint32_t>();
    float scan_ms = 0.f;                                      // the stream was idle while the sizes came back: the offsets' time starts anew
    HIP_TRY(c, hipEventElapsedTime(&scan_ms, c->csr.ev[EV_CSR_SORT0], c->csr.ev[EV_CSR_SORT1]));
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_SORT1], s));
    HIP_TRY(c, vtxr_select_offsets(d_indptr, n_major, d_keep_major, major_map, pos, d_indptr_out, s));
    HIP_TRY(c, vtxr_select_ids(d_keep_major, n_major, major_map, d_major_ids, s));
    HIP_TRY(c, vtxr_select_ids(d_keep_minor, n_minor, minor_map, d_minor_ids, s));
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_OFFSETS1], s));
    if (nnz_out) HIP_TRY(c, vtxr_select_place(d_indices, nnz, pos, minor_map, d_indices_out, d_payload_in, d_payload_out, payload_elem_bytes, n_payload, s));
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_PLACE1], s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (int rc = csr_times(c, true, false, true)) return rc;
    c->csr.ms[1] = scan_ms;
    return VTX_OK;
}

// ---- pseudobulk: a caller's CSR summed per group of columns (include/vtx.h, vtx_csr_group.hip) ----
uint32_t vtx_csr_group_window(void) { return vtxr::GROUP_WINDOW; }
uint32_t vtx_csr_group_max(void) { return vtxr::GROUP_MAX; }
static_assert(VTX_GROUP_NONE == vtxr::GROUP_NONE, "the header's and the kernels' label of no group");

// what both calls refuse on the host, before the device is touched
static int csr_group_args(vtx_ctx* c, const char* who, uint32_t n_minor, uint64_t nnz, const uint64_t* d_indptr, const uint32_t* d_indices,
                          const uint32_t* d_group, uint32_t n_groups) {
    if (int rc = csr_positions_fit(c, who, nnz)) return rc;
    if (!n_groups) return fail(c, VTX_E_INVAL, "%s: no groups", who);
    if (n_groups > vtxr::GROUP_MAX)
        return fail(c, VTX_E_UNSUPPORTED, "%s: %u groups: at most %u (%u windows of %u)", who, n_groups, vtxr::GROUP_MAX, vtxr::GROUP_MAX_WINDOWS, vtxr::GROUP_WINDOW);
    if (!d_indptr || (nnz && !d_indices) || (n_minor && !d_group)) return fail(c, VTX_E_INVAL, "%s: null array", who);
    return VTX_OK;
}

// The checks of the CSR and of the labels, the count and its scan; nnz_out comes back to the host.  Writes into the context's work space only.
static int csr_group_counts(vtx_ctx* c, const char* who, uint32_t n_minor, uint64_t nnz, const vtx_group_in& in, uint32_t* nnz_out) {
    hipStream_t s = c->stream;
    uint64_t verdict[V_COUNT];
    if (int rc = csr_checked(c, who, in.n_major, n_minor, nnz, in.indptr, in.indices, verdict, [&](hipStream_t st) -> int {
            HIP_TRY(c, vtxr_group_check(in.group, n_minor, in.n_groups, c->csr.verdict<uint32_t>(V_LABEL), st));      // reads group[0 .. n_minor) only, whatever the CSR is
            return VTX_OK;
        })) return rc;
    if (const uint32_t first_bad = (uint32_t)verdict[V_LABEL]; first_bad != 0xFFFFFFFFu)
        return fail(c, VTX_E_INVAL, "%s: the label of column %u is neither below n_groups = %u nor VTX_GROUP_NONE", who, first_bad, in.n_groups);
    const size_t tmp = vtxr_scan_temp_bytes((uint64_t)in.n_major + 1);
    HIP_TRY(c, c->csr.d_grp_pos.reserve(((size_t)in.n_major + 1) * sizeof(uint32_t)));
    HIP_TRY(c, c->csr.d_grp_tmp.reserve(std::max<size_t>(tmp, 1)));      // never a null work space: with one the scan only reports its size
    uint32_t* pos = c->csr.d_grp_pos.as<uint32_t>();
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_SORT0], s));
    HIP_TRY(c, vtxr_group_count(in, pos, c->csr.d_grp_tmp.p, tmp, s));
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_SORT1], s));
    HIP_TRY(c, hipMemcpyAsync(nnz_out, pos + in.n_major, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return VTX_OK;
}

int vtx_csr_group_plan(vtx_ctx* c, uint32_t n_major, uint32_t n_minor, uint64_t nnz, const uint64_t* d_indptr, const uint32_t* d_indices,
                       const uint32_t* d_group, uint32_t n_groups, uint64_t* nnz_out) {
    if (!c) return VTX_E_INVAL;
    if (int rc = csr_group_args(c, "vtx_csr_group_plan", n_minor, nnz, d_indptr, d_indices, d_group, n_groups)) return rc;
    if (!nnz_out) return fail(c, VTX_E_INVAL, "vtx_csr_group_plan: null output");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const vtx_group_in in{d_indptr, n_major, d_indices, nullptr, nullptr, nullptr, d_group, n_groups};
    uint32_t n = 0;
    if (int rc = csr_group_counts(c, "vtx_csr_group_plan", n_minor, nnz, in, &n)) return rc;
    if (int rc = csr_times(c, true, true, false, false)) return rc;
    *nnz_out = n;
    return VTX_OK;
}

int vtx_csr_group_sum(vtx_ctx* c, uint32_t n_major, uint32_t n_minor, uint64_t nnz, const uint64_t* d_indptr, const uint32_t* d_indices,
                      const uint32_t* d_alt, const uint32_t* d_ref, const uint32_t* d_unk, const uint32_t* d_group, uint32_t n_groups,
                      uint64_t nnz_out, uint64_t* d_indptr_out, uint32_t* d_indices_out, const vtx_csr_stats* out) {
    if (!c) return VTX_E_INVAL;
    if (int rc = csr_group_args(c, "vtx_csr_group_sum", n_minor, nnz, d_indptr, d_indices, d_group, n_groups)) return rc;
    if (!out || !d_indptr_out || (nnz && (!d_alt || !d_ref || !d_unk)) || (nnz_out && !d_indices_out)) return fail(c, VTX_E_INVAL, "vtx_csr_group_sum: null array");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    const vtx_group_in in{d_indptr, n_major, d_indices, d_alt, d_ref, d_unk, d_group, n_groups};
    uint32_t n = 0;
    if (int rc = csr_group_counts(c, "vtx_csr_group_sum", n_minor, nnz, in, &n)) return rc;
    // stateless: the size is this call's own; a caller whose arrays were made for another fold is refused before a byte is written
    if (n != nnz_out)
        return fail(c, VTX_E_INVAL, "vtx_csr_group_sum: the result has %u entries, the caller said %llu (vtx_csr_group_plan)", n, (unsigned long long)nnz_out);
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_OFFSETS1], s));
    HIP_TRY(c, vtxr_group_fill(in, c->csr.d_grp_pos.as<uint32_t>(), d_indptr_out, d_indices_out, out, s));
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_PLACE1], s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (int rc = csr_times(c, true, true, true, false)) return rc;      // checks, count + scan, no offsets phase, fill
    return VTX_OK;
}

// ---- donor and doublet tally: a caller's cells x variants CSR against a table of donor genotypes, by donor or by pair of donors
// (include/vtx.h, vtx_csr_geno.hip) ----
uint32_t vtx_csr_geno_max(void) { return vtxr::GENO_MAX; }
uint32_t vtx_csr_geno_pair_max(void) { return vtxr::PAIR_MAX; }
static_assert(VTX_GENO_NONE == vtxr::GENO_NONE, "the header's and the kernels' byte of no call");
static_assert(VTX_GENO_PAIR_CLASSES == vtxr::PAIR_CLASSES, "the header's and the kernels' classes of a pair");
static_assert(sizeof(vtx_geno_tally) == 24 && sizeof(vtx_geno_pair_tally) == 24, "three pointers");

// what both tallies refuse on the host, before the device is touched.  n_pairs: the doublet call's (nullptr: the donor call);
// null_array: one of the arrays the call needs is missing
static int csr_geno_args(vtx_ctx* c, const char* who, uint64_t nnz, uint32_t n_donors, const uint32_t* n_pairs, bool null_array) {
    if (int rc = csr_positions_fit(c, who, nnz)) return rc;
    if (!n_donors) return fail(c, VTX_E_INVAL, "%s: no donors", who);
    if (n_pairs && !*n_pairs) return fail(c, VTX_E_INVAL, "%s: no pairs", who);
    if (n_donors > vtxr::GENO_MAX)
        return fail(c, VTX_E_UNSUPPORTED, "%s: %u donors: at most %u (%u passes of %u)", who, n_donors, vtxr::GENO_MAX, vtxr::GENO_MAX_PASSES, vtxr::GENO_WAVE);
    if (n_pairs && *n_pairs > vtxr::PAIR_MAX)
        return fail(c, VTX_E_UNSUPPORTED, "%s: %u pairs: at most %u (%u passes of %u)", who, *n_pairs, vtxr::PAIR_MAX, vtxr::PAIR_MAX_PASSES, vtxr::GENO_WAVE);
    if (null_array) return fail(c, VTX_E_INVAL, "%s: null array", who);
    return VTX_OK;
}

// the verdict of vtxr_geno_check
static int csr_geno_judged(vtx_ctx* c, const char* who, uint64_t first_bad, uint32_t n_donors) {
    if (first_bad == ~0ull) return VTX_OK;
    return fail(c, VTX_E_INVAL, "%s: the genotype of variant %llu, donor %llu is neither 0, 1, 2 nor VTX_GENO_NONE", who,
                (unsigned long long)(first_bad / n_donors), (unsigned long long)(first_bad % n_donors));
}

int vtx_csr_geno_tally(vtx_ctx* c, uint32_t n_major, uint32_t n_minor, uint64_t nnz, const uint64_t* d_indptr, const uint32_t* d_indices,
                       const uint32_t* d_alt, const uint32_t* d_ref, const uint8_t* d_geno, uint32_t n_donors, const vtx_geno_tally* out) {
    const char* who = "vtx_csr_geno_tally";
    if (!c) return VTX_E_INVAL;
    if (int rc = csr_geno_args(c, who, nnz, n_donors, nullptr, !out || !d_indptr || (nnz && (!d_indices || !d_alt || !d_ref)) || (n_minor && !d_geno))) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    uint64_t verdict[V_COUNT];
    if (int rc = csr_checked(c, who, n_major, n_minor, nnz, d_indptr, d_indices, verdict, [&](hipStream_t st) -> int {
            HIP_TRY(c, vtxr_geno_check(d_geno, (uint64_t)n_minor * n_donors, c->csr.verdict<uint64_t>(V_GENO), st));
            return VTX_OK;
        })) return rc;
    if (int rc = csr_geno_judged(c, who, verdict[V_GENO], n_donors)) return rc;
    const vtx_geno_in in{d_indptr, n_major, d_indices, d_alt, d_ref, d_geno, n_donors};
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_OFFSETS1], s));
    HIP_TRY(c, vtxr_geno_tally(in, out, s));
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_PLACE1], s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (int rc = csr_times(c, true, false, true, false)) return rc;      // the two checks and the tally: no sort, no offsets here
    return VTX_OK;
}

int vtx_csr_geno_pair_tally(vtx_ctx* c, uint32_t n_major, uint32_t n_minor, uint64_t nnz, const uint64_t* d_indptr, const uint32_t* d_indices,
                            const uint32_t* d_alt, const uint32_t* d_ref, const uint8_t* d_geno, uint32_t n_donors, const uint32_t* d_pairs,
                            uint32_t n_pairs, const vtx_geno_pair_tally* out) {
    const char* who = "vtx_csr_geno_pair_tally";
    if (!c) return VTX_E_INVAL;
    if (int rc = csr_geno_args(c, who, nnz, n_donors, &n_pairs,
                               !out || !d_indptr || !d_pairs || (nnz && (!d_indices || !d_alt || !d_ref)) || (n_minor && !d_geno))) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    uint64_t verdict[V_COUNT];
    if (int rc = csr_checked(c, who, n_major, n_minor, nnz, d_indptr, d_indices, verdict, [&](hipStream_t st) -> int {
            HIP_TRY(c, vtxr_geno_check(d_geno, (uint64_t)n_minor * n_donors, c->csr.verdict<uint64_t>(V_GENO), st));
            HIP_TRY(c, vtxr_geno_pair_check(d_pairs, n_pairs, n_donors, c->csr.verdict<uint64_t>(V_PAIR), st));
            return VTX_OK;
        })) return rc;
    if (int rc = csr_geno_judged(c, who, verdict[V_GENO], n_donors)) return rc;
    if (const uint64_t first_pair = verdict[V_PAIR]; first_pair != ~0ull) {      // < n_pairs: the check's lanes are the pairs
        uint32_t ab[2] = {0, 0};
        HIP_TRY(c, hipMemcpyAsync(ab, d_pairs + 2 * first_pair, sizeof(ab), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        return fail(c, VTX_E_INVAL, "%s: pair %llu is (%u, %u): a donor is not below n_donors = %u", who, (unsigned long long)first_pair, ab[0], ab[1], n_donors);
    }
    const vtx_geno_pair_in in{d_indptr, n_major, d_indices, d_alt, d_ref, d_geno, n_donors, d_pairs, n_pairs};
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_OFFSETS1], s));
    HIP_TRY(c, vtxr_geno_pair_tally(in, out, s));
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_PLACE1], s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (int rc = csr_times(c, true, false, true, false)) return rc;      // the three checks and the tally: no sort, no offsets here
    return VTX_OK;
}

// ---- CSR x integer tables: a caller's CSR against one or two tables of int32 weights per (minor, column), summed modulo 2^64
// (include/vtx.h, vtx_csr_dense.hip) ----
uint32_t vtx_csr_dense_max(void) { return vtxr::DENSE_MAX; }

int vtx_csr_dense_sum(vtx_ctx* c, uint32_t n_major, uint32_t n_minor, uint64_t nnz, const uint64_t* d_indptr, const uint32_t* d_indices,
                      const uint32_t* d_alt, const uint32_t* d_ref, const int32_t* d_w_alt, const int32_t* d_w_ref, uint32_t n_cols, int64_t* d_out) {
    const char* who = "vtx_csr_dense_sum";
    if (!c) return VTX_E_INVAL;
    if (int rc = csr_positions_fit(c, who, nnz)) return rc;
    if (!n_cols) return fail(c, VTX_E_INVAL, "%s: no columns", who);
    if (n_cols > vtxr::DENSE_MAX)
        return fail(c, VTX_E_UNSUPPORTED, "%s: %u columns: at most %u (%u passes of %u)", who, n_cols, vtxr::DENSE_MAX, vtxr::DENSE_MAX_PASSES, vtxr::GENO_WAVE);
    if (!d_out || !d_indptr || (nnz && (!d_indices || !d_alt || !d_ref))) return fail(c, VTX_E_INVAL, "%s: null array", who);
    if (n_minor && !d_w_alt && !d_w_ref) return fail(c, VTX_E_INVAL, "%s: null tables: w_alt, w_ref or both", who);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    if (int rc = csr_checked(c, who, n_major, n_minor, nnz, d_indptr, d_indices)) return rc;
    const vtx_dense_in in{d_indptr, n_major, d_indices, d_alt, d_ref, d_w_alt, d_w_ref, n_cols};
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_OFFSETS1], s));
    HIP_TRY(c, vtxr_dense_sum(in, d_out, s));
    HIP_TRY(c, hipEventRecord(c->csr.ev[EV_CSR_PLACE1], s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (int rc = csr_times(c, true, false, true, false)) return rc;      // the check and the sum: no sort, no offsets here
    return VTX_OK;
}

int vtx_comm_id(uint8_t id[VTX_COMM_ID_BYTES]) {
    static_assert(VTX_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");
    if (!id) return fail(nullptr, VTX_E_INVAL, "vtx_comm_id: null argument");
    if (!rccl()) return fail(nullptr, VTX_E_UNSUPPORTED, "vtx_comm_id: librccl.so not found");
    ncclUniqueId u;
    NCCL_TRY(nullptr, rccl()->GetUniqueId(&u));
    memcpy(id, u.internal, VTX_COMM_ID_BYTES);
    return VTX_OK;
}

int vtx_comm_init(vtx_ctx* c, const uint8_t id[VTX_COMM_ID_BYTES], int rank, int world) {
    if (!c) return VTX_E_INVAL;
    if (!id || world < 1 || rank < 0 || rank >= world) return fail(c, VTX_E_INVAL, "vtx_comm_init: bad rank %d / world %d", rank, world);
    if (!rccl()) return fail(c, VTX_E_UNSUPPORTED, "vtx_comm_init: librccl.so not found");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    comm_release(c);
    ncclUniqueId u;
    memcpy(u.internal, id, VTX_COMM_ID_BYTES);
    NCCL_TRY(c, rccl()->CommInitRank(&c->comm, world, u, rank));
    c->comm_rank = rank; c->comm_world = world;
    return VTX_OK;
}

// How many ranks the communicator itself reports (ncclCommCount): what bench.py's line quotes next to the launcher's world size.
int vtx_comm_ranks(vtx_ctx* c, int* ranks) {
    if (!c || !ranks) return VTX_E_INVAL;
    if (!c->comm) return fail(c, VTX_E_STATE, "vtx_comm_ranks: no communicator (vtx_comm_init)");
    if (!rccl() || !rccl()->CommCount) return fail(c, VTX_E_UNSUPPORTED, "vtx_comm_ranks: ncclCommCount not available");
    NCCL_TRY(c, rccl()->CommCount(c->comm, ranks));
    return VTX_OK;
}

// The exchange's plan as a pure function of the counts (no device, no communicator): rank r's block lands at
// offsets[r] of the gathered arrays (rank order = row order), *total triplets in all.  VTX_E_UNSUPPORTED when the gathered
// arrays would not fit 32-bit indices.  Every rank computes the same plan from the same all-gathered counts, so every rank
// takes the same decision.
int vtx_gather_plan(int world, const uint64_t* counts, uint64_t* offsets, uint64_t* total) {
    if (world < 1 || !counts || !offsets || !total) return VTX_E_INVAL;
    uint64_t t = 0;
    for (int r = 0; r < world; ++r) { offsets[r] = t; t += counts[r]; }
    *total = t;
    return t > 0xffffffffull ? VTX_E_UNSUPPORTED : VTX_OK;
}

// One all-gather of (count, status) per rank: a rank that cannot take part in the data exchange (its own vtx_run failed,
// the destination could not reserve its buffers) says so HERE, and every rank leaves with VTX_E_PEER before any
// point-to-point call — a Send whose Recv never comes would block for ever.
static int gather_agree(vtx_ctx* c, uint64_t mine, uint64_t status, std::vector<uint64_t>& cnt, std::vector<uint64_t>& st) {
    const int world = c->comm_world;
    hipStream_t s = c->stream;
    Rccl* R = rccl();
    HIP_TRY(c, c->d_g_cnt.reserve(2 * ((size_t)world + 1) * sizeof(uint64_t)));
    uint64_t* d_cnt = c->d_g_cnt.as<uint64_t>();
    const uint64_t pair[2] = {mine, status};
    HIP_TRY(c, hipMemcpyAsync(d_cnt + 2 * world, pair, sizeof pair, hipMemcpyHostToDevice, s));
    NCCL_TRY(c, R->AllGather(d_cnt + 2 * world, d_cnt, 2, ncclUint64, c->comm, s));
    std::vector<uint64_t> both(2 * (size_t)world);
    HIP_TRY(c, hipMemcpyAsync(both.data(), d_cnt, both.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    cnt.resize((size_t)world); st.resize((size_t)world);
    for (int r = 0; r < world; ++r) { cnt[(size_t)r] = both[2 * (size_t)r]; st[(size_t)r] = both[2 * (size_t)r + 1]; }
    return VTX_OK;
}

int vtx_gather_abort(vtx_ctx* c) {
    if (!c) return VTX_E_INVAL;
    if (!c->comm) return fail(c, VTX_E_STATE, "vtx_gather_abort: no communicator (vtx_comm_init)");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    std::vector<uint64_t> cnt, st;
    if (int rc = gather_agree(c, 0, 1, cnt, st)) return rc;
    return VTX_OK;
}

int vtx_gather_coo(vtx_ctx* c, int dst, vtx_coo* out) {
    if (!c) return VTX_E_INVAL;
    if (!out) return fail(c, VTX_E_INVAL, "vtx_gather_coo: null output");
    if (!c->comm) return fail(c, VTX_E_STATE, "vtx_gather_coo: no communicator (vtx_comm_init)");
    const int world = c->comm_world, rank = c->comm_rank;
    if (dst < 0 || dst >= world) return fail(c, VTX_E_INVAL, "vtx_gather_coo: dst %d out of range", dst);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t s = c->stream;
    Rccl* R = rccl();
    memset(out, 0, sizeof *out);
    c->g_nnz = 0;
    // round 1: counts + "my vtx_run completed"
    const uint64_t mine = c->ran ? c->nnz : 0;
    std::vector<uint64_t> cnt, st;
    if (int rc = gather_agree(c, mine, c->ran ? 0 : 1, cnt, st)) return rc;
    for (int r = 0; r < world; ++r)
        if (st[(size_t)r]) return fail(c, r == rank ? VTX_E_STATE : VTX_E_PEER, r == rank ? "vtx_gather_coo: no completed vtx_run"
                                       : "vtx_gather_coo: rank %d reported an error; exchange abandoned", r);
    std::vector<uint64_t> off((size_t)world);
    uint64_t total = 0;
    if (vtx_gather_plan(world, cnt.data(), off.data(), &total) != VTX_OK)      // (the same verdict on every rank)
        return fail(c, VTX_E_UNSUPPORTED, "vtx_gather_coo: more than 2^32 gathered triplets");
    // round 2: the destination has its buffers (the only step before the exchange that can fail on one rank alone)
    DevBuf* dstb[5] = {&c->d_g_row, &c->d_g_col, &c->d_g_alt, &c->d_g_ref, &c->d_g_unk};
    uint64_t ready = 0;
    if (rank == dst) {
        const size_t cap = (size_t)std::max<uint64_t>(total, 1);
        for (DevBuf* b : dstb) if (b->reserve(cap * sizeof(uint32_t)) != hipSuccess) ready = 1;
        if (c->d_g_val.reserve(cap * sizeof(double)) != hipSuccess || c->d_g_refval.reserve(cap * sizeof(double)) != hipSuccess) ready = 1;
        if (ready) (void)hipGetLastError();
    }
    {
        std::vector<uint64_t> c2, s2;
        if (int rc = gather_agree(c, 0, ready, c2, s2)) return rc;
        if (s2[(size_t)dst]) return fail(c, rank == dst ? VTX_E_NOMEM : VTX_E_PEER, "vtx_gather_coo: rank %d could not reserve the gathered arrays", dst);
    }
    const uint32_t* src[5] = {c->d_o_row.as<uint32_t>(), c->d_o_col.as<uint32_t>(), c->d_o_alt.as<uint32_t>(),
                              c->d_o_ref.as<uint32_t>(), c->d_o_unk.as<uint32_t>()};
    if (rank != dst) {
        if (mine) {
            NCCL_TRY(c, R->GroupStart());
            for (int f = 0; f < 5; ++f) NCCL_TRY(c, R->Send(src[f], (size_t)mine, ncclUint32, dst, c->comm, s));
            NCCL_TRY(c, R->GroupEnd());
        }
        HIP_TRY(c, hipStreamSynchronize(s));          // the source arrays may be overwritten by the next vtx_run
        return VTX_OK;
    }
    NCCL_TRY(c, R->GroupStart());
    for (int r = 0; r < world; ++r) {
        if (r == dst || !cnt[(size_t)r]) continue;
        for (int f = 0; f < 5; ++f)
            NCCL_TRY(c, R->Recv(dstb[f]->as<uint32_t>() + off[(size_t)r], (size_t)cnt[(size_t)r], ncclUint32, r, c->comm, s));
    }
    NCCL_TRY(c, R->GroupEnd());
    if (mine)
        for (int f = 0; f < 5; ++f)
            HIP_TRY(c, hipMemcpyAsync(dstb[f]->as<uint32_t>() + off[(size_t)dst], src[f], (size_t)mine * sizeof(uint32_t),
                                      hipMemcpyDeviceToDevice, s));
    HIP_TRY(c, vtxk_values_from_counts(c->d_g_alt.as<uint32_t>(), c->d_g_ref.as<uint32_t>(), c->d_g_unk.as<uint32_t>(), (uint32_t)total,
                                       c->cfg.scoring_mode, c->d_g_val.as<double>(), c->d_g_refval.as<double>(), s));
    HIP_TRY(c, hipStreamSynchronize(s));
    c->g_nnz = total;
    out->row = c->d_g_row.as<uint32_t>(); out->col = c->d_g_col.as<uint32_t>(); out->alt = c->d_g_alt.as<uint32_t>();
    out->ref = c->d_g_ref.as<uint32_t>(); out->unk = c->d_g_unk.as<uint32_t>(); out->value = c->d_g_val.as<double>();
    out->ref_value = c->d_g_refval.as<double>();
    out->nnz = total;
    return VTX_OK;
}

int vtx_fetch_gathered(vtx_ctx* c, vtx_coo* out) {
    if (!c) return VTX_E_INVAL;
    if (!out) return fail(c, VTX_E_INVAL, "vtx_fetch_gathered: null output");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return fetch_arrays(c, (size_t)c->g_nnz, c->d_g_row.p, c->d_g_col.p, c->d_g_alt.p, c->d_g_ref.p, c->d_g_unk.p, c->d_g_val.p, c->d_g_refval.p, out);
}

int vtx_last_timing(vtx_ctx* c, vtx_timing* out) {
    if (!c || !out) return VTX_E_INVAL;
    if (!c->ran) return fail(c, VTX_E_STATE, "vtx_last_timing: no completed vtx_run");
    *out = c->timing;
    return VTX_OK;
}

int vtx_last_cells(vtx_ctx* c, uint64_t* cells) {
    if (!c || !cells) return VTX_E_INVAL;
    if (!c->ran) return fail(c, VTX_E_STATE, "vtx_last_cells: no completed vtx_run");
    *cells = c->cells;
    return VTX_OK;
}

}  // extern "C"
