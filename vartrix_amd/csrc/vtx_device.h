// vtx_device.h — internal declarations shared by the kernels and the C-ABI layer.
#ifndef VTX_DEVICE_H
#define VTX_DEVICE_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/vtx.h"

// Experiment / test hooks.  The PRODUCTION library (libvtx.so) reads one environment variable, VTX_DEBUG (stderr diagnostics; changes
// no result).  Every other knob — stage on/off switches, ablations ("results wrong by design"), buffer caps that force the overflow
// paths, kernel variants, the socket transport that stands in for RCCL in tests — exists only in libvtx_dev.so, the same sources
// compiled with -DVTX_DEVTOOLS (make dev; loaded by tests/ and tools/ through VTX_LIB_VARIANT=dev).  In the production build
// VTX_DEV_ENV("...") is the constant nullptr: the branches fold away and the strings are not in the binary.
#ifdef VTX_DEVTOOLS
#include <cstdlib>
#define VTX_DEV_ENV(name) getenv(name)
#define VTX_DEVTOOLS_ON 1
#else
#define VTX_DEV_ENV(name) ((const char*)nullptr)
#define VTX_DEVTOOLS_ON 0
#endif
// a kernel's profiling-ablation selector: the constant 0 in the production build (the early exits compile out of the hot bodies)
#define VTX_ABLATE(x) (VTX_DEVTOOLS_ON ? (uint32_t)(x) : 0u)

// vtx_load_le, vtx_hash_bytes, vtx_bytes_equal (the tag bytes' hash and compare, identical on the host and the device) and the rules of the
// raw-batch preparation: vtx_prep_core.h, which the host can compile on its own (tests/prepcore/)
#include "vtx_prep_core.h"

// The banded stage's counter block (vtx_ctx::d_cnt): 64 words, all of them zeroed once per pass of the stage (BandPass::run); the groups
// say what zeroes them more often.  A group is what the host zeroes or copies as a unit, by its name and sizeof.  A kernel or launcher
// that is handed the BASE of the block (vtx_diag_routes::counters, vtx_band_out::run_counters) names the members; a kernel
// that is handed the address of a MEMBER counts from it: a vtx_cnt_pair as counters[0], counters[1] (band_kernel / band_coop_kernel:
// general; band_sweep_kernel: sweep; band_diag2_kernel: diag2, from left), a single word as *count (the full-matrix check: check, check2;
// band_diag2_kernel: streamed; slow_align_kernel: slow; band_tail_kernel: tail, recheck), the sweep's reasons as stat_counters[].
struct vtx_cnt_pair { uint32_t hard, overflow; };   // the entries of a kernel's hard list (its band slots in use) and of its overflow list (the tasks it hands on)
constexpr uint32_t VTX_DIAG_WHY_COUNT = 10;         // vtxf::W_COUNT (vtx_fast_core.h, which not every user of this header can include; vtx_band.hip asserts that the reasons fit)
struct vtx_band_counters {
    // band_run_kernel / band_pending_kernel; BandPass::cnt mirrors the group.  hard, pending: zeroed per chunk; overflow grows over the
    // chunks; why (that kernel's overflow reasons, the last one the traceback: also where its profiling aids leave their dummy store)
    // and dropped (hard only because pieces were dropped from a full list) are statistics
    struct run_t { uint32_t hard, overflow, why[6], dropped, pending; } run;
    // the general band kernel (side stream): hard tasks, tasks that need a larger slab.  Zeroed per slice of its list, again per launch
    vtx_cnt_pair general;
    // band_diag_kernel's lists and those of the kernels over its records, zeroed per chunk: tasks left for band_run_kernel, tasks for
    // band_sweep_kernel, records for band_refine_kernel / band_corridor_kernel, tasks with a one-diagonal band
    struct lists_t { uint32_t run_left, dense, refine, tight; } lists;
    // block counters of a claim loop, one per XCD: band_run_kernel's (BandPass::run_stage and its second chance zero them in front of each
    // launch) and, in libvtx_dev.so with VTX_DIAG_CLAIM=1, band_diag_kernel's before that (vtxk_launch_band_diag zeroes them in front of
    // its kernel, per chunk); the two kernels run on one stream, never side by side
    uint32_t block[8];
    // what the full-matrix check in front of the one-diagonal bands leaves, of the first stage and of the second: zeroed per launch
    uint32_t check, check2;
    // band_sweep_kernel: band slots of the slice (zeroed per slice) and declined tasks (per pass).  sweep_spare: two spare words — the second pass of round 4's kernel counted here; the kernel
    // is gone (vtx_sweep_v1.hip, last in commit 5c0dd06), the words stay so that no member behind them moves (see VTX_COUNTER_AT)
    vtx_cnt_pair sweep; uint32_t sweep_spare[2];
    struct diag2_t { uint32_t left, tight; } diag2;   // band_diag2_kernel / band_stream_kernel: tasks left for the sweep, tasks with a one-diagonal band; zeroed per call of the second stage
    uint32_t diag_why[VTX_DIAG_WHY_COUNT];   // band_diag_kernel's reasons, by vtxf::Why (statistics)
    uint32_t diag_dummy;                // where band_diag_kernel's profiling aids leave their dummy store
    uint32_t slow;                      // slow_align_kernel: tasks to retry (zeroed per call)
    // band_tail_kernel.  tail, recheck: the records band_diag_kernel leaves for it and for its recheck mode (tasks that failed the harmless test), zeroed per launch of that
    // kernel; tail_stray (libvtx_dev.so, statistics): records routed towards dense_list / fail_list although a tight list exists: must stay 0
    uint32_t tail, tail_stray, recheck;
    uint32_t recheck_total, recheck_cleared;   // statistics: the records the recheck looked at, and those the tight harmless test cleared
    uint32_t streamed;                  // band_diag2_kernel: tasks handed to band_stream_kernel; zeroed per call of the second stage
    uint32_t spare[16 - VTX_DIAG_WHY_COUNT];   // (a new word, or a new reason of vtxf::Why, takes one of these)
    uint32_t sweep_why[8];              // band_sweep_kernel's reasons (statistics)
};
static_assert(sizeof(vtx_band_counters) == 64 * 4, "the counter block is 64 words");
// The word of an array member at a RUN-TIME index, addressed as `counters[FIRST + i]` was: from the block's base, the sum formed in 32 bits.  (Written cnt->array[i] the compiler folds
// the array's offset into the instruction; that saves an addition and moves band_diag_kernel's and band_run_kernel's registers and schedule.  The kernels' code is the code
// that was measured: profiles/r20_band_counters.json.)
#define VTX_COUNTER_AT(cnt, array, i) ((uint32_t*)(cnt) + ((uint32_t)(offsetof(vtx_band_counters, array) / sizeof(uint32_t)) + (i)))

// The argument bundles of the vtxk_launch_* functions: what many launches share travels by name, what distinguishes a launch (task
// ranges, lists, tiers, workspaces, the stream) stays positional.  HOST code only: a launcher unpacks a bundle at its hipLaunchKernelGGL
// and the kernels keep their __restrict__ parameters (a pointer that reaches a kernel through a struct loses the noalias they carry).
// the batch's arrays nearly every kernel takes; filled once per run from the context
struct vtx_task_arrays { const vtx_record* records; const uint32_t* rec_locus; const vtx_locus* loci; const uint8_t* read; const uint8_t* hap; int32_t* ref; int32_t* alt; };
// the shape of one pass of the banded stage: the haplotypes it takes are those in (min_hap, max_hap] bases, max_read the batch's longest read
struct vtx_band_shape { uint32_t max_hap, min_hap, max_read, tasks_per_locus; };
// the k-mer tables in global memory: room for those of loci [gt_l0, gt_l0 + n_loci) (gtables == nullptr: tables in LDS)
struct vtx_band_tables { uint8_t* gtables; size_t gtables_bytes; uint32_t gt_l0, n_loci; };
// where band_diag_kernel and the kernels over its records (band_tail_kernel in both modes, band_refine_kernel, band_corridor_kernel)
// send a task: the lists, their counters (the base of the block) and the statistics switch.  band_diag_kernel and the
// launches of band_tail_kernel over its records take the SAME object, but for a null fail_list / dense_list where the tail says so.
struct vtx_diag_routes { uint32_t* fail_list; uint32_t* refine_rec; uint32_t refine_cap; vtx_band_counters* counters; int stats; uint32_t* tight_list; uint32_t* tight_pack;
                         uint8_t* stage; uint32_t* dense_list; uint32_t dense_mask; };
// a record buffer band_diag_kernel fills for band_tail_kernel (the tail's, the recheck's): cap records of vtxk_band_tail_words() words
struct vtx_rec_buf { uint32_t* rec; uint32_t cap; };
// where a kernel that builds bands leaves them: band slots, the hard list of the tasks that own one, the list of the tasks it cannot
// hold, and the counters of the two lists (band_run_kernel and band_pending_kernel take run_counters, the base of the block)
struct vtx_band_out { uint16_t* band; uint32_t band_stride; uint32_t* hard_list; uint32_t* overflow_list; vtx_cnt_pair* counters; vtx_band_counters* run_counters; };

extern "C" {
hipError_t vtxk_launch_sw_full(const vtx_task_arrays& a, int R, int GL, uint32_t n_work, const uint32_t* work, uint32_t max_hap_len, hipStream_t stream);
hipError_t vtxk_launch_sw_full_lut(const vtx_task_arrays& a, int R, uint32_t n_work, const uint32_t* work, uint32_t max_hap_len, uint32_t loci_cap, uint32_t* redo,
                                   uint32_t* redo_count, hipStream_t stream);
hipError_t vtxk_launch_sw_full_duo(const vtx_task_arrays& a, int R, uint32_t n_work, const uint32_t* work, uint32_t max_hap_len, uint32_t loci_cap, uint32_t* redo,
                                   uint32_t* redo_count, uint32_t pair_cols, hipStream_t stream);
hipError_t vtxk_launch_sw_banded(const vtx_task_arrays& a, int R, int GL, uint32_t n_hard, const uint32_t* hard, const uint16_t* band, uint32_t band_stride,
                                 uint32_t max_hap_len, hipStream_t stream);
size_t vtxk_band_ws_stride(uint32_t m_cap, uint32_t max_hap);
size_t vtxk_band_lds_stride(uint32_t m_cap, uint32_t max_hap, uint32_t max_read);
hipError_t vtxk_launch_band(const vtx_task_arrays& a, const uint32_t* tasks, uint32_t n_tasks, uint32_t task_base, uint8_t* workspace, uint64_t ws_stride, uint32_t m_cap,
                            const vtx_band_shape& sh, const vtx_band_out& out, int in_lds, hipStream_t s);
hipError_t vtxk_launch_band_run(const vtx_task_arrays& a, uint32_t n_tasks, uint32_t task_base, const vtx_band_shape& sh, const vtx_band_tables& tb,
                                const vtx_band_out& out, uint32_t* logbuf, uint32_t* pending_list, uint32_t* pend_buf, uint32_t hard_cap, uint32_t pend_cap,
                                const uint32_t* task_list, int long_lists, hipStream_t s);
hipError_t vtxk_launch_band_diag(const vtx_task_arrays& a, uint32_t n_tasks, uint32_t task_base, const vtx_band_shape& sh, const vtx_band_tables& tb,
                                 const vtx_diag_routes& routes, vtx_rec_buf tail, int tail_inline, vtx_rec_buf recheck, hipStream_t s);
int vtxk_band_tail_on(vtx_rec_buf tail);
int vtxk_band_recheck_on(vtx_rec_buf recheck, uint32_t max_hap);
hipError_t vtxk_launch_band_recheck(const vtx_task_arrays& a, const vtx_band_shape& sh, const vtx_diag_routes& routes, vtx_rec_buf recheck, hipStream_t s);
hipError_t vtxk_launch_band_tail(const vtx_task_arrays& a, const vtx_band_shape& sh, const vtx_diag_routes& routes, vtx_rec_buf tail, int resident_grid, hipStream_t s);
uint32_t vtxk_band_refine_words(void);
uint32_t vtxk_band_tail_words(void);
hipError_t vtxk_launch_band_corridor(const vtx_task_arrays& a, const uint32_t* recs, uint32_t n_recs, const vtx_diag_routes& routes, const uint32_t* n_dev, hipStream_t s);
hipError_t vtxk_launch_band_refine(const vtx_task_arrays& a, const uint32_t* recs, uint32_t n_recs, const vtx_band_shape& sh, const vtx_band_tables& tb,
                                   const vtx_diag_routes& routes, const uint32_t* n_dev, hipStream_t s);
// the second stage over the tasks band_diag_kernel left with too many off-diagonal matches (vtx_band.hip: band_diag2_kernel, and
// band_stream_kernel for what exceeds its list when stream_list != nullptr)
hipError_t vtxk_launch_band_diag2(const vtx_task_arrays& a, const uint32_t* tasks, uint32_t n_tasks, const vtx_band_shape& sh, const vtx_band_tables& tb,
                                  uint32_t* sweep_list, uint32_t* tight_list, uint32_t* tight_pack, uint32_t* counters, uint32_t* stream_list,
                                  uint32_t* stream_diag, uint32_t* stream_cnt, uint8_t* stage, hipStream_t s);
// ---- the band for any task (vtx_sweep.hip), the masked DP over a device-counted list, the full-matrix check ----
hipError_t vtxk_launch_band_sweep(const vtx_task_arrays& a, const uint32_t* tasks, uint32_t n_tasks, const uint32_t* n_dev, const vtx_band_out& out,
                                  uint32_t* stat_counters, uint8_t* stage, uint32_t* dbg, uint32_t* glog, hipStream_t s);
size_t vtxk_band_sweep_log_bytes(void);            // glog: the section logs of the resident workgroups
uint32_t vtxk_band_sweep_grid(uint32_t n_tasks);
uint32_t vtxk_band_sweep_max_len(void);
hipError_t vtxk_launch_sw_banded_dev(const vtx_task_arrays& a, int R, int GL, uint32_t n_cap, const uint32_t* hard, const uint32_t* n_dev, const uint16_t* band,
                                     uint32_t band_stride, uint32_t max_hap_len, hipStream_t stream);
hipError_t vtxk_launch_sw_check(const vtx_task_arrays& a, int R, int GL, uint32_t n_cap, const uint32_t* list, const uint32_t* packs, const uint32_t* n_dev,
                                uint32_t max_hap_len, uint32_t* recheck_list, uint32_t* recheck_pack, uint32_t* recheck_count, uint8_t* stage, hipStream_t stream);
hipError_t vtxk_launch_sw_diag_band(const vtx_task_arrays& a, int R, int GL, uint32_t n_cap, const uint32_t* list, const uint32_t* packs, const uint32_t* n_dev,
                                    uint32_t max_hap_len, uint8_t* stage, hipStream_t stream);
hipError_t vtxk_mark_stage(const uint32_t* list, uint32_t n, const uint32_t* n_dev, uint8_t code, uint8_t* stage, hipStream_t s);
hipError_t vtxk_mark_stage_records(const uint32_t* recs, uint32_t n, uint8_t code, uint8_t* stage, hipStream_t s);
hipError_t vtxk_fill_i32(int32_t* p, uint32_t n, int32_t v, hipStream_t s);
int vtxk_band_second_chance(uint32_t tasks_per_locus, int long_lists);
uint32_t vtxk_band_lanes(uint32_t n_tasks);
size_t vtxk_band_coop_lds(uint32_t max_hap, uint32_t mc);
hipError_t vtxk_launch_band_coop(const vtx_task_arrays& a, int tier, const uint32_t* tasks, uint32_t n_tasks, const vtx_band_shape& sh, const vtx_band_out& out, hipStream_t s);
size_t vtxk_band_gtables_bytes(uint32_t n_loci, uint32_t max_hap, uint32_t tasks_per_locus, uint32_t* loci_cap);
uint32_t vtxk_band_task_words(void);
uint32_t vtxk_band_pend_words(void);
uint32_t vtxk_band_run_grid(uint32_t nt, uint32_t wpe);
uint32_t vtxk_band_run_lanes(void);
// (out: band_run_kernel's; the kernel lists nothing in overflow_list)
hipError_t vtxk_launch_band_pending(const vtx_task_arrays& a, const uint32_t* pending, uint32_t n_pending, const uint32_t* pend_buf, const vtx_band_out& out, hipStream_t s);
uint32_t vtxk_band_poly_stride(void);
hipError_t vtxk_launch_band_expand(const vtx_task_arrays& a, const uint32_t* hard_list, uint32_t n_hard, const uint16_t* src, uint32_t src_stride, uint16_t* band,
                                   uint32_t band_stride, hipStream_t s);
/* Records the fast kernels hold: reads up to VTX_FAST_READ_LEN bases (16 rows x 64 lanes), haplotypes up to
 * VTX_FAST_HAP_LEN (LDS tables).  Longer ones take slow_align_kernel (exact, one lane per alignment, global scratch). */
#define VTX_FAST_READ_LEN 1024u
#define VTX_FAST_HAP_LEN 2400u
size_t vtxk_slow_ws_stride(uint32_t m_cap, uint32_t max_hap, uint32_t max_read);
hipError_t vtxk_launch_slow_align(const vtx_task_arrays& a, const uint32_t* recs, const uint32_t* tasks, uint32_t n_tasks, int banded, uint8_t* workspace,
                                  uint64_t ws_stride, uint32_t m_cap, uint32_t max_hap, uint32_t max_read, uint32_t* retry_list, uint32_t* counters, hipStream_t s);
hipError_t vtxk_values_from_counts(const uint32_t* alt, const uint32_t* ref, const uint32_t* unk, uint32_t n, int mode,
                                   double* o_val, double* o_refval, hipStream_t s);
hipError_t vtxk_group_heads(const vtx_record* records, const uint32_t* rec_locus, uint32_t n, uint32_t* head_cell,
                            uint32_t* head_umi, hipStream_t s);
hipError_t vtxk_group_table(const vtx_record* records, const uint32_t* rec_locus, const vtx_locus* loci, uint32_t n,
                            const uint32_t* head_cell, const uint32_t* head_umi, const uint32_t* cell_scan,
                            const uint32_t* umi_scan, uint32_t* grp_row, uint32_t* grp_col, uint32_t* umi_cellgrp,
                            uint32_t* grp_start, hipStream_t s);
// the call reduction of short groups in one pass over the scores (one thread per group, vtx_call_core.h)
uint32_t vtxk_reduce_blocks(uint32_t n_grp);     // words reduce_count_kernel writes: one per block of groups
hipError_t vtxk_reduce_count(const int32_t* ref_score, const int32_t* alt_score, const uint32_t* head_umi,
                             const uint32_t* grp_start, uint32_t n_grp, int32_t min_score, int use_umi, int mode,
                             uint32_t* blk_keep, hipStream_t s);
hipError_t vtxk_reduce_emit(const int32_t* ref_score, const int32_t* alt_score, const uint32_t* head_umi,
                            const uint32_t* grp_start, uint32_t n_grp, int32_t min_score, int use_umi, int mode,
                            const uint32_t* blk_keep_scan, const uint32_t* grp_row, const uint32_t* grp_col, uint32_t* o_row,
                            uint32_t* o_col, uint32_t* o_alt, uint32_t* o_ref, uint32_t* o_unk, double* o_val,
                            double* o_refval, hipStream_t s);
hipError_t vtxk_count_calls(const int32_t* ref_score, const int32_t* alt_score, uint32_t n, int32_t min_score,
                            const uint32_t* gscan, uint32_t* cnt, hipStream_t s);
hipError_t vtxk_umi_collapse(const uint32_t* umi_cnt, uint32_t n_umi, const uint32_t* umi_cellgrp,
                             uint32_t* cell_cnt, hipStream_t s);
hipError_t vtxk_keep_flags(const uint32_t* cell_cnt, uint32_t n_grp, int mode, uint32_t* keep, hipStream_t s);
hipError_t vtxk_emit_coo(const uint32_t* cell_cnt, uint32_t n_grp, int mode, const uint32_t* keep,
                         const uint32_t* keep_scan, const uint32_t* grp_row, const uint32_t* grp_col, uint32_t* o_row,
                         uint32_t* o_col, uint32_t* o_alt, uint32_t* o_ref, uint32_t* o_unk, double* o_val,
                         double* o_refval, hipStream_t s);
hipError_t vtxk_inclusive_scan_u32(const uint32_t* in, uint32_t* out, uint32_t n, void* temp, size_t temp_bytes,
                                   hipStream_t s);
size_t vtxk_scan_temp_bytes(uint32_t n);
// ---- vtx_prep.hip: device-side preparation of raw batches ----
hipError_t vtxk_prep_set_shapes(const uint32_t* caps, uint32_t n, uint32_t fast_read_len, uint32_t fast_hap_len);
size_t vtxk_prep_sort_temp_bytes(uint32_t n);
hipError_t vtxk_prep_sort_u64(const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out,
                              uint32_t n, int end_bit, void* temp, size_t temp_bytes, hipStream_t s);
size_t vtxk_sort_keys_u32_temp_bytes(uint32_t n);
hipError_t vtxk_sort_keys_u32(const uint32_t* keys_in, uint32_t* keys_out, uint32_t n, void* temp, size_t temp_bytes, hipStream_t s);
hipError_t vtxk_prep_sort_u8(const uint8_t* keys_in, uint8_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out,
                             uint32_t n, void* temp, size_t temp_bytes, hipStream_t s);
hipError_t vtxk_prep_rec_locus(const vtx_locus* loci, uint32_t n_loci, uint32_t* rec_locus, hipStream_t s);
hipError_t vtxk_prep_resolve(const vtx_raw_record* raw, uint32_t n, const uint32_t* rec_locus, const uint8_t* tags,
                             uint64_t tag_bytes, uint64_t read_bytes, uint32_t max_read_len, const uint32_t* bc_slots,
                             uint32_t bc_mask, const uint64_t* bc_hash, const uint64_t* bc_off, const uint8_t* bc_bytes,
                             int use_umi, uint64_t seed, uint64_t hash_mask, uint32_t cell_bits, uint32_t n_loci,
                             uint64_t* key_lc, uint64_t* key_umi, uint32_t* idx, unsigned long long* counters, hipStream_t s);
hipError_t vtxk_prep_gather_u64(const uint64_t* src, const uint32_t* idx, uint32_t n, uint64_t* dst, hipStream_t s);
hipError_t vtxk_prep_finalize(uint32_t n_kept, const uint32_t* perm, const uint64_t* key_lc_sorted, const uint64_t* key_umi,
                              const vtx_raw_record* raw, const uint8_t* tags, const vtx_locus* loci, uint32_t cell_bits,
                              int use_umi, uint32_t n_shapes, vtx_record* records, uint32_t* rec_locus, uint32_t* umi_head,
                              uint8_t* shape, uint32_t* seq, uint32_t* locus_first, uint32_t* locus_end, uint32_t* shape_cnt,
                              unsigned long long* counters, hipStream_t s);
hipError_t vtxk_prep_locus_counts(uint32_t* first_to_count, const uint32_t* end, uint32_t n_loci, hipStream_t s);
hipError_t vtxk_prep_umi_ids(vtx_record* records, const uint32_t* umi_scan, uint32_t n, hipStream_t s);
hipError_t vtxk_prep_locus_ranges(vtx_locus* loci, const uint32_t* cnt, const uint32_t* cnt_scan, uint32_t n_loci, hipStream_t s);
hipError_t vtxk_prep_lut_check(const uint32_t* work, uint32_t count, const uint32_t* rec_locus, uint32_t cap, uint32_t group,
                               uint32_t* flag, hipStream_t s);
hipError_t vtxk_unpack_nibbles(const uint8_t* in, uint64_t n_in, uint8_t* out, hipStream_t s);
hipError_t vtxk_prep_check(const vtx_record* records, uint32_t n, const uint32_t* rec_locus, const vtx_locus* loci,
                           uint64_t read_bytes, uint32_t max_read_len, uint32_t n_barcodes, int use_umi, uint32_t n_shapes, uint8_t* shape,
                           uint32_t* seq, uint32_t* shape_cnt, unsigned long long* counters, hipStream_t s);
// ---- vtx_csr.hip: row offsets of sorted keys, the checks of a caller's CSR, the stable sort of positions by column, the placement ----
// flag: one zeroed word, the OR of vtxr::Bad bits (vtx_csr_core.h).  n < 2^32 wherever positions are 32-bit (sort, place).
hipError_t vtxr_window_check(const uint32_t* row, uint64_t n, uint32_t begin, uint32_t end, uint32_t* flag, hipStream_t s);
hipError_t vtxr_offsets(const uint32_t* key, uint64_t n, uint32_t begin, uint32_t end, uint64_t* indptr, hipStream_t s);
hipError_t vtxr_check(const uint64_t* indptr, uint32_t n_major, uint64_t nnz, const uint32_t* indices, uint32_t n_minor, uint32_t* flag,
                      hipStream_t s);
size_t vtxr_sort_temp_bytes(uint64_t n, int end_bit);
hipError_t vtxr_sort_positions(const uint32_t* key, uint32_t* key_sorted, uint32_t* iota, uint32_t* perm, uint64_t n, int end_bit, void* temp,
                               size_t temp_bytes, hipStream_t s);
hipError_t vtxr_place(const uint64_t* indptr, uint32_t n_major, const uint32_t* perm, uint64_t n, uint32_t* indices_t, const void* const* in,
                      void* const* out, const uint32_t* elem_bytes, uint32_t n_payload, hipStream_t s);
// ---- vtx_csr_ops.hip: the statistics of every row of a CSR; the stable selection of rows and columns by byte masks ----
// Every CSR here has passed vtxr_check.  G: vtxr::group_lanes (vtx_csr_ops_core.h).  The maps and pos are exclusive sums made in place.
hipError_t vtxr_row_stats(const uint64_t* indptr, uint32_t n_major, const uint32_t* alt, const uint32_t* ref, const uint32_t* unk,
                          const vtx_csr_stats* out, uint32_t G, hipStream_t s);
size_t vtxr_scan_temp_bytes(uint64_t n);
hipError_t vtxr_mask_map(const uint8_t* mask, uint32_t n, uint32_t* map, void* temp, size_t temp_bytes, hipStream_t s);
hipError_t vtxr_keep_positions(const uint64_t* indptr, uint32_t n_major, const uint32_t* indices, uint64_t nnz, const uint8_t* keep_major,
                               const uint8_t* keep_minor, uint32_t* pos, void* temp, size_t temp_bytes, hipStream_t s);
hipError_t vtxr_select_offsets(const uint64_t* indptr, uint32_t n_major, const uint8_t* keep_major, const uint32_t* major_map, const uint32_t* pos,
                               uint64_t* indptr_out, hipStream_t s);
hipError_t vtxr_select_ids(const uint8_t* mask, uint32_t n, const uint32_t* map, uint32_t* ids, hipStream_t s);
hipError_t vtxr_select_place(const uint32_t* indices, uint64_t nnz, const uint32_t* pos, const uint32_t* minor_map, uint32_t* indices_out,
                             const void* const* in, void* const* out, const uint32_t* elem_bytes, uint32_t n_payload, hipStream_t s);
}
// ---- vtx_csr_group.hip: the CSR summed per group of columns (pseudobulk).  The CSR has passed vtxr_check, the labels vtxr_group_check ----
// the matrix and its labels as the count and the fill kernel read them: group[n_minor], every label < n_groups or VTX_GROUP_NONE;
// alt / ref / unk are not read by the count
struct vtx_group_in { const uint64_t* indptr; uint32_t n_major; const uint32_t* indices; const uint32_t *alt, *ref, *unk; const uint32_t* group; uint32_t n_groups; };
extern "C" {
// first_bad: one word, 0xFFFFFFFF in front of the check; behind it the lowest column whose label is neither a group nor VTX_GROUP_NONE
hipError_t vtxr_group_check(const uint32_t* group, uint32_t n_minor, uint32_t n_groups, uint32_t* first_bad, hipStream_t s);
// pos[0 .. n_major]: the (row, group) pairs in the rows below r (counted, then summed in place); pos[n_major] = nnz_out
hipError_t vtxr_group_count(const vtx_group_in& in, uint32_t* pos, void* temp, size_t temp_bytes, hipStream_t s);
// indptr_out[n_major + 1] from pos; indices_out and the arrays of `out` (any of them NULL: not written) have pos[n_major] elements
hipError_t vtxr_group_fill(const vtx_group_in& in, const uint32_t* pos, uint64_t* indptr_out, uint32_t* indices_out, const vtx_csr_stats* out,
                           hipStream_t s);
}
// ---- vtx_csr_geno.hip: a cell's reads tallied against donor genotypes.  The CSR has passed vtxr_check, the table vtxr_geno_check ----
// the matrix (rows = cells, indices = variants) and the table as the tally kernel reads them: geno[n_minor * n_donors], variant-major,
// every byte 0, 1, 2 or VTX_GENO_NONE
struct vtx_geno_in { const uint64_t* indptr; uint32_t n_major; const uint32_t* indices; const uint32_t *alt, *ref; const uint8_t* geno; uint32_t n_donors; };
extern "C" {
// first_bad: one 64-bit word, all ones in front of the check; behind it the lowest flat index of a byte that is neither a class nor VTX_GENO_NONE
hipError_t vtxr_geno_check(const uint8_t* geno, uint64_t n_bytes, uint64_t* first_bad, hipStream_t s);
// the arrays of `out` (any of them NULL: not written) have n_major * n_donors * 4 elements, each stored once
hipError_t vtxr_geno_tally(const vtx_geno_in& in, const vtx_geno_tally* out, hipStream_t s);
}
// ---- vtx_csr_geno.hip too (the same kernel over pairs): a cell's reads tallied against pairs of donors.  The CSR has passed vtxr_check,
// the table vtxr_geno_check, the pairs vtxr_geno_pair_check ----
// vtx_geno_in's matrix and table, and pairs[2 * n_pairs]: the donors (a, b) of pair p at [2 p], [2 p + 1], both < n_donors
struct vtx_geno_pair_in {
    const uint64_t* indptr; uint32_t n_major; const uint32_t* indices; const uint32_t *alt, *ref; const uint8_t* geno; uint32_t n_donors;
    const uint32_t* pairs; uint32_t n_pairs;
};
extern "C" {
// first_bad: one 64-bit word, all ones in front of the check; behind it the lowest index of a pair with a donor >= n_donors
hipError_t vtxr_geno_pair_check(const uint32_t* pairs, uint32_t n_pairs, uint32_t n_donors, uint64_t* first_bad, hipStream_t s);
// the arrays of `out` (any of them NULL: not written) have n_major * n_pairs * 6 elements, each stored once
hipError_t vtxr_geno_pair_tally(const vtx_geno_pair_in& in, const vtx_geno_pair_tally* out, hipStream_t s);
}
// ---- vtx_csr_dense.hip: a CSR times integer tables, summed modulo 2^64.  The CSR has passed vtxr_check; any int32 is a weight ----
// the matrix and the tables as the kernel reads them: w_alt / w_ref[n_minor * n_cols], minor-major; either may be NULL (its term is
// absent), both only where no row has an entry
struct vtx_dense_in { const uint64_t* indptr; uint32_t n_major; const uint32_t* indices; const uint32_t *alt, *ref; const int32_t *w_alt, *w_ref; uint32_t n_cols; };
extern "C" {
// out has n_major * n_cols elements, each stored once
hipError_t vtxr_dense_sum(const vtx_dense_in& in, int64_t* out, hipStream_t s);
}
#endif
