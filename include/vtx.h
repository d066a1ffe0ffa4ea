/*
 * vtx.h — C ABI of the MI355X-native VarTrix genotyping hot path.
 *
 * This is the drop-in boundary for the reference's per-locus hot path.  The
 * reference (10XGenomics/vartrix v1.1.22, one Rust file) has no FFI of its own;
 * the seam this library replaces is the rayon map over chunks of variant loci
 *
 *     src/main.rs:279-291   pool.install(|| rec_chunks.par_iter()
 *                               .map_with(rdr, |r, c| evaluate_chunk(c, r, &args)).collect())
 *     src/main.rs:596-607   evaluate_chunk -> Vec<(usize, EvaluateAlnResults)>
 *
 * plus its consumer, the single-threaded merge loop src/main.rs:320-348 that
 * turns per-locus Scores into matrix triplets.  The host keeps BAM/VCF/FASTA
 * ingest, read filtering (src/main.rs:829-895) and haplotype construction
 * (src/main.rs:958-994) and hands this library *packed batches*:
 *
 *   hap arena   : REF and ALT haplotype byte strings of every locus
 *   read arena  : bases of every read that reached the aligner (src/main.rs:896)
 *   records     : one per (locus, read) = one `Scores` entry of the reference
 *                 (src/main.rs:996-1001), carrying cell_index and an interned
 *                 UMI id instead of the UMI bytes (only UMI equality is used,
 *                 src/main.rs:1053-1056)
 *   loci        : matrix row + the record range + hap offsets of each locus
 *
 * and receives (a) the two Smith-Waterman scores per record — the inner seam
 * src/main.rs:898-901/926-927 — and (b) the matrix triplets of
 * consensus_scoring / alt_frac / coverage (src/main.rs:1111-1164) in the
 * insertion order of the merge loop (row ascending, then cell_index ascending,
 * src/main.rs:320-348 + :932).
 *
 * Conventions: plain C, no exceptions cross the boundary, every entry point
 * returns 0 (VTX_OK) or a negative vtx_status; vtx_strerror gives the message.
 * Inputs are borrowed for the duration of the call only.  Outputs returned by
 * pointer are owned by the context and stay valid until the next vtx_run /
 * vtx_destroy on that context.  A context is bound to one HIP device and is
 * not thread-safe; distinct contexts are independent (one per GPU / per host
 * thread — the analogue of one rayon worker, src/main.rs:466-473).
 *
 * There is NO CPU fallback in this library: every compute entry point needs a
 * gfx950 device and fails with VTX_E_NODEVICE otherwise.
 */
#ifndef VTX_H
#define VTX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VTX_ABI_VERSION 6

typedef enum vtx_status {
    VTX_OK = 0,
    VTX_E_INVAL = -1,      /* bad argument / malformed batch                      */
    VTX_E_NODEVICE = -2,   /* no usable HIP device (the library has no CPU path)  */
    VTX_E_HIP = -3,        /* a HIP runtime call failed                           */
    VTX_E_NOMEM = -4,      /* host or device allocation failed                    */
    VTX_E_UNSUPPORTED = -5,/* valid request this build cannot serve               */
    VTX_E_STATE = -6,      /* call sequence error (e.g. fetch before run)         */
    VTX_E_PEER = -7        /* a collective was abandoned because another rank reported an error */
} vtx_status;

/* Which restatement of bio::alignment::pairwise::banded::Aligner::local
 * (crate bio 0.30.0, called at src/main.rs:899-901) is computed.            */
typedef enum vtx_aligner {
    VTX_ALIGNER_BANDED = 0, /* k-mer seeded band (K=6, W=20, src/main.rs:33-34) */
    VTX_ALIGNER_FULL = 1    /* full-matrix affine local SW                      */
} vtx_aligner;

/* --scoring-method, src/main.rs:89-94 / :323-346 */
typedef enum vtx_scoring_mode {
    VTX_MODE_CONSENSUS = 0, /* consensus_scoring src/main.rs:1111-1129 */
    VTX_MODE_ALT_FRAC = 1,  /* alt_frac          src/main.rs:1131-1145 */
    VTX_MODE_COVERAGE = 2   /* coverage          src/main.rs:1147-1164 */
} vtx_scoring_mode;

/* Compile-time constants of the reference (src/main.rs:27-38) made explicit.
 * vtx_config_default() fills the reference's values.                        */
typedef struct vtx_config {
    int32_t abi_version;   /* must be VTX_ABI_VERSION                           */
    int32_t device;        /* HIP device ordinal                                */
    int32_t aligner;       /* vtx_aligner                                       */
    int32_t scoring_mode;  /* vtx_scoring_mode                                  */
    int32_t use_umi;       /* --umi, src/main.rs:121-123                        */
    int32_t match_score;   /* MATCH      =  1  src/main.rs:35                   */
    int32_t mismatch_score;/* MISMATCH   = -5  src/main.rs:36                   */
    int32_t gap_open;      /* GAP_OPEN   = -5  src/main.rs:37                   */
    int32_t gap_extend;    /* GAP_EXTEND = -1  src/main.rs:38                   */
    int32_t min_score;     /* MIN_SCORE  = 25  src/main.rs:30                   */
    int32_t kmer_k;        /* K = 6            src/main.rs:33                   */
    int32_t band_w;        /* W = 20           src/main.rs:34                   */
    uint32_t n_barcodes;   /* matrix columns (cell_barcodes.len(), :247)        */
    uint32_t reserved;
} vtx_config;

/* One variant locus = one VCF record that reached evaluate_alns
 * (src/main.rs:686).  Skipped loci (multi-allelic :646-653, invalid ALT
 * haplotype :675-684) are simply not submitted; their matrix row stays empty. */
typedef struct vtx_locus {
    uint32_t row;        /* RecHolder.i — matrix row, src/main.rs:226-228        */
    uint32_t rec_begin;  /* first record of this locus in records[]             */
    uint32_t rec_count;  /* number of records (reads that reached the aligner)  */
    uint32_t ref_off;    /* REF haplotype bytes in hap_arena (src/main.rs:984)  */
    uint32_t ref_len;
    uint32_t alt_off;    /* ALT haplotype bytes in hap_arena (src/main.rs:977-981) */
    uint32_t alt_len;
    uint32_t reserved;
} vtx_locus;

/* One scored read at one locus = one `Scores` of the reference
 * (src/main.rs:923-930) before alignment.  Within a locus, records MUST be
 * ordered by (cell_index, umi_id) ascending — the reference's stable sort by
 * cell_index (src/main.rs:932) followed by the per-cell UMI HashMap
 * (src/main.rs:1047-1057), whose iteration order never reaches the output.
 * Without cfg.use_umi the order is by cell_index alone: umi_id is not read.   */
typedef struct vtx_record {
    uint32_t read_off;   /* read bases in read_arena (rec.seq().as_bytes(), :896) */
    uint32_t read_len;
    uint32_t cell_index; /* column, get_cell_barcode src/main.rs:737-750         */
    uint32_t umi_id;     /* interned UB bytes; any value when !use_umi           */
} vtx_record;

typedef struct vtx_batch {
    const vtx_locus* loci;
    uint32_t n_loci;
    const vtx_record* records;
    uint32_t n_records;
    const uint8_t* hap_arena;   /* ASCII bytes; compared by byte equality (:898)  */
    uint64_t hap_bytes;
    const uint8_t* read_arena;  /* ASCII bytes as produced by BAM seq decoding    */
    uint64_t read_bytes;
} vtx_batch;

/* Matrix triplets in merge-loop order (src/main.rs:320-348).  `alt`, `ref`,
 * `unk` are the CellCounts of convert_to_counts (src/main.rs:1032-1039) for the
 * (row, col) group after optional UMI collapse; `value` is the f64 the
 * reference adds to `matrix`, `ref_value` the one it adds to `ref_matrix`
 * (coverage mode only, src/main.rs:336-344; 0 otherwise).                     */
typedef struct vtx_coo {
    const uint32_t* row;
    const uint32_t* col;
    const uint32_t* alt;
    const uint32_t* ref;
    const uint32_t* unk;
    const double* value;
    const double* ref_value;
    uint64_t nnz;
} vtx_coo;

/* Device-side timing of the last vtx_run, from hipEvents on the context's
 * stream (ms).  `sw_ms` covers the alignment kernels only: the full-matrix DP
 * (full flavour) or the band kernels + band-masked DP (banded flavour — it
 * never runs the full-matrix DP).                                            */
typedef struct vtx_timing {
    float total_ms;
    float sw_ms;
    float reduce_ms;
    uint32_t sw_launches;
    uint32_t hard_tasks;   /* banded flavour: alignments that needed the band-masked DP */
    float full_ms;         /* sw_full_kernel launches only (part of sw_ms)                */
    float band_ms;         /* band kernels + band-masked DP (banded flavour; part of sw_ms) */
    float band_run_ms;     /* band_run_kernel launches only (seeds, chain, certificate; part of band_ms) */
    uint32_t overflow_tasks; /* banded flavour: alignments handed to the general band kernel        */
    float diag_ms;         /* band_tables_kernel + band_diag_kernel (single-diagonal stage; part of band_run_ms).  band_tail_kernel is
                              in here only where it runs behind band_diag_kernel on the same stream; where the stage's two branches run
                              side by side (the default for haplotypes up to 255 bases) it runs on the side branch and counts in check_ms */
    uint32_t diag_left;    /* alignments the certificate stages left: band_sweep_kernel + masked DP take them       */
    float check_ms;        /* the side branch: band_tail_kernel (see diag_ms), the second look at the tasks that left with a certificate, their
                              band-masked DP (and, with VTX_BAND_CHECK, the full-matrix check); beside sweep_ms, not in front of it */
    float sweep_ms;        /* band_sweep_kernel + band-masked DP over what is left (part of band_ms)                 */
    uint32_t checked_tasks; /* alignments that left the certificate stages WITH a certificate: one-diagonal band + masked DP */
    uint32_t swept_tasks;  /* alignments handed to band_sweep_kernel                                                 */
    uint32_t resweep_tasks; /* always 0: round 4's sweep kernel, which counted its second pass here, is gone; kept for the layout */
    uint32_t diag2_tasks;  /* alignments the second single-diagonal stage looked at (band_diag2_kernel: what the first left with
                              more off-diagonal matches than its list holds) ...                                              */
    uint32_t diag2_scored; /* ... of which it decided outright (cert == ub); the rest of them is in checked_tasks (one-diagonal
                              band) or swept_tasks                                                                            */
    uint32_t diag2_streamed; /* ... and how many exceeded its list and took band_stream_kernel (the harmless test over a window)       */
} vtx_timing;

typedef struct vtx_ctx vtx_ctx;

/* Reference constants (src/main.rs:27-38), banded aligner, consensus mode.   */
void vtx_config_default(vtx_config* cfg);

/* Replaces the per-run setup of src/main.rs:266-283 (Arguments + thread pool). */
int vtx_create(const vtx_config* cfg, vtx_ctx** out);
void vtx_destroy(vtx_ctx* ctx);

/* Upload one packed batch into HBM (validates offsets/ordering first).
 * Replaces handing `rec_chunk` to a worker, src/main.rs:285-289.  The batch
 * stays resident until the next vtx_submit, so vtx_run may be repeated.      */
int vtx_submit(vtx_ctx* ctx, const vtx_batch* batch);

/* Format of the read arena of the batches submitted from now on (vtx_submit and vtx_submit_raw; sticky until set again):
 *   VTX_READS_BYTES    one ASCII byte per base, what rec.seq().as_bytes() returns (src/main.rs:896) — the default;
 *   VTX_READS_NIBBLES  two bases per byte as the BAM record holds them (high nibble first, "=ACMGRSVTWYHKDBN"): half the bytes to
 *                      write on the host and to move over PCIe.  Offsets and lengths still count BASES of the unpacked arena:
 *                      read i's packed bytes start at read_arena + read_off / 2, so every read_off must be even (a read of odd
 *                      length is followed by one unused base), read_bytes is even and the packed arena holds read_bytes / 2
 *                      bytes; the device unpacks it once per submit (unpack_nibbles_kernel) into the arena the kernels read. */
#define VTX_READS_BYTES 0
#define VTX_READS_NIBBLES 1
int vtx_set_read_format(vtx_ctx* ctx, int format);

/* ---- raw batches: barcode lookup, UMI grouping and the sort done on the device ----------------
 * A raw record is a read that passed the alignment-level filters of evaluate_alns
 * (mapq / flags / useful_alignment, src/main.rs:833-864) but whose cell barcode and UMI are
 * still the tag BYTES of the BAM record.  The device then does what the reference does per read
 * on the CPU: `cell_barcodes.get(..)` (get_cell_barcode, src/main.rs:737-750, :867-876), the
 * UB-present test (:879-888), the grouping of reads by UMI byte string (parse_scores' per-cell
 * HashMap, :1047-1057) and the sort by cell (:932).                                               */
#define VTX_TAG_MISSING 0xffffu   /* umi_len of a read without the UB tag */

typedef struct vtx_raw_record {
    uint32_t read_off;   /* into read_arena */
    uint32_t read_len;
    uint32_t bc_off;     /* cell-barcode tag bytes in tag_arena (the whole Z string, e.g. "ACGT...-1") */
    uint32_t umi_off;    /* UB tag bytes in tag_arena; ignored unless cfg.use_umi                       */
    uint16_t bc_len;
    uint16_t umi_len;    /* VTX_TAG_MISSING: no UB tag (dropped and counted when cfg.use_umi)            */
} vtx_raw_record;

typedef struct vtx_raw_batch {
    const vtx_locus* loci;          /* rec_begin/rec_count delimit RAW records (any order inside a locus) */
    uint32_t n_loci;
    const vtx_raw_record* records;
    uint32_t n_records;
    const uint8_t* hap_arena;
    uint64_t hap_bytes;
    const uint8_t* read_arena;
    uint64_t read_bytes;
    const uint8_t* tag_arena;
    uint64_t tag_bytes;
} vtx_raw_batch;

typedef struct vtx_raw_stats {
    uint64_t num_not_cell_bc;   /* barcode not in the list (Metrics.num_not_cell_bc, src/main.rs:870-876) */
    uint64_t num_non_umi;       /* use_umi and no UB tag, after the barcode test (:879-888)               */
    uint64_t kept;              /* records that reach the aligner                                         */
    float prep_ms;              /* device time of lookup + sort + regrouping                              */
    uint32_t hash_rounds;       /* UMI hash seeds tried (1 unless two UMIs of one cell collided)          */
} vtx_raw_stats;

/* Upload the barcode list (load_barcodes, src/main.rs:697-718): barcode j is
 * bytes[offsets[j] .. offsets[j+1]); j is the matrix column.  A byte string listed twice keeps
 * its FIRST index (:704-710).  n must equal cfg.n_barcodes.                                       */
int vtx_set_barcodes(vtx_ctx* ctx, const uint8_t* bytes, const uint64_t* offsets, uint32_t n);

/* vtx_submit for a raw batch: same resident state afterwards (vtx_run / vtx_fetch_* unchanged).
 * Records are resolved, filtered and ordered by (row, cell_index, UMI) on the device; the order
 * of reads inside one (row, cell, UMI) group is unspecified (no result depends on it).           */
int vtx_submit_raw(vtx_ctx* ctx, const vtx_raw_batch* batch, vtx_raw_stats* stats);

/* Parity/debug: the resolved, sorted records of the resident batch and the per-locus record
 * ranges (n_records entries of vtx_record — umi_id is a dense group number — and n_loci
 * (rec_begin, rec_count) pairs).  Buffers are caller-allocated; n_records = stats.kept.           */
int vtx_fetch_records(vtx_ctx* ctx, vtx_record* records, uint32_t* rec_begin, uint32_t* rec_count);

/* ---- vtx_submit_bam: the ingest itself on the device (round 6) -------------------------------------------------------------
 * Replaces, for one contiguous stretch of a coordinate-sorted BAM, what the reference does per locus on the CPU before the
 * aligner: `bam.fetch(tid, start, end)` + `bam.records()` (src/main.rs:822-830; rust-htslib -> htslib bgzf_read -> zlib below
 * them), the read filters in their order with the Metrics counters (:831-864: num_reads, mapq, primary, duplicates,
 * useful_alignment :790-806), the barcode / UB tags as bytes (:737-757) and rec.seq() (:896); then, as after vtx_submit_raw, the
 * in-list test, the UB test, the UMI grouping and the sort by cell.  The host hands over the FILE BYTES and an index of them:
 *   blocks     consecutive BGZF blocks (payload offset / size, ISIZE) — a header walk, no inflate;
 *   seeds      ascending offsets into the inflated stream of those blocks at which a BAM record starts: the first record to look at
 *              and whatever record starts the .bai's linear index names (SAM spec 5.2: one per 16 kb window with alignments).
 *              Record boundaries are a serial block_size chain; the seeds cut it into independent pieces.  A chain that does not
 *              land exactly on the next seed (index and file disagree) is an error, not a guess;
 *   end_upos   records starting at or beyond this offset are not looked at (a record start, or the end of the stream);
 *   intervals  the loci as the fetch sees them, per contig sorted by start (Locus {chrom, start, end}, src/main.rs:619-623);
 *   loci / hap_arena   as in vtx_raw_batch; rec_begin / rec_count are ignored (the device fills them).
 * The same resident state afterwards as after vtx_submit_raw (vtx_run / vtx_fetch_* unchanged); stats carries the Metrics
 * counters the filters produce.  VTX_E_UNSUPPORTED (with the reason in vtx_strerror) when the device declines — a block its
 * inflater does not accept, a block whose inflated bytes do not have the CRC32 of its trailer (htslib's check in bgzf_read_block;
 * always on), a block whose 8-byte trailer would lie beyond file_bytes, reads above one batch's 4 GiB arena: the caller then packs
 * on the host (libvtxhost), where zlib and the multi-batch logic live.  Nothing is read from the file but
 * [blocks[0].coff, blocks[n - 1].coff + clen + 8): the blocks' payloads and the trailer (CRC32, ISIZE) behind each.                 */
typedef struct vtx_bgzf_block {
    uint64_t coff;       /* file offset of the block's raw-DEFLATE payload (behind the gzip header and its extra field) */
    uint32_t clen;       /* payload bytes (BSIZE + 1 - header - 8)                                                      */
    uint32_t isize;      /* ISIZE: bytes it inflates to (<= 65536)                                                      */
} vtx_bgzf_block;

typedef struct vtx_bam_interval {
    int32_t start, end;  /* [start, end) on its contig, 0-based */
    uint32_t locus;      /* index into vtx_bam_ingest.loci      */
    uint32_t reserved;
} vtx_bam_interval;

typedef struct vtx_bam_ingest {
    const uint8_t* file;                 /* the BAM file's bytes (e.g. a read-only mapping) */
    uint64_t file_bytes;
    const vtx_bgzf_block* blocks;
    uint32_t n_blocks;
    uint32_t n_ref;                      /* contigs of the BAM header */
    const uint64_t* seeds;
    uint32_t n_seeds;
    uint32_t n_intervals;
    uint64_t end_upos;
    const vtx_bam_interval* intervals;   /* contig t owns [tid_begin[t], tid_begin[t + 1]) */
    const uint32_t* tid_begin;           /* n_ref + 1 entries */
    const int32_t* tid_max_span;         /* n_ref entries: the longest end - start among the contig's intervals */
    const vtx_locus* loci;
    uint32_t n_loci;
    uint32_t min_mapq;                   /* --mapq (src/main.rs:112-116)            */
    int32_t primary_only;                /* --primary-alignments (:117-119)         */
    int32_t no_duplicates;               /* --no-duplicates (:120-122)              */
    const uint8_t* hap_arena;
    uint64_t hap_bytes;
    char bam_tag[2];                     /* --bam-tag, default "CB" (:126-129)      */
    char reserved[6];
} vtx_bam_ingest;

typedef struct vtx_ingest_stats {
    uint64_t num_reads, num_low_mapq, num_non_primary, num_duplicates, num_not_useful;   /* Metrics, src/main.rs:449-459 */
    uint64_t num_no_barcode_tag;         /* reads without a usable barcode tag (part of num_not_cell_bc; raw.num_not_cell_bc has the rest) */
    uint64_t bam_records, raw_records;   /* BAM records looked at; (read, locus) pairs handed to the preparation */
    uint64_t compressed_bytes, inflated_bytes;
    vtx_raw_stats raw;
    float h2d_ms, inflate_ms, index_ms, filter_ms;   /* host wall time of the upload; device time of the inflate, the record chains, the filter passes */
    float prefetch_ms, prefetch_wait_ms;             /* vtx_prefetch_file: how long its copy took; how long vtx_submit_bam waited for it (0: not used) */
} vtx_ingest_stats;

/* Optional, before vtx_submit_bam: start moving bytes [file_off, file_off + n) of the file at `path` (n = 0: to its end) to the device
 * NOW — while the host still parses the VCF and walks the BGZF headers.  Returns at once; library threads copy the file (through a
 * read-only mapping of their own) into their pinned buffers and push them.  A later
 * vtx_submit_bam whose blocks lie inside the range uses the bytes (it waits for the copy first), any other uploads its own.  A
 * context may be created for this before the barcode list is known: cfg.n_barcodes = 0 means "taken from the first
 * vtx_set_barcodes".  Every entry point that moves data through the context's copy workers or takes the prefetch's device buffer waits
 * for a copy in flight first: vtx_submit, vtx_submit_raw, vtx_debug_crc32 and a plain vtx_mtx_part keep the prefetched bytes for a later
 * vtx_submit_bam; a later vtx_prefetch_file, vtx_debug_inflate and the gzip matrix writers drop them.                                  */
int vtx_prefetch_file(vtx_ctx* ctx, const char* path, uint64_t file_off, uint64_t n);
int vtx_submit_bam(vtx_ctx* ctx, const vtx_bam_ingest* ingest, vtx_ingest_stats* stats);

/* ---- vtx_submit_bam_segments: the same ingest for SPARSE loci (round 9) -------------------------------------------------------
 * A few thousand loci on a BAM of tens of GB: one contiguous stretch from the first locus to the last would be the whole file.  The
 * plan is a list of SEGMENTS instead, each a run of consecutive BGZF blocks with the record starts inside it — what the reference's
 * indexed fetch per locus reads (src/main.rs:822-826), merged where two fetches touch.  `base` is a vtx_bam_ingest whose arrays are the
 * segments' back to back: base.blocks ascending in the file and consecutive only INSIDE a segment (only those byte ranges travel, into
 * one compact device buffer); base.seeds and segment.end_upos are offsets into the CONCATENATION of the segments' inflated bytes;
 * base.end_upos is ignored.  Segment k owns blocks [block_begin, block_end) and seeds [seed_begin, seed_end), both tiling the arrays
 * in order.  A chain stops at the next seed of its segment; the segment's last chain must land on end_upos — a record start the
 * index names a few windows behind the segment's last locus (or, VTX_SEGMENT_TO_EOF, the end of the file's records).  No record at
 * or behind end_upos is looked at, so the end has to be PROVEN: the record at end_upos must lie on a contig behind end_tid or start
 * at / behind end_pos (the end of the segment's last locus; coordinate-sorted file: nothing later can overlap the segment's loci).
 * The 12 bytes that hold its (tid, pos) are part of the segment's blocks.  A segment that cannot prove its end (a read spliced over
 * all those windows) is never used: VTX_E_UNSUPPORTED, nothing submitted, the caller packs on the host.  Segments are disjoint in
 * the file, so every BAM record is looked at once and the (read, locus) pairs come in BAM order, as from vtx_submit_bam.
 * Afterwards: the state vtx_submit_raw leaves; stats.compressed_bytes / inflated_bytes = the bytes that travelled / were inflated.
 * A vtx_prefetch_file still in flight is cancelled, not waited for: its bytes are of no use here.                                 */
#define VTX_SEGMENT_TO_EOF 1u
typedef struct vtx_bam_segment {
    uint32_t block_begin, block_end;     /* base.blocks[block_begin .. block_end): consecutive in the file                        */
    uint32_t seed_begin, seed_end;       /* base.seeds[seed_begin .. seed_end): ascending, inside this segment's inflated bytes   */
    uint64_t end_upos;                   /* where the last chain lands (offset into the concatenated inflated stream)             */
    int32_t end_tid, end_pos;            /* the record at end_upos must be beyond (end_tid, end_pos)                              */
    uint32_t flags;                      /* VTX_SEGMENT_TO_EOF: end_upos is the end of the file's records, nothing to prove       */
    uint32_t reserved;
} vtx_bam_segment;

typedef struct vtx_bam_segments {
    vtx_bam_ingest base;
    const vtx_bam_segment* segments;
    uint32_t n_segments;
    uint32_t contiguous_blocks;          /* for the log: what ONE stretch from the first locus to the last would have been */
    uint64_t contiguous_compressed, contiguous_inflated;
} vtx_bam_segments;

int vtx_submit_bam_segments(vtx_ctx* ctx, const vtx_bam_segments* plan, vtx_ingest_stats* stats);

/* Test / audit hook: intermediate arrays of the last vtx_submit_bam / vtx_submit_bam_segments (there: the concatenated stream and
 * offsets into it).  *bytes = the array's size, min(cap, *bytes) bytes go to dst. */
#define VTX_INGEST_INFLATED 0        /* the inflated stream of the submitted blocks                           */
#define VTX_INGEST_RECORD_OFFSETS 1  /* uint64 per BAM record: where its block_size word lies in that stream */
#define VTX_INGEST_RAW_RECORDS 2     /* vtx_raw_record per surviving (read, locus) pair, BAM order            */
#define VTX_INGEST_RAW_LOCUS 3       /* uint32 per pair: its locus                                            */
#define VTX_INGEST_TAGS 4            /* the tag arena those records point into                                */
#define VTX_INGEST_READS_PACKED 5    /* the read arena, two bases per byte                                    */
int vtx_debug_ingest(vtx_ctx* ctx, int what, void* dst, uint64_t cap, uint64_t* bytes);
/* Test hook: the device's BGZF inflater on arbitrary raw-DEFLATE payloads (block i = file[coff .. coff + clen), expected to inflate
 * to isize bytes): status[i] = 0 accepted, its bytes at out + (sum of the isizes before it); else the decoder's reason.  The product
 * path (vtx_submit_bam) treats any non-zero status as "the host packer decides".                                              */
int vtx_debug_inflate(vtx_ctx* ctx, const uint8_t* file, uint64_t file_bytes, const vtx_bgzf_block* blocks, uint32_t n_blocks,
                      uint8_t* out, uint64_t out_cap, uint32_t* status);
/* Test hook: the device's CRC-32 (bgzf_crc32_kernel: gzip's, bit for bit zlib's) of arbitrary byte ranges: range i is
 * data[offsets[i] .. offsets[i + 1]) (n + 1 offsets, ascending, each range at most 65536 bytes), crc_out[i] its value.           */
int vtx_debug_crc32(vtx_ctx* ctx, const uint8_t* data, uint64_t n_bytes, const uint64_t* offsets, uint32_t n, uint32_t* crc_out);
/* Device time of the context's last CRC32 check in milliseconds (the last vtx_submit_bam / vtx_submit_bam_segments that succeeded,
 * or vtx_debug_crc32; vtx_ingest_stats.inflate_ms does not contain it).                                                            */
int vtx_last_crc_ms(vtx_ctx* ctx, float* ms);

/* Run the hot path on the resident batch: Smith-Waterman of every record
 * against both haplotypes (src/main.rs:898-901), per-read call
 * (evaluate_scores :1019-1030), UMI collapse (parse_scores :1041-1109) and the
 * per-(row, cell) count histogram; results stay in HBM.  Synchronous: returns
 * after the device finished.  Replaces evaluate_chunk + the scoring half of
 * the merge loop.                                                            */
int vtx_run(vtx_ctx* ctx);

/* Copy the per-record scores of the last vtx_run to host arrays of n_records
 * int32 each (Scores.ref_score / alt_score, src/main.rs:926-927).            */
int vtx_fetch_scores(vtx_ctx* ctx, int32_t* ref_score, int32_t* alt_score);

/* Copy the triplets of the last vtx_run to context-owned host memory.        */
int vtx_fetch_coo(vtx_ctx* ctx, vtx_coo* out);

/* Device pointers of the last vtx_run's per-record scores (for callers that
 * keep results on the GPU, e.g. an RCCL gather).  int32[n_records] each.     */
int vtx_device_scores(vtx_ctx* ctx, const int32_t** d_ref, const int32_t** d_alt);

/* sprs::io::write_matrix_market of the last vtx_run's triplets (src/main.rs:381-389: three header lines, then "row+1 col+1 value"
 * per triplet in insertion order) — formatted on the device and streamed into `path` by the copy workers; the triplets never become
 * host arrays.  which: 0 = `value` (the matrix), 1 = `ref_value` (coverage mode's ref matrix, :385-389).  Integral values only
 * (consensus 1 / 2 / 3, coverage counts: Rust's `{}` of such an f64 is its digits); alt_frac's fractions / NaN return
 * VTX_E_UNSUPPORTED and leave nothing at `path` — use vtx_write_mtx_f64, or format those on the host (vtx_fetch_coo +
 * vtxh_write_mtx).  *sum (optional): the sum of the values written (the reference's "sum of 0" warning, :410-415).                      */
int vtx_write_mtx(vtx_ctx* ctx, const char* path, uint32_t n_rows, uint32_t n_cols, int which, double* sum);

/* vtx_write_mtx for ANY value vtx_run produces — alt_frac's fractions and NaN included: Rust's `{}` of an f64, the shortest digits
 * that round-trip, positional (0.3333333333333333, 0.000033333333333333335, NaN), formatted per lane on the device; byte-identical to
 * vtx_fetch_coo + vtxh_write_mtx.  Integral matrices come out as from vtx_write_mtx.  Domain: NaN, +-0 and 2^-40 <= |v| < 2^53; a
 * value outside it (infinite, subnormal, larger, smaller — nothing a scoring mode computes) returns VTX_E_UNSUPPORTED and leaves
 * nothing at `path`.  *sum (optional): the sum of the values, added up in no fixed order; NaN when a value is NaN (what the host's
 * `sum += v` gives: the "sum of 0" warning stays silent).  (A second name because vtx_write_mtx's refusal of fractions is pinned.)  */
int vtx_write_mtx_f64(vtx_ctx* ctx, const char* path, uint32_t n_rows, uint32_t n_cols, int which, double* sum);

/* The same text gzip-compressed ON THE DEVICE: `path` (used exactly as given) becomes a BGZF file — a series of gzip members of at
 * most 65 280 text bytes each, then BGZF's 28-byte empty member — that zcat, Python's gzip, scanpy.read_10x_mtx and Seurat Read10X
 * read as matrix.mtx.gz; decompressed it is byte for byte what vtx_write_mtx (real = 0) or vtx_write_mtx_f64 (real != 0) writes, the
 * three header lines included.  One wavefront deflates one chunk (LZ77 inside the chunk, the cheapest of a stored, a fixed-Huffman and a
 * dynamic-Huffman block; vartrix_amd/csrc/vtx_deflate_core.h), and only the compressed bytes leave the card.  The bytes are a
 * function of the text alone: every run and the host build of the encoder give the same file.  Preconditions, which, the decline
 * rule (VTX_E_UNSUPPORTED, nothing left at `path`) and *sum as for the two calls above.  *text_bytes (optional): the uncompressed size.
 * Like vtx_write_mtx this call works in the buffers of the device ingest: what vtx_debug_ingest returned before it is no longer
 * there afterwards.  Unlike it, it also takes the buffer of vtx_prefetch_file: it waits for a prefetch in flight and DROPS the
 * prefetched bytes (a later vtx_submit_bam of that file uploads them again).  Device memory while it runs, beyond the text of a
 * pass (T bytes): 2 T for the members' slots and their compacted copy, and 261 120 bytes of token work space per resident workgroup
 * (at most 1 536: 401 MB) — about 1 GB at 306 MB of text; the buffers stay with the context like the ingest's.                     */
int vtx_write_mtx_gz(vtx_ctx* ctx, const char* path, uint32_t n_rows, uint32_t n_cols, int which, int real, double* sum,
                     uint64_t* text_bytes);

/* ---- the matrix in PARTS: for callers that run several batches (streamed ranges of loci, batches of one pack) ----------------------
 * The three calls above write a whole file from ONE vtx_run.  A caller that feeds the loci in several runs — rows ascending from run
 * to run, as vtxh_pack_files_range and the batches of a pack give them — takes a PART after each run instead and joins the parts at
 * the end; nothing stays on the device between the runs, and the context may be destroyed or reused as soon as the call returns.
 *   vtx_mtx_part       the last vtx_run's triplets as a finished piece of the file in host memory: the lines "row+1 col+1 value" and
 *                      nothing else (gz = 0), or those lines as BGZF members (gz != 0: chunks of at most 65 280 text bytes counted from
 *                      the part's first byte, deflated on the device; no header lines, no end-of-file member).  which and real as for
 *                      vtx_write_mtx (real = 0) / vtx_write_mtx_f64 (real != 0), and the same decline rule: VTX_E_UNSUPPORTED, *out
 *                      zeroed, the context usable — format that run on the host (vtx_fetch_coo + vtxh_mtx_part of vtx_host.h; such a
 *                      part joins like any other).  VTX_E_STATE before a completed vtx_run, VTX_E_INVAL for a bad argument.  A run
 *                      without triplets gives nnz = 0, n_bytes = 0, bytes = NULL (no member).  The engine is vtx_write_mtx's: the
 *                      text is the same bytes, the call is synchronous on the context's stream and, like vtx_write_mtx, works in the
 *                      buffers of the device ingest (what vtx_debug_ingest returned before is gone).  It waits for a
 *                      vtx_prefetch_file in flight (the part comes back through the copy workers the prefetch uses); with gz it
 *                      also drops the prefetched bytes, like vtx_write_mtx_gz.  `bytes` belongs to the library: vtx_mtx_part_free.
 *   vtx_mtx_part_free  releases `bytes` and zeroes the struct; nothing to do on a zeroed struct.
 *   vtx_mtx_join       no context, no device: writes `path` = the three header lines with nnz = the sum of the parts' nnz, then the
 *                      parts in the order given.  gz != 0: the header lines are a BGZF member of their own (a stored block) in front,
 *                      BGZF's 28-byte empty member ends the file.  Reads only bytes, n_bytes, text_bytes, nnz and gz of a part.  A
 *                      part whose gz differs from the argument: VTX_E_INVAL.  On any error nothing is left at `path`; the message is
 *                      vtx_strerror(NULL).  No parts, or only empty ones: a valid file with the header alone.  *text_bytes
 *                      (optional): the uncompressed size of the file.
 * Joined, the plain file is byte for byte what vtx_write_mtx / vtx_write_mtx_f64 / vtxh_write_mtx write for all the triplets at once;
 * the gz file decompresses to it (its members are cut differently from vtx_write_mtx_gz's: per part, the header apart).             */
struct vtx_mtx_part {
    uint8_t* bytes;      /* the part: text lines, or BGZF members (no header lines, no EOF member) */
    uint64_t n_bytes;
    uint64_t text_bytes; /* uncompressed size (== n_bytes when gz == 0) */
    uint64_t nnz;        /* lines in this part */
    double   sum;        /* as vtx_write_mtx's *sum: NaN when a value is NaN */
    uint32_t gz;         /* 0 text, 1 BGZF members */
    uint32_t reserved;
};   /* (a struct tag only, no typedef: the call that fills it has the same name, so the type is always written `struct vtx_mtx_part`) */
int vtx_mtx_part(vtx_ctx* ctx, int which, int real, int gz, struct vtx_mtx_part* out);
void vtx_mtx_part_free(struct vtx_mtx_part* part);
int vtx_mtx_join(const char* path, uint32_t n_rows, uint32_t n_cols, int gz, const struct vtx_mtx_part* parts, uint32_t n_parts,
                 uint64_t* text_bytes);

/* Device pointers of the last vtx_run's triplets (same layout as vtx_coo, all
 * arrays resident in HBM) — the payload of the multi-GPU row gather.          */
int vtx_device_coo(vtx_ctx* ctx, vtx_coo* out);

/* ---- the matrices as CSR on the device (vartrix_amd/csrc/vtx_csr.hip) --------------------------------------------------------------
 * The triplets of a run are in merge-loop order (row ascending, column ascending inside a row), so they ARE a variant-major CSR but
 * for the row offsets: `indices` is vtx_coo.col and every data array is the vtx_coo array of the same name — the same addresses
 * vtx_device_coo reports, nothing is copied.  Only `indptr` is new: indptr[r - row_begin], r in [row_begin, row_end], is the offset of
 * the first triplet whose row is >= r, so a row without triplets (a skipped record, a locus no read reached, the empty stretches at
 * the ends of the window) has an empty range.                                                                                        */
typedef struct vtx_csr {
    const uint64_t* indptr;      /* row_end - row_begin + 1 offsets into the arrays below */
    const uint32_t* indices;     /* == vtx_coo.col */
    const uint32_t *alt, *ref, *unk;
    const double *value, *ref_value;
    uint64_t nnz;
    uint32_t row_begin, row_end, n_cols, reserved;   /* n_cols = cfg.n_barcodes */
} vtx_csr;

/* Variant-major CSR of the last vtx_run's triplets over the rows [row_begin, row_end); DEVICE pointers.  VTX_E_STATE before a
 * completed vtx_run; VTX_E_INVAL for row_begin > row_end or when a triplet's row lies outside the window (the window must hold every
 * triplet of the run: the arrays are the run's, not a slice of them).  A run without triplets: nnz = 0 and indptr all zero.
 * Lifetime: the data arrays live as vtx_device_coo's do, until the next vtx_run / vtx_destroy on the context; `indptr` lives in a
 * buffer of its own until the next vtx_device_csr, vtx_run or vtx_destroy.  That buffer is none of the device ingest's: the calls
 * that work in those (vtx_write_mtx, vtx_write_mtx_gz, vtx_mtx_part, and the f64 writer) neither disturb a vtx_csr taken before them nor
 * are disturbed by this call, and it may be repeated after any of them.  It changes nothing vtx_device_coo / vtx_fetch_coo return.
 * Synchronous on the context's stream.  The offsets take 8 (row_end - row_begin + 1) bytes of device memory (VTX_E_NOMEM when the
 * device does not have them); their cost does not depend on how the triplets are spread over the window: a stretch of more than 256
 * rows without triplets is written by one lane per row, not by one lane.                                                             */
int vtx_device_csr(vtx_ctx* ctx, uint32_t row_begin, uint32_t row_end, vtx_csr* out);

/* Stable transpose of ANY CSR in caller-owned DEVICE memory into caller-owned device memory; needs no run (the context gives the
 * device, the stream and the work space).  In: d_indptr[n_major + 1], d_indices[nnz] (each < n_minor; inside a row in any order,
 * duplicates allowed).  Out: d_indptr_t[n_minor + 1], d_indices_t[nnz] and (optional, may be NULL) d_perm[nnz] with
 *     d_indices_t[k] = the major index of source entry perm[k],     perm == the STABLE argsort of d_indices:
 * inside an output row the entries keep their source order (for the library's own triplets: ascending), so the result is a function
 * of the input alone.  n_payload arrays of nnz elements of payload_elem_bytes[i] = 4 or 8 bytes move with the entries,
 * d_payload_out[i][k] = d_payload_in[i][perm[k]], bit for bit (NaN payloads, -0.0, explicit zeros).  The three arrays of pointers and
 * sizes are HOST arrays of device pointers.  Outputs must not overlap inputs.
 * The inputs are checked on the device BEFORE anything is written through them: indptr[0] == 0, indptr non-decreasing,
 * indptr[n_major] == nnz, every index < n_minor; a violation returns VTX_E_INVAL (the reason in vtx_strerror), no output byte is
 * written and the context stays usable.  VTX_E_UNSUPPORTED for nnz >= 2^32; VTX_E_INVAL for a null array that is needed or an element
 * size other than 4 / 8.  Synchronous on the context's stream.
 * Work space (stays with the context, like the ingest's): 8 nnz bytes of sorted keys and positions (12 nnz when d_perm is NULL) plus
 * the radix sort's own: about 8 nnz + 64 KiB more.  n_minor adds nothing: the offsets go straight into d_indptr_t.               */
int vtx_csr_transpose(vtx_ctx* ctx, uint32_t n_major, uint32_t n_minor, uint64_t nnz,
                      const uint64_t* d_indptr, const uint32_t* d_indices,
                      uint64_t* d_indptr_t, uint32_t* d_indices_t, uint32_t* d_perm,
                      const void* const* d_payload_in, void* const* d_payload_out,
                      const uint32_t* payload_elem_bytes, uint32_t n_payload);

/* ---- summaries and selections of a CSR (vartrix_amd/csrc/vtx_csr_ops.hip) -------------------------------------------------------------
 * The first two steps of every consumer of the variants x cells matrices, where the matrices are: the per-row counts of entries with
 * alt / ref support, and the selection of rows and columns by masks (the locus filter of the demultiplexers).  Like vtx_csr_transpose
 * these work on ANY CSR in caller-owned DEVICE memory, need a context (device, stream, work space) but no run, are synchronous on the
 * context's stream, and check their inputs on the device BEFORE anything is written: indptr[0] == 0, indptr non-decreasing,
 * indptr[n_major] == nnz, every index < n_minor; a violation returns VTX_E_INVAL (the reason in vtx_strerror), no output byte is
 * written and the context stays usable.  VTX_E_UNSUPPORTED for nnz >= 2^32; VTX_E_INVAL for a null array that is needed or a payload
 * element size other than 4 / 8.  Integer work only: every result is a function of the input alone.
 *
 * The seven statistics of a row, from the (alt, ref, unk) counts of its entries; n_major elements each, any pointer may be NULL (that
 * array is not written).  The counts are u32, the sums u64: a row of u32 counts can pass 2^32.                                        */
typedef struct vtx_csr_stats {
    uint32_t *n_entries, *n_alt, *n_ref, *n_both;   /* entries; entries with alt > 0; with ref > 0; with both (what consensus writes as 3) */
    uint64_t *sum_alt, *sum_ref, *sum_unk;          /* sums of the counts */
} vtx_csr_stats;

/* The statistics of every row of the CSR d_indptr[n_major + 1], d_indices[nnz] whose entries carry the counts d_alt / d_ref /
 * d_unk[nnz] (vtx_csr's arrays, or the payloads a vtx_csr_transpose moved: then the rows are cells).  A row without entries gets
 * zeros.  A group of 1 .. 64 lanes (from nnz / n_major alone) walks a row and folds inside its wavefront: no atomics, no zeroing
 * pass.  A row is walked by its one group however long it is: for the library's own matrices that is at most n_minor entries; a CSR
 * with duplicate indices (longer rows) is accepted and correct, and need not be fast.  d_indices is read by the check only.  No work
 * space beyond the check's flag word.                                                                                                */
int vtx_csr_row_stats(vtx_ctx* ctx, uint32_t n_major, uint32_t n_minor, uint64_t nnz,
                      const uint64_t* d_indptr, const uint32_t* d_indices,
                      const uint32_t* d_alt, const uint32_t* d_ref, const uint32_t* d_unk,
                      const vtx_csr_stats* out);

/* Stable selection of rows and columns.  d_keep_major[n_major] / d_keep_minor[n_minor] are byte masks: any non-zero byte keeps, a
 * NULL mask keeps everything (a bool array is a valid mask as it is).  An entry survives when its row and its column do; the kept rows
 * and columns are renumbered 0, 1, ... in their order, and the entries keep their source order inside a row.
 * vtx_csr_select_plan reports the sizes of the result: the caller allocates d_indptr_out[n_major_out + 1], d_indices_out[nnz_out], the
 * payload outputs of nnz_out elements and, if wanted, d_major_ids[n_major_out] / d_minor_ids[n_minor_out] (the source row / column of
 * every kept one; may be NULL), and passes the three sizes back to vtx_csr_select.  vtx_csr_select is STATELESS: it recomputes the
 * sizes from its own arguments, and if they differ from the ones passed in it returns VTX_E_INVAL and writes no output byte — an
 * allocation made for another selection cannot be overrun.  d_indices_out receives the NEW column numbers; n_payload arrays of
 * payload_elem_bytes[i] = 4 or 8 bytes per entry move with the kept entries, bit for bit (NaN payloads, -0.0, explicit zeros).  The
 * three arrays of pointers and sizes are HOST arrays of device pointers.  Outputs must not overlap inputs.
 * Work space (stays with the context, like the transpose's): 4 (nnz + 1) bytes of positions, 4 (n_major + n_minor + 2) bytes of maps
 * and the scan's own.                                                                                                                */
int vtx_csr_select_plan(vtx_ctx* ctx, uint32_t n_major, uint32_t n_minor, uint64_t nnz,
                        const uint64_t* d_indptr, const uint32_t* d_indices,
                        const uint8_t* d_keep_major, const uint8_t* d_keep_minor,
                        uint32_t* n_major_out, uint32_t* n_minor_out, uint64_t* nnz_out);
int vtx_csr_select(vtx_ctx* ctx, uint32_t n_major, uint32_t n_minor, uint64_t nnz,
                   const uint64_t* d_indptr, const uint32_t* d_indices,
                   const uint8_t* d_keep_major, const uint8_t* d_keep_minor,
                   uint32_t n_major_out, uint32_t n_minor_out, uint64_t nnz_out,
                   uint64_t* d_indptr_out, uint32_t* d_indices_out,
                   uint32_t* d_major_ids, uint32_t* d_minor_ids,
                   const void* const* d_payload_in, void* const* d_payload_out,
                   const uint32_t* payload_elem_bytes, uint32_t n_payload);

/* ---- pseudobulk: the CSR summed per group of columns (vartrix_amd/csrc/vtx_csr_group.hip) ----------------------------------------------
 * The step after the statistics and the filter: with a label per column (per cell: its cluster, donor, clone, sample) the n_major x
 * n_minor matrix folds into n_major x n_groups.  d_group[n_minor] holds a group number < n_groups per column, or VTX_GROUP_NONE for a
 * column that belongs to no group: its entries are left out.  The result is a CSR with one entry per (row, group) pair that has at
 * least one source entry, group numbers ascending inside a row; each entry carries the seven numbers of vtx_csr_stats over the source
 * entries of that row whose column has that label (so n_alt is the number of cells of the group with alt support, sum_alt their alt
 * count).  vtx_csr_stats is the output struct, its arrays nnz_out long; any pointer may be NULL and is then not written.
 * Like vtx_csr_select these work on ANY CSR in caller-owned DEVICE memory (rows in any order inside, duplicate indices allowed), need
 * a context but no run, are synchronous on the context's stream, and check their inputs on the device BEFORE anything is written: the
 * CSR as above, then the labels: every d_group[j] must be < n_groups or == VTX_GROUP_NONE.  A violation returns VTX_E_INVAL (the reason
 * in vtx_strerror; for a label it names the lowest offending column), no output byte is written and the context stays usable.
 * VTX_E_INVAL also for n_groups == 0 and a null array that is needed; VTX_E_UNSUPPORTED for nnz >= 2^32 and for n_groups >
 * vtx_csr_group_max().  vtx_csr_group_plan reports nnz_out: the caller allocates d_indptr_out[n_major + 1], d_indices_out[nnz_out] and
 * the arrays of `out`, and passes nnz_out back.  vtx_csr_group_sum is STATELESS: it recounts, and if its own nnz_out differs from the
 * one passed in it returns VTX_E_INVAL and writes no output byte.  Outputs must not overlap inputs.
 * One wavefront folds a row in a tile of vtx_csr_group_window() groups in LDS; with more groups it repeats the row once per window
 * (correct, and need not be fast), which vtx_csr_group_max() = 256 windows bounds.  Integer additions only: the result is a function
 * of the input alone.  Work space (stays with the context): 4 (n_major + 1) bytes of counts plus the scan's own.                       */
#define VTX_GROUP_NONE 0xFFFFFFFFu     /* a column that belongs to no group: its entries are left out */
uint32_t vtx_csr_group_window(void);   /* W: groups one pass holds in LDS */
uint32_t vtx_csr_group_max(void);      /* the largest n_groups accepted */
int vtx_csr_group_plan(vtx_ctx* ctx, uint32_t n_major, uint32_t n_minor, uint64_t nnz,
                       const uint64_t* d_indptr, const uint32_t* d_indices,
                       const uint32_t* d_group, uint32_t n_groups, uint64_t* nnz_out);
int vtx_csr_group_sum(vtx_ctx* ctx, uint32_t n_major, uint32_t n_minor, uint64_t nnz,
                      const uint64_t* d_indptr, const uint32_t* d_indices,
                      const uint32_t* d_alt, const uint32_t* d_ref, const uint32_t* d_unk,
                      const uint32_t* d_group, uint32_t n_groups, uint64_t nnz_out,
                      uint64_t* d_indptr_out, uint32_t* d_indices_out, const vtx_csr_stats* out);

/* ---- donor tally: a cell's reads by the genotype class of every pooled donor (vartrix_amd/csrc/vtx_csr_geno.hip) ------------------------
 * The step that produces the donor label: cells of pooled samples are scored against the known genotypes of the donors.  The CSR's
 * MINOR dimension is the variants (rows = cells: the payloads a vtx_csr_transpose moved).  d_geno[n_minor * n_donors] holds one byte
 * per (variant, donor), variant-major: 0 hom-ref, 1 het, 2 hom-alt, or VTX_GENO_NONE for a donor without a call there.  For every
 * (row r, donor d, class g = 0, 1, 2, 3 = missing), at element (r * n_donors + d) * 4 + g of each array of `out`:
 *   sum_alt / sum_ref   the alt / ref counts summed over the entries of row r whose variant has class g in donor d
 *   n_obs               how many of those entries have alt + ref > 0
 * Every likelihood model in use is a linear function of these numbers.  The arrays have n_major * n_donors * 4 elements; any pointer
 * may be NULL and is then not written; every element of the others is written, zeros for rows without entries.
 * Like vtx_csr_select this works on ANY CSR in caller-owned DEVICE memory (rows in any order inside, duplicate indices allowed: every
 * entry counts), needs a context but no run, is synchronous on the context's stream, and checks its inputs on the device BEFORE
 * anything is written: the CSR as above, then the table: every byte must be 0, 1, 2 or VTX_GENO_NONE.  A violation returns VTX_E_INVAL
 * (the reason in vtx_strerror; for a byte it names the variant and the donor of the lowest offending position), no output byte is
 * written and the context stays usable.  VTX_E_INVAL also for n_donors == 0, a null `out` and a null array that is needed (d_geno
 * unless n_minor == 0); VTX_E_UNSUPPORTED for nnz >= 2^32 and for n_donors > vtx_csr_geno_max().  Outputs must not overlap inputs.
 * One wavefront walks a row with up to 64 donors on its lanes and keeps the twelve numbers of a donor in registers; with more donors
 * it repeats the row once per 64 (correct, and need not be fast), which vtx_csr_geno_max() = 16 passes bounds.  No atomics, no zeroing
 * pass, integer additions only: the result is a function of the input alone.  Work space: the checks' flag words only.                */
#define VTX_GENO_NONE 0xFFu            /* a donor without a genotype call at a variant */
typedef struct vtx_geno_tally {
    uint64_t *sum_alt, *sum_ref;       /* n_major * n_donors * 4 elements each */
    uint32_t *n_obs;
} vtx_geno_tally;
uint32_t vtx_csr_geno_max(void);       /* the largest n_donors accepted */
uint32_t vtx_sizeof_geno_tally(void);  /* sizeof(vtx_geno_tally) as the library was built: 24 (the table of vtx_abi_sizes is unchanged) */
int vtx_csr_geno_tally(vtx_ctx* ctx, uint32_t n_major, uint32_t n_minor, uint64_t nnz,
                       const uint64_t* d_indptr, const uint32_t* d_indices,
                       const uint32_t* d_alt, const uint32_t* d_ref,
                       const uint8_t* d_geno, uint32_t n_donors, const vtx_geno_tally* out);

/* ---- doublet tally: a cell's reads by the dosage class of pairs of pooled donors (vartrix_amd/csrc/vtx_csr_geno.hip) --------------------
 * The two-donor hypotheses beside vtx_csr_geno_tally's one-donor ones.  A droplet that holds cells of the donors a and b in EQUAL parts
 * shows an alt read at a variant with a probability that depends only on the dosage g_a + g_b in 0 .. 4; unequal mixtures are out of
 * scope.  The CSR and d_geno[n_minor * n_donors] are exactly vtx_csr_geno_tally's.  d_pairs[2 * n_pairs], in device memory, holds the
 * donors (a, b) of pair p at [2 p], [2 p + 1]; any list is allowed: duplicates, both orders, a == b.  For every (row r, pair p, class
 * c), at element (r * n_pairs + p) * VTX_GENO_PAIR_CLASSES + c of each array of `out`:
 *   sum_alt / sum_ref   the alt / ref counts summed over the entries of row r whose variant has class c under pair p: c = g_a + g_b when
 *                       both donors have a call there, c = 5 when either byte is VTX_GENO_NONE
 *   n_obs               how many of those entries have alt + ref > 0
 * A pair (a, a) therefore carries donor a's one-donor tally on the classes 0, 2, 4, its missing class on 5 and zeros on 1 and 3.  The
 * result is not a function of the one-donor tallies: it needs the joint class of each entry.  The arrays have n_major * n_pairs * 6
 * elements; any pointer may be NULL and is then not written; every element of the others is written, zeros for rows without entries.
 * The contract is vtx_csr_geno_tally's: a context but no run, synchronous on the context's stream, and three checks on the device BEFORE
 * anything is written: the CSR, the table (every byte 0, 1, 2 or VTX_GENO_NONE), and the pairs (a < n_donors and b < n_donors).  A
 * violation returns VTX_E_INVAL (the reason in vtx_strerror; for a pair it names the lowest offending pair index and its two donors),
 * no output byte is written and the context stays usable.  VTX_E_INVAL also for n_donors == 0, n_pairs == 0, a null `out`, a null
 * d_pairs and a null array that is needed (d_geno unless n_minor == 0); VTX_E_UNSUPPORTED for nnz >= 2^32, n_donors >
 * vtx_csr_geno_max() and n_pairs > vtx_csr_geno_pair_max().  Outputs must not overlap inputs.  One GPU.
 * One wavefront walks a row with up to 64 pairs on its lanes and keeps the eighteen numbers of a pair in registers; with more pairs it
 * repeats the row once per 64, which vtx_csr_geno_pair_max() = 64 passes bounds.  No atomics, no zeroing pass, integer additions only:
 * the result is a function of the input alone.  Work space: the checks' flag words only.                                              */
#define VTX_GENO_PAIR_CLASSES 6u       /* dosage 0..4, and 5: either donor without a call */
typedef struct vtx_geno_pair_tally {
    uint64_t *sum_alt, *sum_ref;       /* n_major * n_pairs * 6 elements each */
    uint32_t *n_obs;
} vtx_geno_pair_tally;
uint32_t vtx_csr_geno_pair_max(void);       /* the largest n_pairs accepted: 4096 (64 passes of a wavefront) */
uint32_t vtx_sizeof_geno_pair_tally(void);  /* sizeof(vtx_geno_pair_tally) as the library was built: 24 (the table of vtx_abi_sizes is unchanged) */
int vtx_csr_geno_pair_tally(vtx_ctx* ctx, uint32_t n_major, uint32_t n_minor, uint64_t nnz,
                            const uint64_t* d_indptr, const uint32_t* d_indices,
                            const uint32_t* d_alt, const uint32_t* d_ref,
                            const uint8_t* d_geno, uint32_t n_donors,
                            const uint32_t* d_pairs, uint32_t n_pairs, const vtx_geno_pair_tally* out);

/* ---- CSR x integer tables: the integer part of the models without genotype classes (vartrix_amd/csrc/vtx_csr_dense.hip) ------------------
 * Where the alt probability at a variant is a free parameter per (variant, hypothesis) — clustering without genotypes, an ambient
 * profile, an unequal mixture — the integer part of a likelihood is no tally by class but a sparse-times-dense product:
 *   out[r * n_cols + h] = sum over the entries k of row r of  alt[k] * w_alt[indices[k] * n_cols + h] + ref[k] * w_ref[indices[k] * n_cols + h]
 * d_w_alt and d_w_ref are int32_t[n_minor * n_cols] in device memory, minor-major: element (uint64_t)v * n_cols + h, the columns of one
 * minor index consecutive.  Either table may be NULL and its term is then absent (the same table may so serve as w_alt in one call and
 * as w_ref in the next, without a copy); both NULL is VTX_E_INVAL unless n_minor == 0, where no table has an element.  The sum is
 * COMPUTED MODULO 2^64 and read as two's complement: the counts are zero-extended, the weights sign-extended, the products added in
 * uint64_t.  Wrapping is defined behaviour; the sum is the true sum whenever that fits int64_t.  Any int32_t is a valid weight: the
 * tables are not checked.  d_out has n_major * n_cols elements; every one is written, zeros for rows without entries.
 * The contract is vtx_csr_geno_tally's: ANY CSR in caller-owned device memory (rows in any order inside, duplicate indices allowed:
 * every entry counts), a context but no run, synchronous on the context's stream, and the CSR is checked on the device BEFORE anything
 * is written.  A violation returns VTX_E_INVAL (the reason in vtx_strerror), no output byte is written and the context stays usable.
 * VTX_E_INVAL also for n_cols == 0, a null d_out and a null array that is needed; VTX_E_UNSUPPORTED for nnz >= 2^32 and for n_cols >
 * vtx_csr_dense_max().  Outputs must not overlap inputs.  One GPU.
 * One wavefront walks a row with up to 64 columns on its lanes, one 64-bit sum a lane; with more columns it repeats the row once per
 * 64, which vtx_csr_dense_max() = 16 passes bounds.  No atomics, no zeroing pass, integer arithmetic only: the result is a function of
 * the input alone.  Work space: the check's flag words only.  The call takes no struct: VTX_ABI_VERSION and vtx_abi_sizes are unchanged. */
uint32_t vtx_csr_dense_max(void);    /* the largest n_cols accepted: 1024 (16 passes of a wavefront) */
int vtx_csr_dense_sum(vtx_ctx* ctx, uint32_t n_major, uint32_t n_minor, uint64_t nnz,
                      const uint64_t* d_indptr, const uint32_t* d_indices,
                      const uint32_t* d_alt, const uint32_t* d_ref,
                      const int32_t* d_w_alt, const int32_t* d_w_ref, uint32_t n_cols,
                      int64_t* d_out);

/* Device time of the context's last CSR call that succeeded, in milliseconds, from events on the context's own stream.
 * vtx_device_csr / vtx_csr_transpose: ms[0] the check of the inputs, ms[1] the sort of the positions by column, ms[2] the offsets,
 * ms[3] the placement of the indices and payloads (vtx_device_csr: 1 and 3 are 0).  vtx_csr_row_stats: ms[0] the check, ms[3] the
 * reduction (1 and 2 are 0).  vtx_csr_select_plan / vtx_csr_select: ms[0] the check, ms[1] the scans, ms[2] the offsets and ids, ms[3]
 * the placement (the plan: 2 and 3 are 0).  vtx_csr_group_plan / vtx_csr_group_sum: ms[0] the checks of the CSR and of the labels,
 * ms[1] the count and its scan, ms[3] the fill (2 is 0; the plan: 3 is 0 too).  vtx_csr_geno_tally: ms[0] the checks of the CSR and
 * of the genotype table, ms[3] the tally (1 and 2 are 0).  vtx_csr_geno_pair_tally: ms[0] the checks of the CSR, the table and the
 * pairs, ms[3] the tally (1 and 2 are 0).  vtx_csr_dense_sum: ms[0] the check of the CSR, ms[3] the sum (1 and 2 are 0).  Writes the
 * first n of the four, at most four.                                                                                                  */
int vtx_last_csr_ms(vtx_ctx* ctx, float* ms, uint32_t n);

/* ---- Multi-GPU: one process (one ctx) per GPU, loci sharded over the ranks (src/main.rs:284-291: chunks of loci
 * are independent), and ONE exchange at the end — every rank's triplets travel to rank `dst` over RCCL (xGMI inside
 * a node), concatenated in rank order, which is row order when rank r holds the r-th contiguous range of loci
 * (the merge loop's order, src/main.rs:320-348).
 *   vtx_comm_id      rank 0 only: fills the 128-byte RCCL unique id; the host distributes it to the other ranks by
 *                    its own means (MPI, a socket, a file — it is plain bytes).
 *   vtx_comm_init    every rank, same id: joins the communicator (collective).
 *   vtx_gather_coo   every rank, after its own vtx_run (collective).  The counts go round with one all-gather of a
 *                    (count, status) pair per rank — any rank in error makes EVERY rank return VTX_E_PEER before the data
 *                    exchange, so nobody waits for a peer that left; then each rank sends its (row, col, alt, ref, unk) arrays to `dst`, which
 *                    receives every block at its final offset (grouped point-to-point: no padding, each block crosses
 *                    its own link once) and recomputes the f64 values from the counts (the same arithmetic as
 *                    vtx_run's emit step).  On `dst`, *out holds DEVICE pointers to the gathered arrays (valid until
 *                    the next vtx_gather_coo / vtx_destroy); on the other ranks out->nnz = 0.
 *   vtx_fetch_gathered  `dst` only: copies the gathered triplets to context-owned host memory.
 * librccl is opened on first use (dlopen): a single-GPU process never loads it.                                  */
#define VTX_COMM_ID_BYTES 128
int vtx_comm_id(uint8_t id[VTX_COMM_ID_BYTES]);
int vtx_comm_init(vtx_ctx* ctx, const uint8_t id[VTX_COMM_ID_BYTES], int rank, int world);
int vtx_gather_coo(vtx_ctx* ctx, int dst, vtx_coo* out);
int vtx_fetch_gathered(vtx_ctx* ctx, vtx_coo* out);
/* The number of ranks the communicator itself reports (ncclCommCount) — a cross-check of the launcher's world size. */
int vtx_comm_ranks(vtx_ctx* ctx, int* ranks);
/* A rank whose own work failed after vtx_comm_init (vtx_submit / vtx_run error) calls this INSTEAD of vtx_gather_coo: it takes
 * part in the status round, and every other rank's vtx_gather_coo returns VTX_E_PEER instead of waiting for ever.          */
int vtx_gather_abort(vtx_ctx* ctx);
/* The layout of the exchange as a pure function (no device): offsets[r] = where rank r's counts[r] triplets land, *total =
 * their sum; VTX_E_UNSUPPORTED when the total exceeds 2^32 - 1.  vtx_gather_coo follows exactly this plan.                  */
int vtx_gather_plan(int world, const uint64_t* counts, uint64_t* offsets, uint64_t* total);

int vtx_last_timing(vtx_ctx* ctx, vtx_timing* out);

/* ---- audit / test hooks: none changes a result, none is needed in production --------------------------------------------
 * vtx_set_debug(ctx, VTX_DEBUG_STAGE_TRACE, 0 | 1): the next vtx_run records, one byte per task (task = 2 * record + haplotype,
 *   0 = REF), which stage decided that alignment's score (Scores.ref_score / alt_score, src/main.rs:926-927): a certificate
 *   (no DP cell touched), the full-matrix check of a certificate, or a DP.  vtx_fetch_stage copies the 2 * n_records bytes.
 *   The invariant it lets a test assert over EVERY alignment: a banded score that differs from the full-matrix score was
 *   produced by a DP stage, never by a certificate.
 * vtx_set_debug(ctx, VTX_DEBUG_POISON_SCORES, 1) / (.., VTX_DEBUG_POISON_VALUE, v): every later vtx_run first fills both score
 *   arrays with v, so that a stage that fails to write a task's score cannot hide behind the previous run's value.
 * vtx_debug_bands: the band (banded::Aligner's Band: per column of the DP matrix the row range [lo, hi), columns 0 .. hap_len,
 *   rows 0 .. read_len) band_sweep_kernel builds for n_tasks tasks of the resident batch — lo / hi hold `stride` uint16 per
 *   task (stride >= longest haplotype + 1; empty column: lo 0x7fff, hi 0); status[i] = 0 band written, != 0 declined (the
 *   general kernel takes such a task in vtx_run).  Parity of the BAND, not only of the score it leads to.
 * vtx_debug_tables: the haplotype k-mer tables (the device form of the reference's per-haplotype hash index, bio 0.30.0
 *   sparse::hash_kmers as called from banded::Aligner::local, src/main.rs:898-901) the last banded vtx_run left in global
 *   memory: *bytes = their size (0: that run kept its tables in LDS), min(cap, *bytes) bytes are copied to dst (dst may be
 *   null with cap 0).  Lets a test compare two ways of BUILDING the tables byte for byte (VTX_BAND_TABLES_V1).           */
#define VTX_STAGE_UNKNOWN 0        /* band_run_kernel's / band_pending_kernel's certificate (cert == ub over all pieces: chains over several diagonals) */
#define VTX_STAGE_DIAG_CERT 1      /* band_diag_kernel: cert == ub */
#define VTX_STAGE_REFINE_CERT 2    /* band_refine_kernel: cert == refined ub */
#define VTX_STAGE_FULL_CHECK 3     /* full-matrix score == certificate (cert <= banded <= full); experiment hook VTX_BAND_CHECK only */
#define VTX_STAGE_SWEEP_DP 4       /* band_sweep_kernel's band + band-masked DP */
#define VTX_STAGE_GENERAL_DP 5     /* general band kernel (tasks the sweep declined) + band-masked DP */
#define VTX_STAGE_RUN_DP 6         /* VTX_BAND_LEGACY path: band_run_kernel's staircase + band-masked DP */
#define VTX_STAGE_DIAG_DP 7        /* the certificate stages' one-diagonal band (every off-diagonal match harmless) + band-masked DP */
#define VTX_STAGE_SLOW 8           /* slow_align_kernel (records beyond the fast kernels' limits): exact DP */
#define VTX_STAGE_FULL_DP 9        /* full flavour: the full-matrix DP */
#define VTX_STAGE_BAND_CERT 10     /* band_refine_kernel: cert == the run bound over the pieces trimmed to the one-diagonal band — a bound of the BANDED
                                      score (vtx_band_trim.h): like the DP stages, this one may decide a task whose banded score is below the full one */
#define VTX_STAGE_CORRIDOR_CERT 11 /* band_corridor_kernel (round 6): an exact DP over the cells of the one-diagonal band within 8 diagonals of the main one,
                                      with edges that bound every way around them; decided when the maximum needs none of those edges.  A bound of
                                      the BANDED score as well */
#define VTX_DEBUG_STAGE_TRACE 1
#define VTX_DEBUG_POISON_SCORES 2
#define VTX_DEBUG_POISON_VALUE 3
int vtx_set_debug(vtx_ctx* ctx, int key, int64_t value);
int vtx_fetch_stage(vtx_ctx* ctx, uint8_t* stage);
int vtx_debug_bands(vtx_ctx* ctx, const uint32_t* tasks, uint32_t n_tasks, uint32_t stride, uint16_t* lo, uint16_t* hi, uint8_t* status);
int vtx_debug_tables(vtx_ctx* ctx, void* dst, uint64_t cap, uint64_t* bytes);

/* Number of DP cells the last vtx_run evaluated (sum over records and both
 * haplotypes of rows x columns actually computed) — the roofline numerator.  */
int vtx_last_cells(vtx_ctx* ctx, uint64_t* cells);

/* Message for the last failing call on ctx (ctx may be NULL for create).     */
const char* vtx_strerror(const vtx_ctx* ctx);
const char* vtx_status_name(int status);

/* sizeof() of {vtx_config, vtx_locus, vtx_record, vtx_batch, vtx_coo,
 * vtx_timing, vtx_raw_record, vtx_raw_batch, vtx_raw_stats, vtx_bgzf_block, vtx_bam_interval,
 * vtx_bam_ingest, vtx_ingest_stats, vtx_bam_segment, vtx_bam_segments, vtx_mtx_part, vtx_csr} as compiled into the library,
 * for binding self-checks.  Writes min(n, 17) entries; returns VTX_ABI_VERSION.             */
int vtx_abi_sizes(uint32_t* out, uint32_t n);
/* sizeof(vtx_csr_stats) as compiled into the library.  A call of its own: the table above stays at its 17 entries, which callers
 * already rely on (a caller that asks vtx_abi_sizes for more gets 17).                                                               */
uint32_t vtx_sizeof_csr_stats(void);

#ifdef __cplusplus
}
#endif
#endif /* VTX_H */
