// vtx_ingest.h — internal declarations of the device-side BAM ingest (vtx_ingest.hip), shared with the C-ABI layer (vtx_api.hip).
#ifndef VTX_INGEST_H
#define VTX_INGEST_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vtx.h"
#include "vtx_ingest_plan_core.h"      // vtxg_block, vtxg_segment: the plan in the device's layout, and the host code that makes it
#include "vtx_scan_core.h"

// the read filters of evaluate_alns that need no dictionary (src/main.rs:833-864) + the tag to look for (--bam-tag, :126-129)
typedef vtxs::Filter vtxg_filter;      // { n_ref, min_mapq, primary_only, no_duplicates, bam_tag }: vtx_scan_core.h, where the scan reads it
// per BAM record with at least one surviving pair: where its tags lie (relative to the record body) and their lengths
struct vtxg_recinfo { uint32_t bc_rel, umi_rel, lens; };

// counters[]: 0 num_reads, 1 num_low_mapq, 2 num_non_primary, 3 num_duplicates, 4 num_not_useful, 5 reads without a usable barcode tag
// (Metrics, src/main.rs:449-459), 6 read bases kept (padded to even), 7 tag bytes kept, 8 surviving (read, locus) pairs
#define VTXG_N_COUNTERS 9
// err[0] bits: 1 << vtxi::Status of a block that did not inflate (bits 1..8); err[1]: the first such block
#define VTXG_ERR_CHAIN (1u << 16)      // a record chain did not land on the next seed / ran off the data
#define VTXG_ERR_RECORD (1u << 17)     // a record whose fields run past its block_size
#define VTXG_ERR_SEG_END (1u << 18)    // a segment's end is not proven: the record there may still overlap its loci (err[2]: how many)
#define VTXG_ERR_CRC (1u << 19)        // a block whose inflated bytes do not have the CRC32 of its trailer (err[1]: the first; only when every block inflated)

extern "C" {
hipError_t vtxg_inflate(const uint8_t* comp, const vtxg_block* blocks, uint32_t n_blocks, uint8_t* out, uint32_t* err, uint32_t* status, uint32_t b_base, hipStream_t s);
// CRC32 of the inflated bytes of every block (data + uoff, isize) against the four bytes at comp + coff + clen; comp == nullptr: no
// comparison.  crc_out (optional): the computed values.  width: the slicing width, 4 / 8 / 16 (VTXG_CRC_WIDTH).  data: 16-byte aligned.
#define VTXG_CRC_WIDTH 16
hipError_t vtxg_crc32(const uint8_t* comp, const vtxg_block* blocks, uint32_t n_blocks, const uint8_t* data, uint32_t* err, uint32_t* crc_out,
                      uint32_t b_base, int width, hipStream_t s);
hipError_t vtxg_chain(const uint8_t* data, uint64_t total, const uint64_t* seeds, uint32_t n_seeds, uint64_t end_upos, uint32_t* cnt,
                      const uint32_t* off, uint64_t* rec_upos, uint32_t* err, hipStream_t s);
hipError_t vtxg_chain_segments(const uint8_t* data, const uint64_t* seeds, uint32_t n_seeds, const uint32_t* seed_seg, const vtxg_segment* segs,
                               uint32_t* cnt, const uint32_t* off, uint64_t* rec_upos, uint32_t* err, hipStream_t s);
hipError_t vtxg_scan(int emit, const uint8_t* data, const uint64_t* rec_upos, uint32_t n_rec, vtxg_filter f, const int32_t* iv_start,
                     const int32_t* iv_end, const uint32_t* iv_locus, const uint32_t* tid_begin, const int32_t* tid_span,
                     uint32_t* n_hit, uint32_t* read_sz, uint32_t* tag_sz, vtxg_recinfo* info, const uint32_t* hit_scan,
                     const uint32_t* read_scan, const uint32_t* tag_scan, vtx_raw_record* raw, uint32_t* raw_locus, uint8_t* tags,
                     uint8_t* reads_packed, unsigned long long* counters, uint32_t* err, hipStream_t s);
// Matrix-Market lines of n triplets: byte length per line, sum of the values; then the text at the inclusive scan `end` of the lengths.
// real = 0: integral values only (0 + flag when a value is not a non-negative integer below 2^32).  real = 1: any value in the domain
// of vtx_f64_text.h (fractions, NaN, -0: shortest round-trip digits); 0 + flag outside it; a line is at most VTXG_MTX_LINE_MAX bytes.
#define VTXG_MTX_LINE_MAX 54u      /* "4294967296 4294967296 " + vtxt::MAX_LEN + "\n" (static_assert in vtx_ingest.hip) */
hipError_t vtxg_mtx_len(const uint32_t* row, const uint32_t* col, const double* val, uint32_t n, uint32_t* len, double* sum, uint32_t* flag, int real, hipStream_t s);
hipError_t vtxg_mtx_text(const uint32_t* row, const uint32_t* col, const double* val, uint32_t n, const uint32_t* end, uint8_t* text, int real, hipStream_t s);
// vtx_deflate.hip: `total` bytes of text (4-byte aligned) in n_chunks = ceil(total / vtxd::CHUNK) chunks -> one BGZF member per chunk at
// slots + ch * vtxd::SLOT (4-byte aligned), its size in sizes[ch]; tok: vtxg_deflate_grid(n_chunks) * vtxd::CHUNK words of work space.
// Then, with `end` the inclusive scan of the sizes, the members back to back at out (end[n_chunks - 1] bytes).
uint32_t vtxg_deflate_grid(uint32_t n_chunks);
hipError_t vtxg_mtx_deflate(const uint8_t* text, uint64_t total, uint32_t n_chunks, uint8_t* slots, uint32_t* sizes, uint32_t* tok, hipStream_t s);
hipError_t vtxg_mtx_gz_compact(const uint8_t* slots, const uint32_t* sizes, const uint32_t* end, uint32_t n_chunks, uint8_t* out, hipStream_t s);
}
#endif
