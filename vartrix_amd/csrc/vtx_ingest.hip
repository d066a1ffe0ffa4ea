// vtx_ingest.hip — the BAM ingest on the device (round 6): BGZF inflate, record split, and the fetch + filter half of evaluate_alns.
//
// What it replaces (reference 10XGenomics/vartrix v1.1.22): `bam.fetch(tid, start, end)` + `bam.records()` per locus
// (src/main.rs:822-830; rust-htslib -> htslib bgzf_read -> zlib below them), the read filters in their order with the Metrics
// counters (:831-864), useful_alignment (:790-806), get_cell_barcode / get_umi as tag BYTES (:737-757, :867-888 — the in-list test,
// the UB test, the UMI grouping and the sort by cell follow in vtx_prep.hip, as for vtx_submit_raw) and rec.seq() (:896).
// In rounds 1-5 this was host code (host/vtx_host.cpp: sixteen threads, 1.6 s of a 2.4 s run at config-3 scale, the device 1 % of it).
//
// Pipeline (all on the context's stream; HBM-bound byte work, no MFMA, no host round trip between the kernels):
//   bgzf_inflate_kernel   one LANE per BGZF block (vtx_inflate_core.h: a flat state machine, Huffman codes in registers, the symbol
//                         lists in LDS), every block of the file in flight at once; 0.9 GB -> 3 GB
//   bam_chain_kernel x2   record boundaries: block_size chains are serial, but the .bai's linear index names a record start every
//                         16 kb of genome — one lane per seed walks to the next seed (count, scan, fill)
//   bam_scan_kernel       one lane per BAM record: fixed fields, end position from the CIGAR, the loci it overlaps (binary search in
//                         the contig's sorted intervals), the filters per (read, locus) pair in the reference's order with its
//                         counters, the barcode / UB tag bytes; per record: surviving pairs, read and tag bytes to keep
//   scans                 pair offsets, read-arena and tag-arena offsets (BAM order: the layout the host packer produces)
//   bam_emit_kernel       raw records (vtx_raw_record + locus) per surviving pair, packed bases and tag bytes copied once per read
// and then vtx_prep.hip's barcode lookup / UMI grouping / sort, exactly as after vtx_submit_raw.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "vtx_device.h"
#include "vtx_ingest.h"
#include "vtx_inflate_core.h"
#include "vtx_crc32_core.h"
#include "vtx_f64_text.h"
#include "vtx_scan_core.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------
// BGZF inflate: one lane per block.  LDS: 444 bytes per lane, lane-interleaved (28.4 KB per wavefront: five per CU = 81 920 lanes
// resident on 256 CUs; the first cut kept 16-bit symbols: 47.6 KB, three per CU).
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void bgzf_inflate_kernel(const uint8_t* __restrict__ comp, const vtxg_block* __restrict__ blocks,
                                                          uint32_t n_blocks, uint8_t* __restrict__ out, uint32_t* __restrict__ err,
                                                          uint32_t* __restrict__ status, uint32_t b_base) {
    __shared__ uint8_t s_bytes[vtxi::BYTES * 64];
    __shared__ uint32_t s_hi[vtxi::HI_WORDS * 64];
    __shared__ uint16_t s_cnt[vtxi::CNT_WORDS * 64];
    const vtxi::Scratch sc{s_bytes + threadIdx.x, s_hi + threadIdx.x, s_cnt + threadIdx.x, 64};
    for (uint32_t b = blockIdx.x * 64 + threadIdx.x; b < n_blocks; b += gridDim.x * 64) {
        const vtxg_block B = blocks[b];
        uint32_t st = vtxi::ST_OK;
        if (B.isize) st = vtxi::inflate_block(comp + B.coff, B.clen, out + B.uoff, B.isize, sc, nullptr);
        if (st != vtxi::ST_OK) { atomicMin(&err[1], b_base + b); atomicOr(&err[0], 1u << st); }     // (b_base: the launch covers blocks [b_base, b_base + n_blocks) of the ingest)
        if (status) status[b] = st;                         // (vtx_debug_inflate: the verdict per block)
    }
}

using vtxs::ld32;
using vtxs::ld64;

// ---------------------------------------------------------------------------------------------------------------------------
// BGZF CRC32: one wavefront per block, four per workgroup, grid-stride over the blocks.  The workgroup fills the W slicing tables in
// LDS once (W KiB); a lane then needs W aligned bytes and W table reads per step, and a load instruction of the wavefront covers 64 W
// consecutive bytes (vtx_crc32_core.h has the cut of a block and why the pieces are interleaved).  The expected value is the four
// bytes behind the block's payload in the compressed buffer (comp == nullptr: vtx_debug_crc32, nothing to compare with).  Blocks of
// an ingest in which some block did not inflate are not looked at: err[1] then names that block, and its message comes first.
// `data` is 16-byte aligned (a device allocation's start) and readable from (uoff & ~15) on.
// ---------------------------------------------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(256) void bgzf_crc32_kernel(const uint8_t* __restrict__ comp, const vtxg_block* __restrict__ blocks, uint32_t n_blocks,
                                                         const uint8_t* __restrict__ data, uint32_t* __restrict__ err,
                                                         uint32_t* __restrict__ crc_out, uint32_t b_base) {
    __shared__ uint32_t s_tab[vtxc::TABLE_WORDS(W)];
    if (comp && (err[0] & 0x1ffu)) return;                  // (written by the inflate kernel in front of this one: the same for every lane)
    for (uint32_t i = threadIdx.x; i < (uint32_t)vtxc::TABLE_WORDS(W); i += 256) s_tab[i] = vtxc::table_entry<W>(i);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6); b < n_blocks; b += gridDim.x * 4) {
        const vtxg_block B = blocks[b];
        const uint64_t s = B.uoff, e = B.uoff + B.isize;
        const vtxc::Cut c = vtxc::cut_block<W>(s, e);
        uint32_t v = vtxc::lane_pieces<W>(data, c, lane, s_tab);
        VTXI_UNROLL
        for (int k = 0; k < 6; ++k) {
            const uint32_t partner = __shfl_xor(v, 1 << k);
            if (lane & (1u << k)) v = vtxc::lane_join<W>(partner, v, k);
        }
        const uint32_t crc = vtxc::finish_block<W>(__shfl(v, 63), data, c, s, e);      // (wavefront-uniform: every lane holds it)
        if (lane == 0) {
            if (crc_out) crc_out[b] = crc;
            if (comp && crc != ld32(comp + B.coff + B.clen)) { atomicMin(&err[1], b_base + b); atomicOr(&err[0], VTXG_ERR_CRC); }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Record boundaries.  Seed i (a record start the .bai names) .. seed i + 1: one lane hops from block_size to block_size.
// off == nullptr: count; else: write the offsets.  A chain that does not land on the next seed means the index and the file
// disagree (or a record is malformed): the host packer takes over.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void bam_chain_kernel(const uint8_t* __restrict__ data, uint64_t total, const uint64_t* __restrict__ seeds,
                                                       uint32_t n_seeds, uint64_t end_upos, uint32_t* __restrict__ cnt,
                                                       const uint32_t* __restrict__ off, uint64_t* __restrict__ rec_upos,
                                                       uint32_t* __restrict__ err) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_seeds) return;
    uint64_t p = seeds[i];
    const uint64_t stop = i + 1 < n_seeds ? seeds[i + 1] : end_upos;
    uint32_t k = 0;
    const uint32_t base = off ? (i ? off[i - 1] : 0u) : 0u;      // (off: INCLUSIVE scan of the counts)
    bool bad = false;
    while (p < stop) {
        const uint64_t at = p;
        if (!vtxs::chain_step(data, p, total)) { bad = true; break; }
        if (off) rec_upos[base + k] = at;
        ++k;
    }
    if (bad || p != stop) atomicOr(&err[0], VTXG_ERR_CHAIN);
    if (!off) cnt[i] = k;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Record boundaries of a SEGMENTED plan (sparse loci: the inflated stream is the concatenation of several stretches of the file).
// The same walk, but a lane knows its segment: it stops at the next seed of ITS segment or, as the segment's last lane, at the
// segment's stated end, and reads nothing outside [S.ubegin, S.ulimit) — a record cut by the end of the segment's blocks is an error
// of the plan (VTXG_ERR_CHAIN), not something to skip.  The last lane then PROVES the end: nothing at or behind it is looked at, so
// the record that starts there must lie behind every locus of the segment ((tid, pos) beyond (end_tid, end_pos); the file is
// coordinate-sorted; tid -1, the unplaced reads at the end of a file, compares as the largest).  Its 12 bytes are inside the
// segment's blocks (the plan adds the block that holds them).  err[2] counts the segments whose end does not hold.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void bam_chain_seg_kernel(const uint8_t* __restrict__ data, const uint64_t* __restrict__ seeds,
                                                           uint32_t n_seeds, const uint32_t* __restrict__ seed_seg,
                                                           const vtxg_segment* __restrict__ segs, uint32_t* __restrict__ cnt,
                                                           const uint32_t* __restrict__ off, uint64_t* __restrict__ rec_upos,
                                                           uint32_t* __restrict__ err) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_seeds) return;
    const vtxg_segment S = segs[seed_seg[i]];
    const bool last = i + 1 == S.seed_end;
    uint64_t p = seeds[i];
    const uint64_t stop = last ? S.end_upos : seeds[i + 1];
    uint32_t k = 0;
    const uint32_t base = off ? (i ? off[i - 1] : 0u) : 0u;      // (off: INCLUSIVE scan of the counts)
    bool bad = p < S.ubegin || stop > S.ulimit;
    while (!bad && p < stop) {
        const uint64_t at = p;
        if (!vtxs::chain_step(data, p, S.ulimit)) { bad = true; break; }
        if (off) rec_upos[base + k] = at;
        ++k;
    }
    if (bad || p != stop) atomicOr(&err[0], VTXG_ERR_CHAIN);
    else if (last && !off && !(S.flags & VTX_SEGMENT_TO_EOF)) {
        bool proven = false;
        if (stop + 12 <= S.ulimit) {
            const int32_t tid = (int32_t)ld32(data + stop + 4), pos = (int32_t)ld32(data + stop + 8);
            proven = (uint32_t)tid > (uint32_t)S.end_tid || (tid == S.end_tid && pos >= S.end_pos);
        }
        if (!proven) { atomicOr(&err[0], VTXG_ERR_SEG_END); atomicAdd(&err[2], 1u); }
    }
    if (!off) cnt[i] = k;
}

// One lane per BAM record.  EMIT = false: counts (pairs that survive, metrics, the bytes to keep); EMIT = true: the raw records.
template <bool EMIT>
__global__ __launch_bounds__(256) void bam_scan_kernel(const uint8_t* __restrict__ data, const uint64_t* __restrict__ rec_upos,
                                                       uint32_t n_rec, vtxg_filter f, const int32_t* __restrict__ iv_start,
                                                       const int32_t* __restrict__ iv_end, const uint32_t* __restrict__ iv_locus,
                                                       const uint32_t* __restrict__ tid_begin, const int32_t* __restrict__ tid_span,
                                                       uint32_t* __restrict__ n_hit, uint32_t* __restrict__ read_sz,
                                                       uint32_t* __restrict__ tag_sz, vtxg_recinfo* __restrict__ info,
                                                       const uint32_t* __restrict__ hit_scan, const uint32_t* __restrict__ read_scan,
                                                       const uint32_t* __restrict__ tag_scan, vtx_raw_record* __restrict__ raw,
                                                       uint32_t* __restrict__ raw_locus, uint8_t* __restrict__ tags,
                                                       uint8_t* __restrict__ reads_packed, unsigned long long* __restrict__ counters,
                                                       uint32_t* __restrict__ err) {
    __shared__ unsigned long long s_cnt[VTXG_N_COUNTERS];
    if (!EMIT) {
        if (threadIdx.x < VTXG_N_COUNTERS) s_cnt[threadIdx.x] = 0;
        __syncthreads();
    }
    for (uint32_t rix = blockIdx.x * 256 + threadIdx.x; rix < n_rec; rix += gridDim.x * 256) {
        if (EMIT && n_hit[rix] == 0) continue;
        const uint64_t p = rec_upos[rix];
        const vtxs::RecView v = vtxs::view_record(data, p);
        vtxs::Verdict V;
        uint32_t h_base = 0, roff = 0, toff = 0;
        if (EMIT) {
            h_base = rix ? hit_scan[rix - 1] : 0u;
            roff = rix ? read_scan[rix - 1] : 0u;
            toff = rix ? tag_scan[rix - 1] : 0u;
            const vtxg_recinfo I = info[rix];
            V.bc_rel = I.bc_rel; V.umi_rel = I.umi_rel; V.bc_len = I.lens & 0xffffu; V.umi_len = I.lens >> 16;
        }
        if (v.malformed) { if (!EMIT) atomicOr(&err[0], VTXG_ERR_RECORD); }
        else
            vtxs::scan_pairs<!EMIT>(v, f, iv_start, iv_end, tid_begin, tid_span, V, [&](uint32_t k, uint32_t outcome, uint32_t hit) {
                if (EMIT && outcome == vtxs::PAIR_KEPT) {
                    vtx_raw_record rr;
                    rr.read_off = roff; rr.read_len = v.l_seq;
                    rr.bc_off = toff; rr.umi_off = V.umi_len != VTX_TAG_MISSING ? toff + V.bc_len : 0u;
                    rr.bc_len = (uint16_t)V.bc_len; rr.umi_len = (uint16_t)V.umi_len;
                    raw[h_base + hit] = rr;
                    raw_locus[h_base + hit] = iv_locus[k];
                }
            });
        const uint32_t hits = V.hits, bc_len = V.bc_len, umi_len = V.umi_len, bc_rel = V.bc_rel, umi_rel = V.umi_rel;
        const uint32_t m_reads = V.reads, m_mapq = V.low_mapq, m_prim = V.non_primary, m_dup = V.duplicate, m_useful = V.not_useful, m_nobc = V.no_barcode;
        if (!EMIT) {
            n_hit[rix] = hits;
            read_sz[rix] = hits ? (v.l_seq + 1u) & ~1u : 0u;           // bases; every read starts at an even one (two per byte)
            tag_sz[rix] = hits ? bc_len + (umi_len != VTX_TAG_MISSING ? umi_len : 0u) : 0u;
            if (hits) info[rix] = vtxg_recinfo{bc_rel, umi_rel, bc_len | (umi_len << 16)};
            if (hits && v.l_seq > 0x7fffffffu) atomicOr(&err[0], VTXG_ERR_RECORD);
            if (m_reads) atomicAdd(&s_cnt[0], (unsigned long long)m_reads);
            if (m_mapq) atomicAdd(&s_cnt[1], (unsigned long long)m_mapq);
            if (m_prim) atomicAdd(&s_cnt[2], (unsigned long long)m_prim);
            if (m_dup) atomicAdd(&s_cnt[3], (unsigned long long)m_dup);
            if (m_useful) atomicAdd(&s_cnt[4], (unsigned long long)m_useful);
            if (m_nobc) atomicAdd(&s_cnt[5], (unsigned long long)m_nobc);
            if (hits) { atomicAdd(&s_cnt[6], (unsigned long long)read_sz[rix]); atomicAdd(&s_cnt[7], (unsigned long long)tag_sz[rix]); atomicAdd(&s_cnt[8], (unsigned long long)hits); }
        } else if (hits) {
            // the read's packed bases and its tag bytes, once per read (its pairs share them): exact byte counts — the neighbours
            // belong to other lanes
            uint8_t* d = tags + toff;
            const uint8_t* s = v.r + bc_rel;
            for (uint32_t i = 0; i < bc_len; ++i) d[i] = s[i];
            if (umi_len != VTX_TAG_MISSING) { d += bc_len; s = v.r + umi_rel; for (uint32_t i = 0; i < umi_len; ++i) d[i] = s[i]; }
            const uint32_t nb = (v.l_seq + 1u) >> 1;
            d = reads_packed + (roff >> 1);
            s = v.sq;
            uint32_t i = 0;
            for (; i + 8 <= nb; i += 8) { const uint64_t w = ld64(s + i); __builtin_memcpy(d + i, &w, 8); }
            for (; i < nb; ++i) d[i] = s[i];
            // (an odd read's last low nibble travels as the BAM holds it, like the host packer's memcpy: it is never read)
        }
    }
    if (!EMIT) {
        __syncthreads();
        if (threadIdx.x < VTXG_N_COUNTERS && s_cnt[threadIdx.x]) atomicAdd(&counters[threadIdx.x], s_cnt[threadIdx.x]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Matrix-Market text of resident triplets (sprs::io::write_matrix_market, src/main.rs:381-389): "row+1 col+1 value\n" per triplet,
// Rust `{}` of an f64 that holds a non-negative integer = its decimal digits (consensus 1 / 2 / 3, coverage counts).  Any other
// value (alt_frac's fractions, NaN) sets the flag: the host formatter (shortest round-trip digits, vtxh_write_mtx) takes over.
// REAL (vtx_write_mtx_f64): such a value is formatted too, by vtx_f64_text.h (shortest round-trip digits, positional; its domain covers
// everything alt_frac produces), and only a value outside that domain sets the flag.  The integral test comes first and keeps its
// digits; -0 ("-0" in Rust) is not integral there.  The sum takes every value of the domain as it is: one NaN makes it NaN.
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ndigits(uint32_t v) {
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u
         : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
__device__ __forceinline__ uint8_t* put_u32(uint8_t* p, uint32_t v, uint32_t nd) {      // nd = ndigits(v); returns the end
    for (uint32_t i = nd; i-- > 0;) { p[i] = (uint8_t)('0' + v % 10u); v /= 10u; }
    return p + nd;
}
static_assert(10 + 1 + 10 + 1 + vtxt::MAX_LEN + 1 == VTXG_MTX_LINE_MAX, "longest Matrix-Market line");
template <bool REAL>
__global__ __launch_bounds__(256) void mtx_len_kernel(const uint32_t* __restrict__ row, const uint32_t* __restrict__ col,
                                                      const double* __restrict__ val, uint32_t n, uint32_t* __restrict__ len,
                                                      double* __restrict__ sum, uint32_t* __restrict__ flag) {
    __shared__ double s_sum[4];
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    double v = 0.0;
    if (k < n) {
        v = val[k];
        const bool integral = v >= 0.0 && v < 4294967296.0 && v == (double)(uint32_t)v;      // (false for NaN)
        if (REAL) {
            const uint32_t nv = integral && !__builtin_signbit(v) ? ndigits((uint32_t)v) : vtxt::f64_len(v);
            if (!nv) { atomicOr(flag, 1u); v = 0.0; len[k] = 0; }
            else len[k] = ndigits(row[k] + 1u) + ndigits(col[k] + 1u) + nv + 3u;
        }
        else if (!integral) { atomicOr(flag, 1u); v = 0.0; len[k] = 0; }
        else len[k] = ndigits(row[k] + 1u) + ndigits(col[k] + 1u) + ndigits((uint32_t)v) + 3u;
    }
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) { const double t = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]; if (t != 0.0) atomicAdd(sum, t); }
}
template <bool REAL>
__global__ __launch_bounds__(256) void mtx_text_kernel(const uint32_t* __restrict__ row, const uint32_t* __restrict__ col,
                                                       const double* __restrict__ val, uint32_t n, const uint32_t* __restrict__ end,
                                                       uint8_t* __restrict__ text) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    if (!REAL) {
        const uint32_t r = row[k] + 1u, c = col[k] + 1u, v = (uint32_t)val[k];
        uint8_t* p = text + (k ? end[k - 1] : 0u);
        p = put_u32(p, r, ndigits(r)); *p++ = ' ';
        p = put_u32(p, c, ndigits(c)); *p++ = ' ';
        p = put_u32(p, v, ndigits(v)); *p = '\n';
    } else {
        const uint32_t beg = k ? end[k - 1] : 0u;
        if (end[k] == beg) return;                          // outside the formatter's domain: no line (the caller has seen the flag)
        const uint32_t r = row[k] + 1u, c = col[k] + 1u;
        const double d = val[k];
        uint8_t* p = text + beg;
        p = put_u32(p, r, ndigits(r)); *p++ = ' ';
        p = put_u32(p, c, ndigits(c)); *p++ = ' ';
        if (d >= 0.0 && d < 4294967296.0 && d == (double)(uint32_t)d && !__builtin_signbit(d)) p = put_u32(p, (uint32_t)d, ndigits((uint32_t)d));
        else p = vtxt::f64_put(p, d);
        *p = '\n';
    }
}

}  // namespace

extern "C" {

hipError_t vtxg_inflate(const uint8_t* comp, const vtxg_block* blocks, uint32_t n_blocks, uint8_t* out, uint32_t* err, uint32_t* status, uint32_t b_base, hipStream_t s) {
    if (!n_blocks) return hipSuccess;
    const uint32_t wgs = std::min<uint32_t>((n_blocks + 63) / 64, 256u * 5u);
    hipLaunchKernelGGL(bgzf_inflate_kernel, dim3(wgs), dim3(64), 0, s, comp, blocks, n_blocks, out, err, status, b_base);
    return hipGetLastError();
}

hipError_t vtxg_crc32(const uint8_t* comp, const vtxg_block* blocks, uint32_t n_blocks, const uint8_t* data, uint32_t* err, uint32_t* crc_out,
                      uint32_t b_base, int width, hipStream_t s) {
    if (!n_blocks) return hipSuccess;
    if ((uintptr_t)data & 15u) return hipErrorInvalidValue;
    // workgroups: all blocks at once up to what 256 CUs hold (the tables cost W KiB of a CU's 160: eight workgroups of four wavefronts fit beside them)
    const dim3 wgs(std::min<uint32_t>((n_blocks + 3) / 4, 256u * 8u)), wg(256);
    switch (width) {
    case 4: hipLaunchKernelGGL(bgzf_crc32_kernel<4>, wgs, wg, 0, s, comp, blocks, n_blocks, data, err, crc_out, b_base); break;
    case 8: hipLaunchKernelGGL(bgzf_crc32_kernel<8>, wgs, wg, 0, s, comp, blocks, n_blocks, data, err, crc_out, b_base); break;
    case 16: hipLaunchKernelGGL(bgzf_crc32_kernel<16>, wgs, wg, 0, s, comp, blocks, n_blocks, data, err, crc_out, b_base); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t vtxg_chain_segments(const uint8_t* data, const uint64_t* seeds, uint32_t n_seeds, const uint32_t* seed_seg, const vtxg_segment* segs,
                               uint32_t* cnt, const uint32_t* off, uint64_t* rec_upos, uint32_t* err, hipStream_t s) {
    if (!n_seeds) return hipSuccess;
    hipLaunchKernelGGL(bam_chain_seg_kernel, dim3((n_seeds + 63) / 64), dim3(64), 0, s, data, seeds, n_seeds, seed_seg, segs, cnt, off, rec_upos, err);
    return hipGetLastError();
}

hipError_t vtxg_chain(const uint8_t* data, uint64_t total, const uint64_t* seeds, uint32_t n_seeds, uint64_t end_upos, uint32_t* cnt,
                      const uint32_t* off, uint64_t* rec_upos, uint32_t* err, hipStream_t s) {
    if (!n_seeds) return hipSuccess;
    hipLaunchKernelGGL(bam_chain_kernel, dim3((n_seeds + 63) / 64), dim3(64), 0, s, data, total, seeds, n_seeds, end_upos, cnt, off, rec_upos, err);
    return hipGetLastError();
}

hipError_t vtxg_scan(int emit, const uint8_t* data, const uint64_t* rec_upos, uint32_t n_rec, vtxg_filter f, const int32_t* iv_start,
                     const int32_t* iv_end, const uint32_t* iv_locus, const uint32_t* tid_begin, const int32_t* tid_span,
                     uint32_t* n_hit, uint32_t* read_sz, uint32_t* tag_sz, vtxg_recinfo* info, const uint32_t* hit_scan,
                     const uint32_t* read_scan, const uint32_t* tag_scan, vtx_raw_record* raw, uint32_t* raw_locus, uint8_t* tags,
                     uint8_t* reads_packed, unsigned long long* counters, uint32_t* err, hipStream_t s) {
    if (!n_rec) return hipSuccess;
    const uint32_t wgs = std::min<uint32_t>((n_rec + 255) / 256, 256u * 32u);
    if (emit)
        hipLaunchKernelGGL(bam_scan_kernel<true>, dim3(wgs), dim3(256), 0, s, data, rec_upos, n_rec, f, iv_start, iv_end, iv_locus, tid_begin,
                           tid_span, n_hit, read_sz, tag_sz, info, hit_scan, read_scan, tag_scan, raw, raw_locus, tags, reads_packed, counters, err);
    else
        hipLaunchKernelGGL(bam_scan_kernel<false>, dim3(wgs), dim3(256), 0, s, data, rec_upos, n_rec, f, iv_start, iv_end, iv_locus, tid_begin,
                           tid_span, n_hit, read_sz, tag_sz, info, hit_scan, read_scan, tag_scan, raw, raw_locus, tags, reads_packed, counters, err);
    return hipGetLastError();
}

hipError_t vtxg_mtx_len(const uint32_t* row, const uint32_t* col, const double* val, uint32_t n, uint32_t* len, double* sum, uint32_t* flag, int real, hipStream_t s) {
    if (!n) return hipSuccess;
    if (real) hipLaunchKernelGGL(mtx_len_kernel<true>, dim3((n + 255) / 256), dim3(256), 0, s, row, col, val, n, len, sum, flag);
    else hipLaunchKernelGGL(mtx_len_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, s, row, col, val, n, len, sum, flag);
    return hipGetLastError();
}
hipError_t vtxg_mtx_text(const uint32_t* row, const uint32_t* col, const double* val, uint32_t n, const uint32_t* end, uint8_t* text, int real, hipStream_t s) {
    if (!n) return hipSuccess;
    if (real) hipLaunchKernelGGL(mtx_text_kernel<true>, dim3((n + 255) / 256), dim3(256), 0, s, row, col, val, n, end, text);
    else hipLaunchKernelGGL(mtx_text_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, s, row, col, val, n, end, text);
    return hipGetLastError();
}

}  // extern "C"
