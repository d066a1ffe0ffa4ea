// vtx_ingest_plan_core.h — the HOST half of the device BAM ingest (vtx_submit_bam / vtx_submit_bam_segments, vtx_api.hip): the checks
// of a caller's plan — the API's guard in front of kernels that trust the plan — and its rewrite into the device's own layout.  Pure
// arithmetic on the caller's arrays: plain C++17, no HIP, no context.  Compiles for the host alone (tests/ingestplancore/: against a
// model written from include/vtx.h, every reject, and a stand-alone program under AddressSanitizer / UBSan; CPU suite).
//
// Every comparison of caller-supplied 64-bit offsets is written so that it cannot wrap: `a + b > limit` is `a > limit || b > limit - a`.
#ifndef VTX_INGEST_PLAN_CORE_H
#define VTX_INGEST_PLAN_CORE_H

#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/vtx.h"

// a BGZF block on the device: offsets into the uploaded compressed range / the inflated buffer
struct vtxg_block { uint64_t coff, uoff; uint32_t clen, isize; };
// a segment of a segmented plan on the device: its stretch [ubegin, ulimit) of the concatenated inflated stream, where its last chain
// lands, one past its last seed, and what the record at end_upos must lie beyond (vtx_bam_segment)
struct vtxg_segment { uint64_t ubegin, ulimit, end_upos; uint32_t seed_end; int32_t end_tid, end_pos; uint32_t flags; };

namespace vtxp {

// a block's trailer (CRC32, ISIZE) follows its payload, and bgzf_crc32_kernel reads the CRC32 of every block: the 8 bytes behind a
// stretch of blocks travel with it
constexpr uint64_t kTrailer = 8;

// The intervals as the scan reads them, five arrays in one allocation of words(ni, nref) 32-bit words: start[ni], end[ni], locus[ni],
// tid_begin[nref + 1], tid_span[nref].  ONE definition of that layout: the host fills it through these accessors (layout(), below), the
// device side reads it through the same ones over the uploaded copy.
struct IntervalArrays {
    uint32_t* base;
    uint32_t ni, nref;
    static size_t words(uint32_t ni, uint32_t nref) { return (size_t)ni * 3 + ((size_t)nref + 1) + nref; }
    int32_t* start() const { return (int32_t*)base; }
    int32_t* end() const { return (int32_t*)base + ni; }
    uint32_t* locus() const { return base + 2 * (size_t)ni; }
    uint32_t* tid_begin() const { return base + 3 * (size_t)ni; }
    int32_t* tid_span() const { return (int32_t*)(base + 3 * (size_t)ni + nref + 1); }
};

// bytes [file_off, file_off + bytes) of the file land at dst_off of the compact device buffer (segmented plans; back to back)
struct Piece { uint64_t file_off, dst_off, bytes; };

// A plan in the device's layout.
struct Layout {
    std::vector<vtxg_block> blocks;     // coff relative to `lo` (contiguous) or to the compact buffer the pieces are gathered into (segmented)
    std::vector<vtxg_segment> segs;     // segmented only: the segment table ...
    std::vector<uint32_t> seed_seg;     // ... and every seed's segment
    std::vector<Piece> pieces;          // ... and what travels: per segment [first.coff, last.coff + clen + kTrailer)
    std::vector<uint32_t> iv;           // the packed interval array
    uint64_t lo = 0, hi = 0;            // the blocks' payloads span [lo, hi) of the file
    uint64_t utotal = 0;                // inflated bytes of all blocks
    uint64_t comp_bytes = 0;            // bytes that travel: hi - lo + kTrailer, or the sum of the pieces
    uint64_t end_upos = 0;              // the plan's, clamped to utotal (contiguous plans: no record at or beyond it is looked at)
    IntervalArrays intervals(uint32_t ni, uint32_t nref) { return IntervalArrays{iv.data(), ni, nref}; }
};

#define VTXP_REJECT(code, ...) do { snprintf(why, cap, __VA_ARGS__); return (code); } while (0)

// First: are the arrays there at all, and is the hap arena one the 32-bit offsets of vtx_locus can address.  (The loci's own check,
// check_loci_haps, sits between this and layout() in today's order of checks and is shared with vtx_submit_raw: it stays in vtx_api.hip.)
inline int check_arrays(const vtx_bam_ingest& g, char* why, size_t cap) {
    if ((g.n_blocks && (!g.blocks || !g.file)) || (g.n_loci && !g.loci) || (g.hap_bytes && !g.hap_arena) || (g.n_seeds && !g.seeds) ||
        (g.n_intervals && !g.intervals) || !g.tid_begin || (g.n_ref && !g.tid_max_span))
        VTXP_REJECT(VTX_E_INVAL, "vtx_submit_bam: null array with non-zero count");
    if (g.hap_bytes > 0xffffffffull) VTXP_REJECT(VTX_E_UNSUPPORTED, "vtx_submit_bam: hap arena above 4 GiB");
    return VTX_OK;
}

// tid_begin tiles the intervals; per contig they are sorted by start, name a locus and are no longer than the contig's stated span
inline int check_intervals(const vtx_bam_ingest& g, char* why, size_t cap) {
    const uint32_t ni = g.n_intervals;
    if (g.tid_begin[0] != 0 || g.tid_begin[g.n_ref] != ni) VTXP_REJECT(VTX_E_INVAL, "vtx_submit_bam: tid_begin does not cover the intervals");
    for (uint32_t t = 0; t < g.n_ref; ++t) {
        if (g.tid_begin[t] > g.tid_begin[t + 1]) VTXP_REJECT(VTX_E_INVAL, "vtx_submit_bam: tid_begin not ascending at %u", t);
        // (an entry above n_intervals comes back down to it later and is rejected there as not ascending: nothing is read beyond the array)
        for (uint32_t k = g.tid_begin[t]; k < std::min(g.tid_begin[t + 1], ni); ++k) {
            const vtx_bam_interval& I = g.intervals[k];
            if (I.locus >= g.n_loci || I.end < I.start || (k > g.tid_begin[t] && g.intervals[k - 1].start > I.start) || (int64_t)I.end - I.start > g.tid_max_span[t])
                VTXP_REJECT(VTX_E_INVAL, "vtx_submit_bam: interval %u: bad locus / order / span", k);
        }
    }
    return VTX_OK;
}

// blocks: ascending in the file, inside it with their trailers; the compressed range [lo, hi) travels as it is, and the kTrailer
// bytes behind it
inline int layout_blocks(const vtx_bam_ingest& g, Layout& L, char* why, size_t cap) {
    const uint32_t nb = g.n_blocks;
    L.blocks.resize(nb);
    L.lo = L.hi = nb ? g.blocks[0].coff : 0;
    L.utotal = 0;
    for (uint32_t i = 0; i < nb; ++i) {
        const vtx_bgzf_block& B = g.blocks[i];
        if (B.coff < L.hi || B.coff > g.file_bytes || B.clen > g.file_bytes - B.coff || B.isize > 65536u)
            VTXP_REJECT(VTX_E_INVAL, "vtx_submit_bam: block %u: out of order, outside the file or above 64 KiB", i);
        if (g.file_bytes - B.coff - B.clen < kTrailer)
            VTXP_REJECT(VTX_E_UNSUPPORTED, "vtx_submit_bam: BGZF block %u: its trailer (CRC32, ISIZE) lies beyond the end of the file: the host packer decides", i);
        L.blocks[i] = vtxg_block{B.coff - L.lo, L.utotal, B.clen, B.isize};
        L.hi = B.coff + B.clen;
        L.utotal += B.isize;
    }
    L.comp_bytes = nb ? L.hi - L.lo + kTrailer : 0;
    return VTX_OK;
}

// segmented: blocks[].coff is rebased to the compact buffer the segments' byte ranges are gathered into; the segment table tiles the
// blocks and the seeds in order; every seed and every end lies inside its segment's inflated bytes
inline int layout_segments(const vtx_bam_ingest& g, const vtx_bam_segments& sg, Layout& L, char* why, size_t cap) {
    const uint32_t nseg = sg.n_segments, nb = g.n_blocks;
    if ((nseg && !sg.segments) || (!nseg && (nb || g.n_seeds))) VTXP_REJECT(VTX_E_INVAL, "vtx_submit_bam_segments: blocks or seeds without segments");
    L.segs.resize(nseg); L.seed_seg.resize(g.n_seeds); L.pieces.reserve(nseg);
    uint32_t nbk = 0, nsd = 0;
    uint64_t ub = 0, cb = 0;
    for (uint32_t k = 0; k < nseg; ++k) {
        const vtx_bam_segment& S = sg.segments[k];
        if (S.block_begin != nbk || S.block_end <= S.block_begin || S.block_end > nb || S.seed_begin != nsd || S.seed_end <= S.seed_begin || S.seed_end > g.n_seeds)
            VTXP_REJECT(VTX_E_INVAL, "vtx_submit_bam_segments: segment %u: its blocks / seeds do not follow the segment before, or are empty", k);
        const uint64_t first = g.blocks[S.block_begin].coff, end = g.blocks[S.block_end - 1].coff + g.blocks[S.block_end - 1].clen;
        uint64_t ul = ub;
        for (uint32_t i = S.block_begin; i < S.block_end; ++i) { L.blocks[i].coff = cb + (g.blocks[i].coff - first); ul += g.blocks[i].isize; }
        const bool to_eof = (S.flags & VTX_SEGMENT_TO_EOF) != 0;
        if (S.end_upos > ul || (!to_eof && ul - S.end_upos < 12) || S.end_upos <= ub)
            VTXP_REJECT(VTX_E_INVAL, "vtx_submit_bam_segments: segment %u: its end (and the 12 bytes of the record there) lies outside its blocks", k);
        for (uint32_t i = S.seed_begin; i < S.seed_end; ++i) {
            if (g.seeds[i] < ub || g.seeds[i] >= S.end_upos || (i > S.seed_begin && g.seeds[i] <= g.seeds[i - 1]))
                VTXP_REJECT(VTX_E_INVAL, "vtx_submit_bam_segments: seed %u: not ascending or outside segment %u", i, k);
            L.seed_seg[i] = k;
        }
        L.segs[k] = vtxg_segment{ub, ul, S.end_upos, S.seed_end, S.end_tid, S.end_pos, S.flags};
        L.pieces.push_back(Piece{first, cb, end - first + kTrailer});      // (with its last block's trailer)
        nbk = S.block_end; nsd = S.seed_end; ub = ul; cb += end - first + kTrailer;
    }
    if (nbk != nb || nsd != g.n_seeds) VTXP_REJECT(VTX_E_INVAL, "vtx_submit_bam_segments: blocks or seeds behind the last segment");
    L.comp_bytes = cb;
    return VTX_OK;
}

// Second, behind check_arrays (and the loci's check): the rest of the checks in their order — tid_begin and intervals, blocks, segments,
// a contiguous plan's seeds — and the plan in the device's layout.  sg == nullptr: a contiguous plan (vtx_submit_bam); else g = sg->base.
// VTX_OK: L is filled.  VTX_E_INVAL / VTX_E_UNSUPPORTED: the reason in why[0 .. cap), L half filled and of no use.
inline int layout(const vtx_bam_ingest& g, const vtx_bam_segments* sg, Layout& L, char* why, size_t cap) {
    if (int rc = check_intervals(g, why, cap)) return rc;
    if (int rc = layout_blocks(g, L, why, cap)) return rc;
    if (sg) { if (int rc = layout_segments(g, *sg, L, why, cap)) return rc; }
    L.end_upos = std::min<uint64_t>(g.end_upos, L.utotal);
    for (uint32_t i = 0; !sg && i < g.n_seeds; ++i)
        if (g.seeds[i] >= L.end_upos || (i && g.seeds[i] <= g.seeds[i - 1])) VTXP_REJECT(VTX_E_INVAL, "vtx_submit_bam: seed %u: not ascending or beyond the end", i);
    const uint32_t ni = g.n_intervals, nref = g.n_ref;
    L.iv.assign(IntervalArrays::words(ni, nref), 0u);
    const IntervalArrays a = L.intervals(ni, nref);
    for (uint32_t k = 0; k < ni; ++k) { a.start()[k] = g.intervals[k].start; a.end()[k] = g.intervals[k].end; a.locus()[k] = g.intervals[k].locus; }
    for (uint32_t t = 0; t <= nref; ++t) a.tid_begin()[t] = g.tid_begin[t];
    for (uint32_t t = 0; t < nref; ++t) a.tid_span()[t] = g.tid_max_span[t];
    return VTX_OK;
}

#undef VTXP_REJECT

}  // namespace vtxp
#endif
