// vtx_scan_core.h — what bam_scan_kernel (vtx_ingest.hip) knows about ONE BAM record: its fixed fields and end position, the CIGAR
// walk behind useful_alignment, the aux lookup, and the overlap-and-filter loop over the loci of its contig.
//
// What it replaces (reference 10XGenomics/vartrix v1.1.22): `bam.fetch(tid, start, end)` + `bam.records()` as seen from one record
// (htslib's overlap of [pos, bam_endpos) with [start, end), src/main.rs:822-830), the read filters in their order (:831-864),
// useful_alignment (:790-806, rust-htslib 0.36 CigarStringView::read_pos below it) and get_cell_barcode / get_umi as tag bytes
// (:737-757).  The host packer (host/vtx_host.cpp) and the oracle (oracle/vtx_oracle.c, oracle/refpipe.py) restate the same rules.
//
// Compiles for the host too (tests/scancore/: the same functions on raw record bytes, against an independently written model in
// tests/bam_grammar_util.py; CPU suite).
#ifndef VTX_SCAN_CORE_H
#define VTX_SCAN_CORE_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/vtx.h"

#ifdef __HIPCC__
#define VTXS_FN __device__ __forceinline__
#else
#define VTXS_FN static inline
#endif

namespace vtxs {

VTXS_FN uint32_t ld32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
VTXS_FN uint32_t ld16(const uint8_t* p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }
VTXS_FN uint64_t ld64(const uint8_t* p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }

constexpr uint32_t AUX_NONE = 0xffffffffu;

// ---------------------------------------------------------------------------------------------------------------------------
// rust-htslib 0.36 CigarStringView::read_pos(ref_pos, include_softclips = false, include_dels = true) as called from
// useful_alignment (src/main.rs:796): 1 = Some, 0 = None, -1 = Err.  Same restatement as host/vtx_host.cpp: cigar_read_pos and
// oracle/vtx_oracle.c: vtxo_cigar_read_pos.
// ---------------------------------------------------------------------------------------------------------------------------
VTXS_FN int cigar_read_pos(const uint8_t* cig, uint32_t n_ops, int64_t pos, int64_t ref_pos) {
    int64_t rpos = pos;
    uint32_t j = 0;
    for (uint32_t i = 0; i < n_ops; ++i) {
        const uint32_t op = ld32(cig + 4 * i) & 15u;
        if (op == 0 || op == 7 || op == 8 || op == 1) { j = i; break; }
        if (op == 4) { j = i; break; }
        if (op == 2 || op == 3) return -1;
        if (op == 5 && i > 0 && i + 1 < n_ops) return -1;
        if ((op == 6 || op == 5) && i + 1 == n_ops) return 0;
    }
    while (rpos <= ref_pos && j < n_ops) {
        const uint32_t c = ld32(cig + 4 * j), op = c & 15u;
        const int64_t l = c >> 4;
        const bool contains = rpos <= ref_pos && rpos + l > ref_pos;
        switch (op) {
        case 0: case 7: case 8: if (contains) return 1; rpos += l; ++j; break;
        case 4: ++j; break;
        case 2: if (contains) return 1; rpos += l; ++j; break;
        case 3: rpos += l; ++j; break;
        case 1: case 6: ++j; break;
        case 5: if (j + 1 < n_ops) return -1; return 0;
        default: return -1;
        }
    }
    return 0;
}
// useful_alignment, src/main.rs:790-806 (probes start..=end, inclusive; an invalid CIGAR drops the read, :799-802)
VTXS_FN bool useful_alignment(const uint8_t* cig, uint32_t n_ops, int64_t pos, int64_t start, int64_t end) {
    for (int64_t i = start; i <= end; ++i) {
        const int r = cigar_read_pos(cig, n_ops, pos, i);
        if (r == 1) return true;
        if (r < 0) return false;
    }
    return false;
}
// rec.aux(tag) matched against Aux::String (src/main.rs:742-748, :753-755): type 'Z' only.  Returns the value's offset from aux
// (AUX_NONE: no such Z tag) and *len.
VTXS_FN uint32_t aux_string(const uint8_t* aux, uint32_t n, uint32_t tag2, uint32_t* len) {
    uint32_t o = 0;
    while (o + 3 <= n) {
        const uint32_t t2 = ld16(aux + o);
        const uint32_t ty = aux[o + 2];
        o += 3;
        uint32_t size;
        bool is_z = false;
        switch (ty) {
        case 'A': case 'c': case 'C': size = 1; break;
        case 's': case 'S': size = 2; break;
        case 'i': case 'I': case 'f': size = 4; break;
        case 'd': size = 8; break;
        case 'Z': case 'H': {
            uint32_t e = o;
            while (e < n && aux[e]) ++e;
            if (e >= n) return AUX_NONE;              // no NUL inside the record: htslib's bam_aux_get gives NULL on corrupt aux data
            size = e - o + 1;
            is_z = ty == 'Z';
            break;
        }
        case 'B': {
            if (o + 5 > n) return AUX_NONE;
            const uint32_t sub = aux[o];
            const uint32_t cnt = ld32(aux + o + 1);
            const uint32_t es = (sub == 'c' || sub == 'C') ? 1u : (sub == 's' || sub == 'S') ? 2u : (sub == 'i' || sub == 'I' || sub == 'f') ? 4u : 0u;
            if (!es) return AUX_NONE;                 // (an unknown subtype has no size: corrupt, as for htslib's skip_aux)
            const uint64_t sz = 5ull + (uint64_t)cnt * es;
            if (sz > n) return AUX_NONE;
            size = (uint32_t)sz;
            break;
        }
        default: return AUX_NONE;
        }
        if (t2 == tag2) {
            if (!is_z) return AUX_NONE;
            *len = size - 1;
            return o;
        }
        o += size;
    }
    return AUX_NONE;
}

struct RecView {
    const uint8_t* r;          // behind block_size
    uint32_t bs;
    int32_t tid;
    int64_t pos, endpos;
    uint32_t mapq, flag, n_cig, l_seq;
    const uint8_t* cig;
    const uint8_t* sq;
    const uint8_t* aux;
    bool malformed;
};
VTXS_FN RecView view_record(const uint8_t* data, uint64_t p) {
    RecView v;
    v.bs = ld32(data + p);
    v.r = data + p + 4;
    v.tid = (int32_t)ld32(v.r);
    v.pos = (int32_t)ld32(v.r + 4);
    const uint32_t w2 = ld32(v.r + 8), w3 = ld32(v.r + 12);
    const uint32_t l_rn = w2 & 0xffu;
    v.mapq = (w2 >> 8) & 0xffu;
    v.n_cig = w3 & 0xffffu;
    v.flag = w3 >> 16;
    v.l_seq = ld32(v.r + 16);
    v.cig = v.r + 32 + l_rn;
    v.sq = v.cig + 4 * (size_t)v.n_cig;
    const uint64_t aux_off = 32ull + l_rn + 4ull * v.n_cig + ((uint64_t)v.l_seq + 1) / 2 + v.l_seq;
    v.malformed = aux_off > v.bs;
    v.aux = v.r + (v.malformed ? v.bs : aux_off);
    int64_t rlen = 0;                                     // bam_endpos: unmapped or no reference-consuming op => pos + 1
    if (!v.malformed && !(v.flag & 0x4u))
        for (uint32_t k = 0; k < v.n_cig; ++k) {
            const uint32_t c = ld32(v.cig + 4 * k), op = c & 15u;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += c >> 4;
        }
    v.endpos = v.pos + (rlen > 0 ? rlen : 1);
    return v;
}

// One step of a record-chain walk (bam_chain_kernel, bam_chain_seg_kernel: block_size to block_size from a seed): the record at p
// must have its block_size and fixed fields (36 bytes) and its whole body inside [.., limit); a block_size below the 32 fixed bytes
// is no record.  true: p moves behind the record.  false: the chain is broken at p (left as it is).  Reads data[p .. p + 4) only,
// and only when p + 36 <= limit.
VTXS_FN bool chain_step(const uint8_t* data, uint64_t& p, uint64_t limit) {
    if (p + 36 > limit) return false;
    const uint32_t bs = ld32(data + p);
    if (bs < 32 || p + 4 + (uint64_t)bs > limit) return false;
    p += 4 + (uint64_t)bs;
    return true;
}

// hi = first interval of the contig with start >= endpos (the loci that can overlap lie below it)
VTXS_FN uint32_t first_not_below(const int32_t* __restrict__ iv_start, uint32_t lo, uint32_t hi, int64_t endpos) {
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((int64_t)iv_start[mid] < endpos) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// What became of one (read, locus) pair: the filters in the reference's order, each with the Metrics counter it feeds.
enum Pair : uint32_t { PAIR_KEPT = 0, PAIR_LOW_MAPQ, PAIR_NON_PRIMARY, PAIR_DUPLICATE, PAIR_NOT_USEFUL, PAIR_NO_BARCODE };
struct Filter { uint32_t n_ref, min_mapq, primary_only, no_duplicates, bam_tag; };
// per record: the counters of its pairs, and where its barcode / UB tag bytes lie (offsets from the record body; a length of
// VTX_TAG_MISSING: no such Z tag — a value of 65 535 bytes or more counts as missing, the length travels as 16 bits)
struct Verdict {
    uint32_t hits = 0, reads = 0, low_mapq = 0, non_primary = 0, duplicate = 0, not_useful = 0, no_barcode = 0;
    uint32_t bc_rel = 0, umi_rel = 0, bc_len = VTX_TAG_MISSING, umi_len = VTX_TAG_MISSING;
};

// The loci of the record's contig it overlaps, from the highest interval down, and the filters per pair.  FIND_TAGS: look the tags
// up at the first pair that gets that far (otherwise V comes with them); visit(k, outcome, hit) sees every overlapping interval k,
// hit = the running number of kept pairs.  The record is not malformed.
template <bool FIND_TAGS, class Visit>
VTXS_FN void scan_pairs(const RecView& v, const Filter& f, const int32_t* __restrict__ iv_start, const int32_t* __restrict__ iv_end,
                        const uint32_t* __restrict__ tid_begin, const int32_t* __restrict__ tid_span, Verdict& V, Visit&& visit) {
    if (!(v.tid >= 0 && (uint32_t)v.tid < f.n_ref)) return;
    const uint32_t i0 = tid_begin[v.tid], i1 = tid_begin[v.tid + 1];
    if (i1 <= i0) return;
    bool tags_ready = false;
    const int64_t span = tid_span[v.tid];
    uint32_t k = first_not_below(iv_start, i0, i1, v.endpos);
    // loci of this contig with start < endpos && end > pos (htslib's overlap on [start, end), src/main.rs:822-826)
    while (k-- > i0) {
        if ((int64_t)iv_start[k] + span <= v.pos) break;
        if ((int64_t)iv_end[k] <= v.pos) continue;
        ++V.reads;                                                                                   // :831
        if (v.mapq < f.min_mapq) { ++V.low_mapq; visit(k, PAIR_LOW_MAPQ, V.hits); continue; }                        // :833
        if (f.primary_only && (v.flag & (0x100u | 0x800u))) { ++V.non_primary; visit(k, PAIR_NON_PRIMARY, V.hits); continue; }   // :841
        if (f.no_duplicates && (v.flag & 0x400u)) { ++V.duplicate; visit(k, PAIR_DUPLICATE, V.hits); continue; }     // :849
        if (!useful_alignment(v.cig, v.n_cig, v.pos, iv_start[k], iv_end[k])) { ++V.not_useful; visit(k, PAIR_NOT_USEFUL, V.hits); continue; }   // :857
        if (FIND_TAGS && !tags_ready) {
            tags_ready = true;
            const uint32_t n_aux = (uint32_t)(v.r + v.bs - v.aux);
            uint32_t len = 0;
            uint32_t o = aux_string(v.aux, n_aux, f.bam_tag, &len);            // :867 (the in-list test: vtx_prep.hip)
            if (o != AUX_NONE && len < VTX_TAG_MISSING) {
                V.bc_rel = (uint32_t)(v.aux - v.r) + o; V.bc_len = len;
                o = aux_string(v.aux, n_aux, (uint32_t)'U' | ((uint32_t)'B' << 8), &len);   // :879 (the test itself: vtx_prep.hip)
                if (o != AUX_NONE && len < VTX_TAG_MISSING) { V.umi_rel = (uint32_t)(v.aux - v.r) + o; V.umi_len = len; }
            }
        }
        if (V.bc_len == VTX_TAG_MISSING) { ++V.no_barcode; visit(k, PAIR_NO_BARCODE, V.hits); continue; }
        visit(k, PAIR_KEPT, V.hits);
        ++V.hits;
    }
}

// The 4-bit base codes of a BAM record (SAM spec 4.2.3: "=ACMGRSVTWYHKDBN"; rec.seq().as_bytes(), src/main.rs:896, decodes with the
// same table), as two 64-bit constants: unpack_nibbles_kernel (vtx_kernels.hip) decodes with shifts, no table in memory.
VTXS_FN uint32_t nt16_char(uint32_t nib) {
    const uint64_t lut_lo = 0x565352474d43413dull, lut_hi = 0x4e42444b48595754ull;      // "=ACMGRSV", "TWYHKDBN" (little endian)
    return (uint32_t)(((nib & 8u) ? lut_hi : lut_lo) >> (8u * (nib & 7u))) & 0xffu;
}

}  // namespace vtxs

#endif
