// Host build of vartrix_amd/csrc/vtx_scan_core.h for tests/test_scan_core.py: the functions bam_scan_kernel is compiled from, one C
// entry per function, on raw record bytes.  The *_table entries take a whole table of cases in one call (the CIGAR enumeration has
// a quarter of a million probes).
#include <stdint.h>
#include <string.h>

#include "../../vartrix_amd/csrc/vtx_scan_core.h"

extern "C" {

int vtxs_t_read_pos(const uint8_t* cig, uint32_t n_ops, int64_t pos, int64_t ref_pos) { return vtxs::cigar_read_pos(cig, n_ops, pos, ref_pos); }
int vtxs_t_useful(const uint8_t* cig, uint32_t n_ops, int64_t pos, int64_t start, int64_t end) { return vtxs::useful_alignment(cig, n_ops, pos, start, end) ? 1 : 0; }

// CIGAR c = ops[cig_off[c] .. cig_off[c + 1]) at pos[c]; its probes = probes[probe_off[c] .. probe_off[c + 1]); out: one verdict per probe
void vtxs_t_read_pos_table(const uint32_t* ops, const uint64_t* cig_off, uint64_t n, const int64_t* pos, const int64_t* probes,
                           const uint64_t* probe_off, int8_t* out) {
    for (uint64_t c = 0; c < n; ++c)
        for (uint64_t q = probe_off[c]; q < probe_off[c + 1]; ++q)
            out[q] = (int8_t)vtxs::cigar_read_pos((const uint8_t*)(ops + cig_off[c]), (uint32_t)(cig_off[c + 1] - cig_off[c]), pos[c], probes[q]);
}
// the same with windows: win[2 q], win[2 q + 1] = start, end (inclusive) of window q
void vtxs_t_useful_table(const uint32_t* ops, const uint64_t* cig_off, uint64_t n, const int64_t* pos, const int64_t* win,
                         const uint64_t* win_off, int8_t* out) {
    for (uint64_t c = 0; c < n; ++c)
        for (uint64_t q = win_off[c]; q < win_off[c + 1]; ++q)
            out[q] = vtxs::useful_alignment((const uint8_t*)(ops + cig_off[c]), (uint32_t)(cig_off[c + 1] - cig_off[c]), pos[c], win[2 * q], win[2 * q + 1]) ? 1 : 0;
}

// view_record of the record at data + p (its block_size first).  out[12]: bs, tid, pos, endpos, mapq, flag, n_cig, l_seq and the
// offsets of the CIGAR, the bases and the aux block from the record body, malformed
void vtxs_t_view(const uint8_t* data, uint64_t p, int64_t* out) {
    const vtxs::RecView v = vtxs::view_record(data, p);
    out[0] = v.bs; out[1] = v.tid; out[2] = v.pos; out[3] = v.endpos; out[4] = v.mapq; out[5] = v.flag; out[6] = v.n_cig; out[7] = v.l_seq;
    out[8] = v.cig - v.r; out[9] = v.sq - v.r; out[10] = v.aux - v.r; out[11] = v.malformed ? 1 : 0;
}
void vtxs_t_view_table(const uint8_t* data, const uint64_t* rec_off, uint64_t n, int64_t* out) {
    for (uint64_t i = 0; i < n; ++i) vtxs_t_view(data, rec_off[i], out + 12 * i);
}

// aux_string: the value's offset from aux (0xffffffff: no such Z tag) and *len
uint32_t vtxs_t_aux_string(const uint8_t* aux, uint32_t n, const char* tag, uint32_t* len) {
    return vtxs::aux_string(aux, n, (uint32_t)(uint8_t)tag[0] | ((uint32_t)(uint8_t)tag[1] << 8), len);
}

uint32_t vtxs_t_first_not_below(const int32_t* iv_start, uint32_t lo, uint32_t hi, int64_t endpos) { return vtxs::first_not_below(iv_start, lo, hi, endpos); }
uint32_t vtxs_t_nt16(uint32_t code) { return vtxs::nt16_char(code); }

// The overlap-and-filter loop on one record, as the counting pass runs it (the tags looked up).  filter[5]: n_ref, min_mapq,
// primary_only, no_duplicates, the tag's two bytes; pair_k / pair_outcome (cap entries): every overlapping interval in the order
// the loop visits them and what became of the pair (vtxs::Pair); verdict[11]: hits, reads, low_mapq, non_primary, duplicate,
// not_useful, no_barcode, bc_rel, umi_rel, bc_len, umi_len.  Returns the number of pairs, -1: the record is malformed (the kernel
// does not scan it), -2: more than cap pairs.
int vtxs_t_scan(const uint8_t* data, uint64_t p, const uint32_t* filter, const int32_t* iv_start, const int32_t* iv_end,
                const uint32_t* tid_begin, const int32_t* tid_span, uint32_t* pair_k, uint32_t* pair_outcome, uint32_t cap, uint32_t* verdict) {
    const vtxs::RecView v = vtxs::view_record(data, p);
    if (v.malformed) return -1;
    const vtxs::Filter f{filter[0], filter[1], filter[2], filter[3], filter[4]};
    vtxs::Verdict V;
    uint32_t n = 0;
    bool over = false, hits_ok = true;
    vtxs::scan_pairs<true>(v, f, iv_start, iv_end, tid_begin, tid_span, V, [&](uint32_t k, uint32_t outcome, uint32_t hit) {
        if (hit != V.hits) hits_ok = false;                 // (the running number of kept pairs, as the emit pass indexes with it)
        if (n < cap) { pair_k[n] = k; pair_outcome[n] = outcome; ++n; } else over = true;
    });
    const uint32_t out[11] = {V.hits, V.reads, V.low_mapq, V.non_primary, V.duplicate, V.not_useful, V.no_barcode, V.bc_rel, V.umi_rel, V.bc_len, V.umi_len};
    memcpy(verdict, out, sizeof out);
    return over ? -2 : hits_ok ? (int)n : -3;
}

}
