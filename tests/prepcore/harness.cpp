// Host build of vartrix_amd/csrc/vtx_prep_core.h for tests/test_prep_core.py and tests/test_gpu_prep_cases.py (ctypes): the tag hash
// and compare, the barcode table, the key widths, vtx_submit's record codes, and the whole preparation of a raw batch (prep_host.h).
// The tag arena and the barcode bytes are copied into buffers with 64 spare bytes: a MUTANT build (-DVTXR_MUTANT=n, one rule wrong on
// purpose) may compare past a string's end, and must give a wrong answer, not a fault.  What the real header touches is checked by the
// stand-alone program (main.cpp) in allocations of exactly the arrays' sizes, under sanitizers.
#include <string.h>

#include "prep_host.h"

extern "C" {
int vtxt_prep_mutant(void) { return VTXR_MUTANT; }
uint64_t vtxt_hash_bytes(const uint8_t* p, uint32_t n, uint64_t seed) { return vtx_hash_bytes(p, n, seed); }
int vtxt_bytes_equal(const uint8_t* a, const uint8_t* b, uint32_t n) { return vtx_bytes_equal(a, b, n) ? 1 : 0; }
uint64_t vtxt_next_seed(uint64_t seed) { return seed ? vtxp::next_seed(seed) : vtxp::UMI_SEED0; }      // 0 -> the first seed
// out: cell_bits, end_bit, dropped key, the key of (n_loci - 1, n_barcodes - 1)
void vtxt_key_widths(uint32_t n_barcodes, uint32_t n_loci, uint64_t* out) {
    const uint32_t cb = vtxp::cell_bits_of(n_barcodes);
    out[0] = cb; out[1] = vtxp::end_bit_of(cb, n_loci); out[2] = vtxp::dropped_key(n_loci, cb);
    out[3] = vtxp::kept_key(n_loci ? n_loci - 1 : 0, n_barcodes ? n_barcodes - 1 : 0, cb);
}
// the table of a list: returns its slot count, slots_out (room for table_capacity(n)) may be null
uint32_t vtxt_table(const uint8_t* bc_bytes, const uint64_t* bc_off, uint32_t n, uint32_t* slots_out) {
    const uint32_t cap = vtxp::table_capacity(n);
    if (slots_out) {
        std::vector<uint64_t> hashes(std::max(n, 1u));
        memset(slots_out, 0, cap * sizeof(uint32_t));
        vtxp::table_build(bc_bytes, bc_off, n, cap, slots_out, hashes.data());
    }
    return cap;
}
// table_probe over the caller's arrays (the hashes need not be those of the bytes): the index found, or 0xFFFFFFFF
uint32_t vtxt_table_probe(const uint32_t* slots, uint32_t mask, const uint64_t* hash, const uint64_t* off, const uint8_t* bytes, uint32_t n,
                          const uint8_t* tag, uint32_t len) {
    std::vector<uint8_t> b(off[n] + 64, 0x5A), t((size_t)len + 64, 0xA5);
    if (off[n]) memcpy(b.data(), bytes, off[n]);
    if (len) memcpy(t.data(), tag, len);
    return vtxp::table_probe(slots, mask, hash, off, b.data(), t.data(), len);
}
// stats: not_cell_bc, non_umi, kept, rounds, cell_bits, end_bit, table slots.  records_out holds n_records, rec_begin / rec_count n_loci.
int vtxt_prep_run(const vtx_locus* loci, uint32_t n_loci, const vtx_raw_record* raw, uint32_t n_records, const uint8_t* tags,
                  uint64_t tag_bytes, uint64_t read_bytes, uint32_t max_read_len, int nibbles, const uint8_t* bc_bytes,
                  const uint64_t* bc_off, uint32_t n_barcodes, int use_umi, uint32_t weak_rounds, vtx_record* records_out,
                  uint32_t* rec_begin, uint32_t* rec_count, uint64_t* stats) {
    std::vector<uint8_t> t(tag_bytes + 64, 0xA5), b((n_barcodes ? bc_off[n_barcodes] : 0) + 64, 0x5A);
    if (tag_bytes) memcpy(t.data(), tags, tag_bytes);
    if (n_barcodes && bc_off[n_barcodes]) memcpy(b.data(), bc_bytes, bc_off[n_barcodes]);
    prep_host::In in{loci, n_loci, raw, n_records, t.data(), tag_bytes, read_bytes, max_read_len, nibbles, b.data(), bc_off, n_barcodes, use_umi, weak_rounds};
    const prep_host::Out o = prep_host::run(in);
    stats[0] = o.not_cell_bc; stats[1] = o.non_umi; stats[2] = o.kept; stats[3] = o.rounds; stats[4] = o.cell_bits; stats[5] = o.end_bit;
    stats[6] = o.table_slots;
    if (o.status) return o.status;
    if (o.kept) memcpy(records_out, o.records.data(), o.kept * sizeof(vtx_record));
    if (n_loci) { memcpy(rec_begin, o.rec_begin.data(), n_loci * 4); memcpy(rec_count, o.rec_count.data(), n_loci * 4); }
    return 0;
}
// prep_check_kernel's word for a packed batch: all ones, or the smallest (record << 3 | code)
uint64_t vtxt_prep_check(const vtx_locus* loci, uint32_t n_loci, const vtx_record* records, uint32_t n_records, uint64_t read_bytes,
                         uint32_t max_read_len, int nibbles, uint32_t n_barcodes, int use_umi) {
    return prep_host::check(loci, n_loci, records, n_records, read_bytes, max_read_len, nibbles, n_barcodes, use_umi);
}
}
