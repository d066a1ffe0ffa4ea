// vtx_prep_core.h — the decisions of the raw-batch preparation (vtx_prep.hip: prep_resolve_kernel, prep_finalize_kernel,
// prep_check_kernel; vtx_api.hip: vtx_set_barcodes, raw_prepare), as functions the host can compile too.
//
// What they restate (reference src/main.rs): load_barcodes (:697-718, the first index of a repeated line wins), get_cell_barcode and its
// use (:737-750, :867-876: a tag that is not in the list counts as num_not_cell_bc), the UB test (:879-888: only behind the barcode
// test, only with --umi), the grouping of a cell's reads by UMI BYTE STRING (:1047-1057) and the sort by cell (:932).
//
//   tag bytes      vtx_load_le, vtx_hash_bytes, vtx_bytes_equal: a 64-bit hash over little-endian 8-byte words, and the compare that must
//                  decide whenever two hashes are equal.  Every step of the hash is invertible, so equal hashes of different strings
//                  are easy to build (tests/prep_hash.py does): the byte and length compares are what keeps such tags apart.
//   barcode table  open addressing, slot = index + 1, 0 = empty, load <= 1/2, at least TABLE_MIN_SLOTS slots: table_build (host),
//                  table_probe (device and host)
//   records        raw_record_bad (the five conditions a raw record is turned away for), classify (barcode test, then UB test)
//   keys           bits_for, cell_bits_of, end_bit_of, kept_key, dropped_key: the (locus, cell) key the second radix sort orders by
//                  its low end_bit bits — dropped records carry the locus n_loci, which those bits must hold
//   heads          finalize_decide: group head, UMI head, collision flag, first / last record of a locus, for one sorted position
//   vtx_submit     check_code: the per-record code of the packed path's validation
//
// Compiles for the host (tests/prepcore/: the whole preparation run on the CPU from these functions against oracle/prep.py, plain and
// under sanitizers; CPU suite).  Mutation testing: VTXR_MUTANT = n > 0 makes ONE of the rules wrong on purpose, so that the tests can
// show they catch it (tests/test_prep_core.py).  Only the CPU harness's mutant builds define it; no GPU library ever does.
#ifndef VTX_PREP_CORE_H
#define VTX_PREP_CORE_H

#include <stdint.h>
#include <string.h>

#include "../../include/vtx.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VTXP_HD static __host__ __device__ inline
#else
#define VTXP_HD static inline
#endif

#ifndef VTXR_MUTANT
#define VTXR_MUTANT 0
#endif
#if VTXR_MUTANT && (defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__))
#error "VTXR_MUTANT is for the CPU harness only"
#endif

// 64-bit hash of a tag byte string (FNV-1a style over little-endian 8-byte words + fmix64), identical on the
// host (barcode table build) and the device.  The words are read with memcpy: gfx950 global memory takes
// unaligned dwordx2 loads, so a lane hashes an 18-byte barcode with 3 loads instead of 18.
VTXP_HD uint64_t vtx_load_le(const uint8_t* p, uint32_t n) {   // n <= 8 bytes, zero-extended
    uint64_t w = 0;
    if (n == 8) { __builtin_memcpy(&w, p, 8); return w; }
    for (uint32_t i = 0; i < n; ++i) w |= (uint64_t)p[i] << (8 * i);
    return w;
}
VTXP_HD uint64_t vtx_hash_bytes(const uint8_t* p, uint32_t n, uint64_t seed) {
    uint64_t h = (0xcbf29ce484222325ull ^ seed) + n;
    for (uint32_t i = 0; i < n; i += 8) { h ^= vtx_load_le(p + i, n - i < 8 ? n - i : 8); h *= 0x100000001b3ull; h ^= h >> 29; }
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
    return h;
}
VTXP_HD bool vtx_bytes_equal(const uint8_t* a, const uint8_t* b, uint32_t n) {
    bool eq = true;
#if VTXR_MUTANT == 1
    if (n > 8) n = 8;                                   // the first word only
#elif VTXR_MUTANT == 2
    n &= ~7u;                                           // whole words only
#endif
    for (uint32_t i = 0; i < n; i += 8) { const uint32_t m = n - i < 8 ? n - i : 8; eq &= vtx_load_le(a + i, m) == vtx_load_le(b + i, m); }
    return eq;
}

namespace vtxp {

// ---- the barcode table ----
constexpr uint32_t TABLE_MIN_SLOTS = 16;
constexpr uint32_t NO_CELL = 0xffffffffu;

VTXP_HD uint32_t table_capacity(uint32_t n) {          // a power of two, load <= 1/2
    uint32_t cap = TABLE_MIN_SLOTS;
    while (cap < 2ull * n) cap <<= 1;
    return cap;
}

// slots[cap] (zeroed) and hashes[n] from the list bytes[offsets[j] .. offsets[j + 1]): a byte string that occurs again keeps its first index
static inline void table_build(const uint8_t* bytes, const uint64_t* offsets, uint32_t n, uint32_t cap, uint32_t* slots, uint64_t* hashes) {
    for (uint32_t j = 0; j < n; ++j) {
        const uint8_t* b = bytes + offsets[j];
        const uint32_t len = (uint32_t)(offsets[j + 1] - offsets[j]);
        const uint64_t h = vtx_hash_bytes(b, len, 0);
        hashes[j] = h;
        bool dup = false;
        uint32_t sidx = (uint32_t)h & (cap - 1);
        for (; slots[sidx]; sidx = (sidx + 1) & (cap - 1)) {
            const uint32_t k = slots[sidx] - 1;
            if (hashes[k] == h && offsets[k + 1] - offsets[k] == len && memcmp(bytes + offsets[k], b, len) == 0) { dup = true; break; }
        }
        if (!dup) slots[sidx] = j + 1;
    }
}

// the index of the tag b[0 .. len) in the list, or NO_CELL: equal hash, equal length and equal bytes, walking on past everything else
// until an empty slot
VTXP_HD uint32_t table_probe(const uint32_t* slots, uint32_t mask, const uint64_t* hash, const uint64_t* off, const uint8_t* bytes,
                             const uint8_t* b, uint32_t len) {
    const uint64_t h = vtx_hash_bytes(b, len, 0);
    uint32_t cell = NO_CELL;
#if VTXR_MUTANT == 5
    for (uint32_t s = (uint32_t)h & mask;; s = s == mask ? 1u : s + 1) {
#else
    for (uint32_t s = (uint32_t)h & mask;; s = (s + 1) & mask) {
#endif
        const uint32_t e = slots[s];
        if (!e) break;
        const uint32_t j = e - 1;
        if (hash[j] != h) continue;
        const uint64_t o = off[j];
#if VTXR_MUTANT == 4
        if (off[j + 1] - o == len && vtx_bytes_equal(bytes + o, b, len)) cell = j;
        break;                                          // the first equal hash decides
#else
#if VTXR_MUTANT != 3
        if (off[j + 1] - o != len) continue;
#endif
        if (vtx_bytes_equal(bytes + o, b, len)) { cell = j; break; }
#endif
    }
    return cell;
}

// ---- raw records ----
// what vtx_submit_raw turns a record away for (VTX_E_INVAL): barcode bytes or read outside the arena, read too long, read at an odd
// base (odd_mask = 1: VTX_READS_NIBBLES), UMI bytes outside the arena — those only where the UMI is read (use_umi, tag present)
VTXP_HD bool raw_record_bad(const vtx_raw_record& r, uint64_t tag_bytes, uint64_t read_bytes, uint32_t max_read_len, uint32_t odd_mask,
                            int use_umi) {
    const bool umi_missing = r.umi_len == VTX_TAG_MISSING;
    return (uint64_t)r.bc_off + r.bc_len > tag_bytes || (uint64_t)r.read_off + r.read_len > read_bytes ||
           r.read_len > max_read_len || (r.read_off & odd_mask) || (use_umi && !umi_missing && (uint64_t)r.umi_off + r.umi_len > tag_bytes);
}

enum Class : uint32_t { KEEP = 0, NOT_CELL_BC = 1, NON_UMI = 2 };
// the barcode test first (:870-876), the UB test behind it and only with --umi (:879-888): a record counts once
VTXP_HD Class classify(uint32_t cell, int use_umi, bool umi_missing) {
#if VTXR_MUTANT == 9
    if (use_umi && umi_missing) return NON_UMI;
    if (cell == NO_CELL) return NOT_CELL_BC;
    return KEEP;
#else
    if (cell == NO_CELL) return NOT_CELL_BC;
    if (use_umi && umi_missing) return NON_UMI;
    return KEEP;
#endif
}

// ---- sort keys ----
VTXP_HD uint32_t bits_for(uint64_t max_value) {   // bits needed to represent values 0..max_value
    uint32_t b = 1;
    while (b < 64 && (max_value >> b)) ++b;
    return b;
}
VTXP_HD uint32_t cell_bits_of(uint32_t n_barcodes) { return bits_for(n_barcodes ? n_barcodes - 1 : 0); }
// the bits the (locus, cell) sort looks at: the locus field holds 0 .. n_loci, the last value being the dropped records'
VTXP_HD uint32_t end_bit_of(uint32_t cell_bits, uint32_t n_loci) {
#if VTXR_MUTANT == 7
    return cell_bits + bits_for(n_loci) - 1;
#else
    return cell_bits + bits_for(n_loci);
#endif
}
VTXP_HD uint64_t kept_key(uint32_t locus, uint32_t cell, uint32_t cell_bits) { return ((uint64_t)locus << cell_bits) | cell; }
// larger than every kept key: dropped records end up behind the n_kept kept ones
VTXP_HD uint64_t dropped_key(uint32_t n_loci, uint32_t cell_bits) {
#if VTXR_MUTANT == 6
    return (uint64_t)(n_loci - 1) << cell_bits;
#else
    return (uint64_t)n_loci << cell_bits;
#endif
}
VTXP_HD uint32_t key_locus(uint64_t k, uint32_t cell_bits) { return (uint32_t)(k >> cell_bits); }
VTXP_HD uint32_t key_cell(uint64_t k, uint32_t cell_bits) { return (uint32_t)(k & ((1ull << cell_bits) - 1)); }

// the UMI hash seeds of raw_prepare's rounds
constexpr uint64_t UMI_SEED0 = 0x9e3779b97f4a7c15ull;
constexpr uint32_t UMI_MAX_ROUNDS = 8;
VTXP_HD uint64_t next_seed(uint64_t seed) { return seed * 0xd1342543de82ef95ull + 1; }

// ---- group heads ----
// What sorted position j (of n_kept; r = raw[perm[j]]) is.  head: the first record of a (locus, cell) group or, with UMIs, of a UMI
// inside it.  collide: its predecessor in the group has the same UMI hash and OTHER bytes — this seed merges two molecules, the caller
// takes the next one.  The predecessor is position j - 1 whatever workgroup handles it.
struct Decision { uint32_t locus, cell; bool head, collide, locus_first, locus_last; };
VTXP_HD Decision finalize_decide(uint32_t j, uint32_t n_kept, const uint32_t* perm, const uint64_t* key_lc_sorted, const uint64_t* key_umi,
                                 const vtx_raw_record* raw, const vtx_raw_record& r, const uint8_t* tags, uint32_t cell_bits, int use_umi) {
    Decision d;
    const uint64_t k = key_lc_sorted[j];
    d.locus = key_locus(k, cell_bits); d.cell = key_cell(k, cell_bits);
#if VTXR_MUTANT == 10
    const uint64_t kprev = (j & 255u) ? key_lc_sorted[j - 1] : ~0ull;
#else
    const uint64_t kprev = j ? key_lc_sorted[j - 1] : ~0ull;
#endif
    d.head = kprev != k;
    d.collide = false;
    if (use_umi && !d.head) {
        const uint32_t i = perm[j], ip = perm[j - 1];
        if (key_umi[ip] != key_umi[i]) d.head = true;
#if VTXR_MUTANT == 8
        (void)raw; (void)r; (void)tags;                 // equal hashes are taken for equal bytes
#else
        else {
            // equal hashes inside one (locus, cell): must be the same bytes, else this seed collides
            const vtx_raw_record q = raw[ip];
            if (q.umi_len != r.umi_len || !vtx_bytes_equal(tags + q.umi_off, tags + r.umi_off, r.umi_len)) d.collide = true;
        }
#endif
    }
    // records are sorted by locus: the run boundaries give every locus its record range
    d.locus_first = j == 0 || key_locus(kprev, cell_bits) != d.locus;
    d.locus_last = j + 1 == n_kept || key_locus(key_lc_sorted[j + 1], cell_bits) != d.locus;
    return d;
}

// ---- vtx_submit's per-record validation ----
// 0 = fine, 1 read outside the arena, 2 read too long, 3 cell_index >= n_barcodes, 5 read at an odd base (odd_mask = 1), 4 order:
// (cell_index, umi_id) descending inside a locus (cell_index alone when !use_umi).  The first condition in that sequence names the record.
VTXP_HD uint32_t check_code(const vtx_record* records, const uint32_t* rec_locus, uint32_t j, const vtx_record& r, uint32_t locus,
                            uint64_t read_bytes, uint32_t max_read_len, uint32_t odd_mask, uint32_t n_barcodes, int use_umi) {
    uint32_t code = 0;
    if ((uint64_t)r.read_off + r.read_len > read_bytes) code = 1;
    else if (r.read_len > max_read_len) code = 2;
    else if (r.cell_index >= n_barcodes) code = 3;
    else if (r.read_off & odd_mask) code = 5;
    else if (j > 0 && rec_locus[j - 1] == locus) {
        const vtx_record q = records[j - 1];
        if (q.cell_index > r.cell_index || (use_umi && q.cell_index == r.cell_index && q.umi_id > r.umi_id)) code = 4;
    }
    return code;
}
// what the batch reports is the minimum of these over the offending records: the smallest record, then its code
VTXP_HD unsigned long long check_word(uint32_t j, uint32_t code) { return ((unsigned long long)j << 3) | code; }

}  // namespace vtxp

#endif
