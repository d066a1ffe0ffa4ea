// vtx_crc32_core.h — the CRC-32 of gzip (RFC 1952 8.: reflected polynomial 0xEDB88320, register starts and ends with all ones; bit for
// bit zlib's crc32()) of one BGZF block by ONE WAVEFRONT: the lane and wavefront logic of bgzf_crc32_kernel (vtx_ingest.hip).
//
// What it replaces: htslib bgzf_read_block -> crc32() of every inflated block against the block's trailer, behind `bam.records()`
// (src/main.rs:822-830; a mismatch is the Err of `let rec = _rec?`, :829-830).
//
// A CRC is linear over GF(2): the raw register (started from ZERO, no final xor) of A || B is raw(A) * x^(8|B|) + raw(B) modulo the
// polynomial, and leading zero bytes leave a zero register as it is.  So a block is cut into pieces that lanes work on independently,
// and the all-ones start and final xor are added at the end as 0xFFFFFFFF * x^(8 n) + 0xFFFFFFFF.
//
// The lane-chunk rule (the issue suggested one contiguous chunk per lane; that makes the lanes of a load 1 KiB apart — 64 cache lines
// per instruction — unless tiles are staged through LDS): the pieces are INTERLEAVED instead.  The block's bytes up to the last
// W-aligned address (W = 4, 8 or 16 bytes per step) are W-byte pieces at W-aligned addresses; piece k goes to lane k mod 64, so one
// load instruction of the wavefront reads 64 W consecutive, aligned bytes.  A lane's bytes are then W bytes out of every 64 W: its
// register has to skip 63 W zero bytes between two pieces, and the slicing tables do that for nothing — table j holds, for every byte
// value, the register of that byte followed by (W - 1 - j) + 63 W zero bytes instead of (W - 1 - j).  The same W lookups per step as
// plain slicing-by-W, coalesced loads, no staging.  Rules:
//   head   the bytes of the first piece in front of the block's start are read (same allocation, aligned) and masked to zero;
//   pad    the piece count is rounded up to a multiple of 64 with zero pieces IN FRONT (not loaded; they leave the zero register
//          alone), so every lane's last piece is in the same, last row;
//   lanes  after its last piece lane l is (63 - l) W bytes from the end of the aligned part and its tables have skipped 63 W: the six
//          butterfly steps multiply by x^(8 W d), d = 1, 2, .. 32 (wavefront-uniform), and ONE multiplication by the constant
//          x^(-8 * 63 W) takes the surplus back (x is invertible: the polynomial's constant term is 1);
//   tail   the block's last (end mod W) bytes go through the register one by one;
//   ends   + 0xFFFFFFFF * x^(8 n) + 0xFFFFFFFF.
// Reads: [start & ~(W - 1), end) only.
//
// Compiles for the host too (tests/crc32core/: the same functions, the 64 lanes as a loop, against zlib.crc32; CPU suite).
#ifndef VTX_CRC32_CORE_H
#define VTX_CRC32_CORE_H

#include <stdint.h>

#ifdef __HIPCC__
#define VTXC_FN __host__ __device__ __forceinline__ constexpr
#define VTXC_DEV __device__ __forceinline__
#else
#define VTXC_FN static inline constexpr
#define VTXC_DEV static inline
#endif

namespace vtxc {

constexpr uint32_t POLY = 0xEDB88320u;      // reflected: bit 31 is x^0, bit 0 is x^31
constexpr uint32_t ONE = 0x80000000u;       // the polynomial 1

VTXC_FN uint32_t mulx(uint32_t v) { return (v >> 1) ^ ((v & 1u) ? POLY : 0u); }                           // v * x
VTXC_FN uint32_t divx(uint32_t v) { return (v & ONE) ? (((v ^ POLY) << 1) | 1u) : (v << 1); }              // v * x^-1 (mulx undone)
VTXC_FN uint32_t mulmod(uint32_t a, uint32_t b) {                                                          // a * b
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) { if (a & (ONE >> i)) p ^= b; b = mulx(b); }
    return p;
}
VTXC_FN uint32_t xpow8(uint64_t n) {                                                                       // x^(8 n), square and multiply
    uint32_t r = ONE, sq = 0x00800000u;      // x^8
    for (; n; n >>= 1) { if (n & 1u) r = mulmod(r, sq); sq = mulmod(sq, sq); }
    return r;
}
VTXC_FN uint32_t xinvpow8(uint32_t n) {                                                                    // x^(-8 n): compile-time constants only
    uint32_t r = ONE;
    for (uint32_t i = 0; i < 8 * n; ++i) r = divx(r);
    return r;
}
// zlib's crc32_combine: the CRC of A || B from the CRCs of A and B (finished ones: the all-ones terms cancel)
VTXC_FN uint32_t combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return mulmod(crc_a, xpow8(len_b)) ^ crc_b; }
// the raw register after one byte from a zero register (the classic table's entry)
VTXC_FN uint32_t byte_reg(uint32_t b) { for (int i = 0; i < 8; ++i) b = mulx(b); return b; }
// one byte through the register
VTXC_FN uint32_t step_byte(uint32_t reg, uint32_t b) { return (reg >> 8) ^ byte_reg((reg ^ b) & 0xffu); }

// ---- per slicing width W (bytes per lane and step) ----
template <int W> struct Consts {
    static_assert(W == 4 || W == 8 || W == 16, "slicing width");
    uint32_t tab_mul[W];        // table j: a byte followed by (W - 1 - j) + 63 W zero bytes
    uint32_t lane_mul[6];       // butterfly step d = 1 << k: x^(8 W d)
    uint32_t unskip;            // x^(-8 * 63 W)
};
template <int W> VTXC_FN Consts<W> make_consts() {
    Consts<W> c{};
    for (int j = 0; j < W; ++j) c.tab_mul[j] = xpow8((uint64_t)(W - 1 - j) + 63u * W);
    for (int k = 0; k < 6; ++k) c.lane_mul[k] = xpow8((uint64_t)W << k);
    c.unskip = xinvpow8(63u * W);
    return c;
}
constexpr int TABLE_WORDS(int W) { return W * 256; }
// entry i of the W tables (table i >> 8, byte value i & 255): the kernel's workgroup fills LDS with these once
template <int W> VTXC_FN uint32_t table_entry(uint32_t i) {
    constexpr Consts<W> K = make_consts<W>();
    return mulmod(byte_reg(i & 255u), K.tab_mul[i >> 8]);
}

// How a block [s, e) (offsets into the inflated buffer, whose base is W-aligned) is cut: wavefront-uniform.
struct Cut {
    uint64_t a0;          // address of real piece 0 (s rounded down to W)
    uint32_t head;        // bytes of piece 0 in front of s (masked)
    uint32_t n_pieces;    // real pieces: [a0, a0 + W n_pieces) ends at the last W-aligned address <= e (0: everything is tail)
    uint32_t rows;        // ceil(n_pieces / 64)
    uint32_t pad;         // zero pieces in front: 64 rows - n_pieces
    uint64_t tail_begin;  // [tail_begin, e): bytes that go through the register one by one (< W of them, or the whole of a tiny block)
};
template <int W> VTXC_FN Cut cut_block(uint64_t s, uint64_t e) {
    Cut c{};
    c.a0 = s & ~(uint64_t)(W - 1);
    const uint64_t e0 = e & ~(uint64_t)(W - 1);
    c.head = (uint32_t)(s - c.a0);
    c.n_pieces = e0 > s ? (uint32_t)((e0 - c.a0) / W) : 0u;
    c.rows = (c.n_pieces + 63u) / 64u;
    c.pad = c.rows * 64u - c.n_pieces;
    c.tail_begin = c.n_pieces ? e0 : s;
    return c;
}

template <int W> VTXC_DEV void load_piece(const uint8_t* p, uint32_t (&w)[W / 4]) {      // p is W-aligned
    __builtin_memcpy(w, __builtin_assume_aligned(p, W), W);
}
// one step of a lane: W bytes through the register, then 63 W zero bytes (the tables' doing)
template <int W> VTXC_DEV uint32_t step_piece(uint32_t reg, uint32_t (&w)[W / 4], const uint32_t* tab) {
    w[0] ^= reg;
    uint32_t r = 0;
    for (int j = 0; j < W; ++j) r ^= tab[j * 256 + ((w[j >> 2] >> (8 * (j & 3))) & 0xffu)];
    return r;
}
// a lane's share of the aligned part: its register after its last piece and the 63 W zero bytes behind it
template <int W> VTXC_DEV uint32_t lane_pieces(const uint8_t* data, const Cut& c, uint32_t lane, const uint32_t* tab) {
    uint32_t reg = 0;
    for (uint32_t r = 0; r < c.rows; ++r) {
        const uint32_t g = r * 64u + lane;
        if (g < c.pad) continue;                     // (row 0 only)
        const uint32_t k = g - c.pad;
        uint32_t w[W / 4];
        load_piece<W>(data + c.a0 + (uint64_t)W * k, w);
        if (k == 0 && c.head) {                      // (reg is still 0 here: the lane's earlier pieces were padding)
            for (int q = 0; q < W / 4; ++q) {        // (constant indices: w stays in registers)
                const int nb = (int)c.head - 4 * q;
                if (nb >= 4) w[q] = 0; else if (nb > 0) w[q] &= 0xffffffffu << (8 * nb);
            }
        }
        reg = step_piece<W>(reg, w, tab);
    }
    return reg;
}
// butterfly step k of the 64 lanes (d = 1 << k): what the lane with bit d set makes of its partner's register (lane ^ d) and its own
template <int W> VTXC_DEV uint32_t lane_join(uint32_t partner, uint32_t own, int k) {
    constexpr Consts<W> K = make_consts<W>();
    return mulmod(partner, K.lane_mul[k]) ^ own;
}
// from lane 63's register after the six steps to the block's CRC
template <int W> VTXC_DEV uint32_t finish_block(uint32_t joined, const uint8_t* data, const Cut& c, uint64_t s, uint64_t e) {
    constexpr Consts<W> K = make_consts<W>();
    uint32_t reg = c.n_pieces ? mulmod(joined, K.unskip) : 0u;
    for (uint64_t p = c.tail_begin; p < e; ++p) reg = step_byte(reg, data[p]);
    return reg ^ mulmod(0xFFFFFFFFu, xpow8(e - s)) ^ 0xFFFFFFFFu;
}

#ifndef __HIPCC__
// The wavefront as a loop (host builds: tests): the same cut, lane, join and finish functions the kernel calls.
template <int W> static inline uint32_t block_crc_host(const uint8_t* data, uint64_t s, uint64_t e, const uint32_t* tab) {
    const Cut c = cut_block<W>(s, e);
    uint32_t v[64];
    for (uint32_t l = 0; l < 64; ++l) v[l] = lane_pieces<W>(data, c, l, tab);
    for (int k = 0; k < 6; ++k) {
        uint32_t nv[64];
        for (uint32_t l = 0; l < 64; ++l) nv[l] = (l & (1u << k)) ? lane_join<W>(v[l ^ (1u << k)], v[l], k) : v[l];
        for (uint32_t l = 0; l < 64; ++l) v[l] = nv[l];
    }
    return finish_block<W>(v[63], data, c, s, e);
}
#endif

}  // namespace vtxc
#endif
