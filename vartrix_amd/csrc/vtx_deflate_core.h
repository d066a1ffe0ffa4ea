// vtx_deflate_core.h — a DEFLATE encoder (RFC 1951) in BGZF framing (a gzip member per chunk, RFC 1952 + the BC extra field) by ONE
// WAVEFRONT per chunk: the lane and wavefront logic of mtx_deflate_kernel (vtx_deflate.hip), which compresses the Matrix-Market text
// the device has formatted (vtx_write_mtx_gz) before it leaves the card.  The reference writes plain text only; the gzip form is what
// the readers of a 10x matrix directory take.
//
// One chunk (at most CHUNK = 65 280 bytes, BGZF's payload size) becomes one member:
//   18 header bytes   1f 8b 08 04 00 00 00 00 00 ff 06 00 'B' 'C' 02 00 BSIZE-1 (u16)
//   one DEFLATE block (BFINAL = 1): stored, fixed-Huffman or dynamic-Huffman, whichever is shortest in whole bytes
//   CRC32, ISIZE      (the CRC comes from the caller: vtx_crc32_core.h's wavefront functions)
// A member is never longer than n + 31 bytes (the stored form): it always fits its slot of SLOT bytes and BSIZE.
//
// Matching (LZ77 inside the chunk only: members are independent).  The wavefront takes 64 consecutive positions per step; lane l has
// position p = base + l.  A multiplicative hash of the 4 bytes at p indexes a table of 16-bit positions in LDS.  The DEFINED ORDER:
//   1. every lane reads its bucket as the previous steps left it (positions < base);
//   2. a lane whose hash an EARLIER lane of this step shares takes the nearest such lane's position instead (so runs and the repeats
//      from one text line to the next, distances < 64, are found);
//   3. of the lanes of this step that share a hash only the LAST writes the bucket — one writer per bucket, no race;
//   4. every lane checks its one candidate (distance <= 32 768, the 4 bytes equal) and extends it up to min(258, n - p);
//   5. selection is greedy and wave-serial over the ballot of the lanes that hold a match: the first position not covered by an
//      accepted match emits its match if it has one, else its literal; `skip` carries a match's cover into the next step.
// Nothing depends on lane timing: the host build (the 64 lanes as a loop) and the kernel produce the same bytes.
//
// Coding.  Histograms of the literal/length and distance symbols in LDS (atomic adds); length-limited Huffman codes (Moffat's in-place
// minimum-redundancy lengths on the rank-sorted frequencies, then the Kraft fix-up known from miniz: <= 15 bits, <= 7 for the
// code-length code); an alphabet with fewer than two used symbols gets symbols 0 / 1 added so that every code is COMPLETE (no used
// distance code: codes 0 and 1 of one bit each) — every inflater accepts that.  The dynamic header lists the HLIT + HDIST lengths one
// by one (no run-length symbols 16 / 17 / 18).  The three forms' sizes follow from the histograms alone, so the form and BSIZE are
// known before a bit is emitted.
//
// Emission.  Per step 64 tokens: each lane's bits (<= 48: code, extra, code, extra), an exclusive wave scan of the bit counts, atomic
// ORs into a window of 32-bit words in LDS, whole words out with coalesced stores.  Header and trailer go through the same writer.
//
// Every loop is bounded by the chunk length or a constant; none waits on another lane or wavefront.
//
// Compiles for the host too (tests/deflatecore/): the same text, the 64 lanes as a loop — VTXD_LANES(l) is that loop, Lanes<T> a
// value per lane, and only the cross-lane primitives at the top differ.
#ifndef VTX_DEFLATE_CORE_H
#define VTX_DEFLATE_CORE_H

#include <stdint.h>

#ifdef __HIPCC__
#define VTXD_DEV __device__ __forceinline__
#define VTXD_MEM __device__ __forceinline__
#define VTXD_NLANE 1
#define VTXD_LANES(l) for (uint32_t l = vtxd::lane_id(), l##_once = 1; l##_once; l##_once = 0)
#define VTXD_SYNC() __syncthreads()      /* the workgroup IS the wavefront */
#else
#define VTXD_DEV static inline
#define VTXD_MEM inline
#define VTXD_NLANE 64
#define VTXD_LANES(l) for (uint32_t l = 0; l < 64; ++l)
#define VTXD_SYNC() ((void)0)
#endif

namespace vtxd {

constexpr uint32_t CHUNK = 65280;                 // payload bytes per member (htslib's BGZF_BLOCK_SIZE - slack: 0xff00)
constexpr uint32_t HEADER = 18, TRAILER = 8;
constexpr uint32_t SLOT = 65312;                  // >= CHUNK + 31, a multiple of 16: a chunk's fixed-stride place for its member
constexpr uint32_t HASH_BITS = 13, HASH_SIZE = 1u << HASH_BITS;
constexpr uint32_t MAX_MATCH = 258, MIN_MATCH = 4, MAX_DIST = 32768;
constexpr uint32_t LL = 0, NLL = 286, DS = 288, NDS = 30, CL = 320, NCL = 19, NSYM = 352;      // alphabets in one index space
constexpr uint32_t WIN_WORDS = 100;               // 31 + 64 * 48 bits and a word to spare
constexpr uint32_t NOHASH = 0xffffffffu, NONE = 0xffffffffu;
enum Form { STORED = 0, FIXED = 1, DYNAMIC = 2 };

// the first 16 header bytes of every member, little-endian
constexpr uint64_t HEAD_LO = 0x0000000004088b1full, HEAD_HI = 0x000243420006ff00ull;
// the 28-byte empty member that ends a BGZF file (host code only)
constexpr uint8_t EOF_BLOCK[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

template <class T> struct Lanes {
    T v[VTXD_NLANE];
    VTXD_MEM T& operator[](uint32_t l) { return v[VTXD_NLANE == 1 ? 0 : l]; }
    VTXD_MEM const T& operator[](uint32_t l) const { return v[VTXD_NLANE == 1 ? 0 : l]; }
};

// ---- cross-lane primitives ----
#ifdef __HIPCC__
VTXD_DEV uint32_t lane_id() { return threadIdx.x & 63u; }
VTXD_DEV uint64_t ballot(const Lanes<uint32_t>& p) { return __ballot(p.v[0] != 0); }
VTXD_DEV uint32_t bcast(const Lanes<uint32_t>& x, uint32_t src) { return (uint32_t)__shfl((int)x.v[0], (int)src); }      // src: wavefront-uniform
VTXD_DEV uint32_t excl_scan(Lanes<uint32_t>& x) {                                        // in place; returns the total
    const uint32_t own = x.v[0], l = lane_id();
    uint32_t inc = own;
    for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)inc, d); if (l >= d) inc += t; }
    x.v[0] = inc - own;
    return (uint32_t)__shfl((int)inc, 63);
}
VTXD_DEV void lds_add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
VTXD_DEV void lds_or(uint32_t* p, uint32_t v) { atomicOr(p, v); }
#else
static inline uint64_t ballot(const Lanes<uint32_t>& p) { uint64_t m = 0; for (uint32_t l = 0; l < 64; ++l) if (p.v[l]) m |= 1ull << l; return m; }
static inline uint32_t bcast(const Lanes<uint32_t>& x, uint32_t src) { return x.v[src & 63u]; }
static inline uint32_t excl_scan(Lanes<uint32_t>& x) { uint32_t s = 0; for (uint32_t l = 0; l < 64; ++l) { const uint32_t o = x.v[l]; x.v[l] = s; s += o; } return s; }
static inline void lds_add(uint32_t* p, uint32_t v) { *p += v; }
static inline void lds_or(uint32_t* p, uint32_t v) { *p |= v; }
#endif

VTXD_DEV uint32_t ld32(const uint8_t* p) { uint32_t x; __builtin_memcpy(&x, p, 4); return x; }
VTXD_DEV uint64_t ld64(const uint8_t* p) { uint64_t x; __builtin_memcpy(&x, p, 8); return x; }
VTXD_DEV uint32_t hash4(uint32_t x) { return (x * 2654435761u) >> (32 - HASH_BITS); }
VTXD_DEV uint32_t log2u(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }          // x > 0
VTXD_DEV uint32_t popc64(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }
VTXD_DEV uint32_t ctz64(uint64_t x) { return (uint32_t)__builtin_ctzll(x); }              // x != 0

// ---- the symbol tables of RFC 1951 3.2.5 as arithmetic ----
VTXD_DEV uint32_t len_sym(uint32_t L) {            // L = length - 3 (0 .. 255)
    if (L < 8) return 257 + L;
    if (L == 255) return 285;
    const uint32_t e = log2u(L) - 2;
    return 261 + 4 * e + ((L >> e) & 3u);
}
VTXD_DEV uint32_t len_extra(uint32_t sym) { return (sym < 265 || sym == 285) ? 0u : (sym - 261) >> 2; }        // sym: 257 .. 285
VTXD_DEV uint32_t dist_sym(uint32_t D) {           // D = distance - 1 (0 .. 32767)
    if (D < 4) return D;
    const uint32_t e = log2u(D) - 1;
    return 2 * (e + 1) + ((D >> e) & 1u);
}
VTXD_DEV uint32_t dist_extra(uint32_t sym) { return sym < 4 ? 0u : (sym >> 1) - 1; }
VTXD_DEV uint32_t fixed_len(uint32_t sym) { return sym < 144 ? 8u : sym < 256 ? 9u : sym < 280 ? 7u : 8u; }
VTXD_DEV uint32_t cl_order(uint32_t j) {           // the order in which the code-length code's lengths are listed
    return j < 3 ? 16 + j : j == 3 ? 0 : (j & 1u) ? 8 - ((j - 3) >> 1) : 8 + ((j - 4) >> 1) + 0u;      // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
}
VTXD_DEV uint32_t rev_bits(uint32_t c, uint32_t n) { uint32_t r = 0; for (uint32_t i = 0; i < n; ++i) { r = (r << 1) | (c & 1u); c >>= 1; } return r; }

// a token: a literal (its byte) or TOK_MATCH | (length - 3) | (distance - 1) << 8
constexpr uint32_t TOK_MATCH = 0x80000000u;

// The wavefront's LDS (host: plain arrays).
struct Lds {
    uint16_t* hash;       // HASH_SIZE positions, 0xffff = empty
    uint32_t* freq;       // NSYM
    uint32_t* key;        // 288: sort / Moffat work
    uint16_t* sym;        // 288
    uint16_t* code;       // NSYM: bit-reversed codes
    uint8_t* len;         // NSYM
    uint32_t* win;        // WIN_WORDS
    uint32_t* misc;       // 40: counts per length, next code per length
};
#define VTXD_LDS_DECL(Q) Q uint16_t d_hash[vtxd::HASH_SIZE]; Q uint32_t d_freq[vtxd::NSYM]; Q uint32_t d_key[288]; Q uint16_t d_sym[288]; \
    Q uint16_t d_code[vtxd::NSYM]; Q uint8_t d_len[vtxd::NSYM]; Q uint32_t d_win[vtxd::WIN_WORDS]; Q uint32_t d_misc[40]; \
    const vtxd::Lds lds{d_hash, d_freq, d_key, d_sym, d_code, d_len, d_win, d_misc};

// ---- the bit writer: bits [0, bitpos) of the member are settled; whole words are in `out`, the open word is win[0] ----
struct BitW { uint32_t* out; uint32_t bitpos; };

// every lane appends nb[l] bits (<= 48; v[l] has no bit above them), lane 0's first
VTXD_DEV void put(const Lds& lds, BitW& bw, const Lanes<uint64_t>& v, const Lanes<uint32_t>& nb) {
    Lanes<uint32_t> off = nb;
    const uint32_t total = excl_scan(off);
    const uint32_t r = bw.bitpos & 31u, wbase = bw.bitpos >> 5;
    VTXD_LANES(l) {
        if (nb[l]) {
            const uint32_t b = r + off[l], w = b >> 5, s = b & 31u;
            const uint64_t lo = v[l] << s;
            const uint32_t hi = s ? (uint32_t)(v[l] >> (64 - s)) : 0u;
            if ((uint32_t)lo) lds_or(&lds.win[w], (uint32_t)lo);
            if (lo >> 32) lds_or(&lds.win[w + 1], (uint32_t)(lo >> 32));
            if (hi) lds_or(&lds.win[w + 2], hi);
        }
    }
    VTXD_SYNC();
    const uint32_t nfull = (r + total) >> 5;       // <= WIN_WORDS - 3
    Lanes<uint32_t> part;
    VTXD_LANES(l) {
        for (uint32_t i = l; i < nfull; i += 64) { if (wbase + i < SLOT / 4) bw.out[wbase + i] = lds.win[i]; lds.win[i] = 0; }      // (the bound never binds: the size is known beforehand)
        part[l] = lds.win[nfull];
    }
    VTXD_SYNC();
    VTXD_LANES(l) if (l == 0) { lds.win[nfull] = 0; lds.win[0] = part[l]; }
    VTXD_SYNC();
    bw.bitpos += total;
}
// lanes [0, count) append nbits bits each of what f(lane) gives
#define VTXD_PUT_EACH(count, nbits, expr) do { Lanes<uint64_t> pv_; Lanes<uint32_t> pn_; \
    VTXD_LANES(l) { pn_[l] = l < (uint32_t)(count) ? (uint32_t)(nbits) : 0u; pv_[l] = l < (uint32_t)(count) ? (uint64_t)(expr) : 0ull; } \
    put(lds, bw, pv_, pn_); } while (0)

// ---- Huffman: lengths of alphabet [base, base + nsym) from lds.freq, at most maxbits, complete, at least two symbols ----
// returns the number of symbols that have a code
VTXD_DEV uint32_t build_lengths(const Lds& lds, uint32_t base, uint32_t nsym, uint32_t maxbits) {
    // used symbols, and the first of them
    uint32_t nu = 0, first = NONE;
    for (uint32_t s0 = 0; s0 < nsym; s0 += 64) {
        Lanes<uint32_t> u;
        VTXD_LANES(l) u[l] = (s0 + l < nsym && lds.freq[base + s0 + l]) ? 1u : 0u;
        const uint64_t m = ballot(u);
        if (m && first == NONE) first = s0 + ctz64(m);
        nu += popc64(m);
    }
    const bool f0 = nu == 0 || (nu == 1 && first != 0), f1 = nu == 0 || (nu == 1 && first == 0);     // symbols added to make two
    const uint32_t n = nu < 2 ? 2 : nu;
    // rank sort by (frequency, symbol): one writer per rank
    VTXD_LANES(l) {
        for (uint32_t s = l; s < nsym; s += 64) {
            lds.len[base + s] = 0;
            const uint32_t f = lds.freq[base + s];
            if (!(f || (s == 0 && f0) || (s == 1 && f1))) continue;
            uint32_t r = 0;
            for (uint32_t t = 0; t < nsym; ++t) {
                const uint32_t g = lds.freq[base + t];
                if (!(g || (t == 0 && f0) || (t == 1 && f1))) continue;
                if (g < f || (g == f && t < s)) ++r;
            }
            lds.key[r] = f;
            lds.sym[r] = (uint16_t)s;
        }
    }
    VTXD_SYNC();
    VTXD_LANES(l) if (l == 0) {
        uint32_t* A = lds.key;
        // Moffat & Katajainen, in-place calculation of minimum-redundancy code lengths (A ascending, n >= 2)
        A[0] += A[1];
        uint32_t root = 0, leaf = 2;
        for (uint32_t next = 1; next + 1 < n; ++next) {
            if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; } else A[next] = A[leaf++];
            if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; } else A[next] += A[leaf++];
        }
        A[n - 2] = 0;
        for (int32_t next = (int32_t)n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
        int32_t avbl = 1, used = 0, dpth = 0, rt = (int32_t)n - 2, nx = (int32_t)n - 1;
        while (avbl > 0) {
            while (rt >= 0 && (int32_t)A[rt] == dpth) { ++used; --rt; }
            while (avbl > used) { A[nx--] = (uint32_t)dpth; --avbl; }
            avbl = 2 * used; ++dpth; used = 0;
        }
        // counts per length, the lengths above maxbits folded into it; then the Kraft fix-up
        uint32_t* cnt = lds.misc;
        for (uint32_t i = 0; i <= maxbits; ++i) cnt[i] = 0;
        for (uint32_t i = 0; i < n; ++i) cnt[A[i] < maxbits ? A[i] : maxbits] += 1;
        uint32_t total = 0;
        for (uint32_t i = maxbits; i > 0; --i) total += cnt[i] << (maxbits - i);
        while (total > (1u << maxbits)) {                                        // (each round takes one unit off)
            cnt[maxbits] -= 1;
            for (uint32_t i = maxbits - 1; i > 0; --i) if (cnt[i]) { cnt[i] -= 1; cnt[i + 1] += 2; break; }
            total -= 1;
        }
        // the most frequent symbols get the shortest codes
        uint32_t j = n;
        for (uint32_t i = 1; i <= maxbits; ++i) for (uint32_t k = cnt[i]; k > 0; --k) lds.len[base + lds.sym[--j]] = (uint8_t)i;
    }
    VTXD_SYNC();
    return n;
}
// canonical codes (RFC 1951 3.2.2) of [base, base + nsym) from lds.len, stored bit-reversed: the stream is filled from bit 0
VTXD_DEV void assign_codes(const Lds& lds, uint32_t base, uint32_t nsym) {
    VTXD_LANES(l) if (l == 0) {
        uint32_t* cnt = lds.misc;
        uint32_t* nxt = lds.misc + 20;
        for (uint32_t i = 0; i < 16; ++i) cnt[i] = 0;
        for (uint32_t s = 0; s < nsym; ++s) cnt[lds.len[base + s]] += 1;
        cnt[0] = 0;
        uint32_t c = 0;
        for (uint32_t i = 1; i < 16; ++i) { c = (c + cnt[i - 1]) << 1; nxt[i] = c; }
        for (uint32_t s = 0; s < nsym; ++s) {
            const uint32_t n = lds.len[base + s];
            lds.code[base + s] = n ? (uint16_t)rev_bits(nxt[n]++, n) : (uint16_t)0;
        }
    }
    VTXD_SYNC();
}
// sum over s in [0, nsym) of freq[base + s] * weight(s): every lane returns it
#define VTXD_SUM(result, base, nsym, weight) do { Lanes<uint32_t> sv_; \
    VTXD_LANES(l) { uint32_t a_ = 0; for (uint32_t s = l; s < (uint32_t)(nsym); s += 64) a_ += lds.freq[(base) + s] * (uint32_t)(weight); sv_[l] = a_; } \
    result = excl_scan(sv_); } while (0)

// ---- matching: tokens of the chunk into tok[], histograms into lds.freq (LL and DS; the end-of-block symbol counted); returns the token count ----
VTXD_DEV uint32_t match_pass(const uint8_t* in, uint32_t n, uint32_t* tok, const Lds& lds) {
    uint32_t skip = 0, ntok = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t cnt = n - base < 64 ? n - base : 64;
        Lanes<uint32_t> h, cand, mlen, x4, last;
        VTXD_LANES(l) {
            const uint32_t p = base + l;
            h[l] = NOHASH; cand[l] = NONE; mlen[l] = 0; x4[l] = 0; last[l] = 1;
            if (p + 4 <= n) {
                x4[l] = ld32(in + p);
                h[l] = hash4(x4[l]);
                const uint32_t c = lds.hash[h[l]];
                if (c != 0xffffu) cand[l] = c;
            }
        }
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint32_t hj = bcast(h, j);
            VTXD_LANES(l) {
                if (hj == h[l] && hj != NOHASH) {
                    if (j < l) cand[l] = base + j;
                    else if (j > l) last[l] = 0;
                }
            }
        }
        VTXD_SYNC();
        VTXD_LANES(l) if (h[l] != NOHASH && last[l]) lds.hash[h[l]] = (uint16_t)(base + l);
        VTXD_LANES(l) {
            const uint32_t p = base + l, c = cand[l];
            if (c != NONE && p - c <= MAX_DIST && ld32(in + c) == x4[l]) {
                const uint32_t maxl = n - p < MAX_MATCH ? n - p : MAX_MATCH;
                uint32_t k = 4;
                bool open = true;
                while (open && k + 8 <= maxl) {
                    const uint64_t d = ld64(in + c + k) ^ ld64(in + p + k);
                    if (d) { k += ctz64(d) >> 3; open = false; } else k += 8;
                }
                while (open && k < maxl && in[c + k] == in[p + k]) ++k;
                mlen[l] = k;
            }
        }
        // greedy, wave-serial
        const uint64_t M = ballot(mlen);
        uint64_t start = 0;
        uint32_t pos = skip;
        while (pos < cnt) {
            const uint64_t rest = M >> pos;
            if (!rest) { start |= ~0ull << pos; pos = cnt; break; }
            const uint32_t j = pos + ctz64(rest);
            if (j > pos) start |= ((1ull << (j - pos)) - 1) << pos;
            start |= 1ull << j;
            pos = j + bcast(mlen, j);
        }
        if (cnt < 64) start &= (1ull << cnt) - 1;
        skip = pos > 64 ? pos - 64 : 0;
        VTXD_LANES(l) {
            if ((start >> l) & 1u) {
                const uint32_t p = base + l, at = ntok + popc64(start & ((1ull << l) - 1));
                if (mlen[l]) {
                    const uint32_t L = mlen[l] - 3, D = p - cand[l] - 1;
                    tok[at] = TOK_MATCH | L | (D << 8);
                    lds_add(&lds.freq[LL + len_sym(L)], 1u);
                    lds_add(&lds.freq[DS + dist_sym(D)], 1u);
                } else {
                    const uint32_t b = in[p];
                    tok[at] = b;
                    lds_add(&lds.freq[LL + b], 1u);
                }
            }
        }
        ntok += popc64(start);
    }
    VTXD_LANES(l) if (l == 0) lds.freq[LL + 256] = 1;
    VTXD_SYNC();
    return ntok;
}

// ---- one chunk -> one member at out (4-byte aligned, SLOT bytes); tok: CHUNK words of work space; returns the member's size ----
VTXD_DEV uint32_t encode_member(const uint8_t* in, uint32_t n, uint32_t crc, uint8_t* out, uint32_t* tok, const Lds& lds) {
    VTXD_LANES(l) {
        for (uint32_t i = l; i < HASH_SIZE; i += 64) lds.hash[i] = 0xffffu;
        for (uint32_t i = l; i < NSYM; i += 64) { lds.freq[i] = 0; lds.len[i] = 0; lds.code[i] = 0; }
        for (uint32_t i = l; i < WIN_WORDS; i += 64) lds.win[i] = 0;
    }
    VTXD_SYNC();
    const uint32_t ntok = match_pass(in, n, tok, lds);

    uint32_t extra, extra_d, fixed_bits, n_dist;
    VTXD_SUM(extra, LL + 257, 29, len_extra(257 + s));
    VTXD_SUM(extra_d, DS, NDS, dist_extra(s));
    VTXD_SUM(fixed_bits, LL, NLL, fixed_len(s));
    VTXD_SUM(n_dist, DS, NDS, 1);
    extra += extra_d;
    fixed_bits += 3 + 5 * n_dist + extra;

    build_lengths(lds, LL, NLL, 15);
    build_lengths(lds, DS, NDS, 15);
    // HLIT, HDIST: up to the last symbol that has a code
    uint32_t hlit = 257, hdist = 1;
    {
        Lanes<uint32_t> u;
        VTXD_LANES(l) u[l] = (257 + l < NLL && lds.len[LL + 257 + l]) ? 1u : 0u;
        uint64_t m = ballot(u);
        if (m) hlit = 257 + (64 - (uint32_t)__builtin_clzll(m));
        VTXD_LANES(l) u[l] = (l < NDS && lds.len[DS + l]) ? 1u : 0u;
        m = ballot(u);
        if (m) hdist = 64 - (uint32_t)__builtin_clzll(m);
    }
    VTXD_LANES(l) {
        for (uint32_t i = l; i < hlit + hdist; i += 64) lds_add(&lds.freq[CL + (i < hlit ? lds.len[LL + i] : lds.len[DS + i - hlit])], 1u);
    }
    VTXD_SYNC();
    build_lengths(lds, CL, NCL, 7);
    uint32_t hclen = 4;
    {
        Lanes<uint32_t> u;
        VTXD_LANES(l) u[l] = (l < NCL && lds.len[CL + cl_order(l < NCL ? l : 0)]) ? 1u : 0u;
        const uint64_t m = ballot(u);
        if (m && 64 - (uint32_t)__builtin_clzll(m) > 4) hclen = 64 - (uint32_t)__builtin_clzll(m);
    }
    uint32_t body, body_d, head;
    VTXD_SUM(body, LL, NLL, lds.len[LL + s]);
    VTXD_SUM(body_d, DS, NDS, lds.len[DS + s]);
    VTXD_SUM(head, CL, NCL, lds.len[CL + s]);
    const uint32_t dyn_bits = 3 + 14 + 3 * hclen + head + body + body_d + extra;

    const uint32_t stored_bytes = 5 + n, fixed_bytes = (fixed_bits + 7) >> 3, dyn_bytes = (dyn_bits + 7) >> 3;
    uint32_t form = DYNAMIC, best = dyn_bytes;
    if (fixed_bytes < best) { form = FIXED; best = fixed_bytes; }
    if (stored_bytes < best) { form = STORED; best = stored_bytes; }
    const uint32_t member = HEADER + best + TRAILER;

    if (form == FIXED) {
        VTXD_LANES(l) {
            for (uint32_t s = l; s < 288; s += 64) lds.len[LL + s] = (uint8_t)fixed_len(s);
            if (l < 32) lds.len[DS + l] = 5;
        }
        VTXD_SYNC();
        assign_codes(lds, LL, 288);
        assign_codes(lds, DS, 32);
    } else if (form == DYNAMIC) {
        assign_codes(lds, LL, NLL);
        assign_codes(lds, DS, NDS);
        assign_codes(lds, CL, NCL);
    }

    BitW bw{(uint32_t*)out, 0};
    const uint32_t bsize1 = member - 1;
    VTXD_PUT_EACH(HEADER, 8, l < 8 ? (HEAD_LO >> (8 * l)) & 0xffu : l < 16 ? (HEAD_HI >> (8 * (l - 8))) & 0xffu : (bsize1 >> (8 * (l - 16))) & 0xffu);
    if (form == STORED) {
        VTXD_PUT_EACH(3, l == 0 ? 8 : 16, l == 0 ? 1u : l == 1 ? n : (~n & 0xffffu));
        for (uint32_t base = 0; base < n; base += 256) {
            Lanes<uint64_t> v; Lanes<uint32_t> nb;
            VTXD_LANES(l) {
                const uint32_t k = base + 4 * l;
                uint32_t x = 0, m = 0;
                if (k < n) { m = n - k < 4 ? n - k : 4; for (uint32_t q = 0; q < m; ++q) x |= (uint32_t)in[k + q] << (8 * q); }
                v[l] = x; nb[l] = 8 * m;
            }
            put(lds, bw, v, nb);
        }
    } else {
        if (form == FIXED) VTXD_PUT_EACH(1, 3, 3u);
        else {
            VTXD_PUT_EACH(4 + hclen, l == 0 ? 3 : l < 3 ? 5 : l == 3 ? 4 : 3,
                          l == 0 ? 5u : l == 1 ? hlit - 257 : l == 2 ? hdist - 1 : l == 3 ? hclen - 4 : lds.len[CL + cl_order(l - 4 < NCL ? l - 4 : 0)]);
            for (uint32_t base = 0; base < hlit + hdist; base += 64) {
                Lanes<uint64_t> v; Lanes<uint32_t> nb;
                VTXD_LANES(l) {
                    const uint32_t i = base + l;
                    v[l] = 0; nb[l] = 0;
                    if (i < hlit + hdist) {
                        const uint32_t L = i < hlit ? lds.len[LL + i] : lds.len[DS + i - hlit];
                        v[l] = lds.code[CL + L]; nb[l] = lds.len[CL + L];
                    }
                }
                put(lds, bw, v, nb);
            }
        }
        for (uint32_t base = 0; base < ntok; base += 64) {
            Lanes<uint64_t> v; Lanes<uint32_t> nb;
            VTXD_LANES(l) {
                v[l] = 0; nb[l] = 0;
                if (base + l < ntok) {
                    const uint32_t t = tok[base + l];
                    if (t & TOK_MATCH) {
                        const uint32_t L = t & 0xffu, D = (t >> 8) & 0x7fffu, ls = len_sym(L), ds = dist_sym(D);
                        const uint32_t le = len_extra(ls), de = dist_extra(ds);
                        uint64_t x = lds.code[LL + ls];
                        uint32_t b = lds.len[LL + ls];
                        x |= (uint64_t)(L < 8 ? 0u : L & ((1u << le) - 1)) << b; b += le;
                        x |= (uint64_t)lds.code[DS + ds] << b; b += lds.len[DS + ds];
                        x |= (uint64_t)(D & ((1u << de) - 1)) << b; b += de;
                        v[l] = x; nb[l] = b;
                    } else {
                        v[l] = lds.code[LL + t]; nb[l] = lds.len[LL + t];
                    }
                }
            }
            put(lds, bw, v, nb);
        }
        VTXD_PUT_EACH(1, lds.len[LL + 256], lds.code[LL + 256]);
    }
    // to the byte boundary, then CRC32 and ISIZE
    const uint32_t pad = (0u - bw.bitpos) & 7u;
    VTXD_PUT_EACH(9, l == 0 ? pad : 8, l == 0 ? 0u : l < 5 ? (crc >> (8 * (l - 1))) & 0xffu : (n >> (8 * (l - 5))) & 0xffu);
    VTXD_LANES(l) if (l < ((bw.bitpos & 31u) >> 3) && (bw.bitpos >> 5) * 4 + l < SLOT) out[(bw.bitpos >> 5) * 4 + l] = (uint8_t)(lds.win[0] >> (8 * l));
    VTXD_SYNC();
    return (bw.bitpos >> 3) < SLOT ? bw.bitpos >> 3 : SLOT;       // == member
}

}  // namespace vtxd
#endif
